"""The host arithmetic of the device epoch walk (bcnf_amd/epoch.py) and of the gradient bucket's block ranges
(bcnf_amd/bucket.py): no GPU, no library."""
import pytest
import torch

from bcnf_amd.bucket import range_blocks
from bcnf_amd.epoch import DevicePool, check_indices, graph_schedule, whole_batches


@pytest.mark.parametrize("args, want", [
    ((20, 8, 2), [8, 8, 4]),
    ((7, 8, 2), [4, 2]),            # one batch left for a single replay
    ((1, 8, 2), []),
    ((0, 8, 2), []),
    ((11, 8, 1), [8, 2, 1]),
    ((3, 1, 1), [1, 1, 1]),
])
def test_graph_schedule_cases(args, want):
    assert graph_schedule(*args) == want


@pytest.mark.parametrize("smallest", [1, 2])
def test_graph_schedule_leaves_less_than_the_smallest_graph(smallest):
    for n in range(41):
        sizes = graph_schedule(n, 8, smallest)
        assert sum(sizes) <= n and n - sum(sizes) < smallest, (n, sizes)
        assert sizes == sorted(sizes, reverse=True) and set(sizes) <= {8, 4, 2, 1}, (n, sizes)


@pytest.mark.parametrize("args, want", [
    ((26, 4), [(20, 26), (13, 20), (6, 13), (0, 6)]),      # round() sends 6.5 to 6 and 19.5 to 20
    ((2, 2), [(1, 2), (0, 1)]),
    ((26, 1), [(0, 26)]),
])
def test_range_blocks_cases(args, want):
    assert range_blocks(*args) == want


def test_range_blocks_partition():
    for n_blocks in range(1, 33):
        for r in range(1, n_blocks + 1):
            ranges = range_blocks(n_blocks, r)
            assert all(lo < hi for lo, hi in ranges), (n_blocks, r, ranges)
            assert ranges[0][1] == n_blocks and ranges[-1][0] == 0, (n_blocks, r, ranges)
            # descending and gapless: each range ends where the one before it began
            assert all(b[1] == a[0] for a, b in zip(ranges, ranges[1:])), (n_blocks, r, ranges)


def test_check_indices():
    n = 37
    check_indices(torch.empty(0, dtype=torch.int64), n)
    check_indices(torch.tensor([0, n - 1]), n)
    for bad in (-1, n):
        with pytest.raises(IndexError, match=r"out of range \[0, 37\)"):
            check_indices(torch.tensor([3, bad, 5]), n)


def test_device_pool_refuses_other_tensors():
    good = torch.zeros(4, 3)
    for bad in (good, torch.zeros(3, 4).t(), good.double()):        # CPU; non-contiguous; float64
        with pytest.raises(ValueError, match="set_pool: contiguous fp32 device tensors required"):
            DevicePool(bad, good)
    with pytest.raises(ValueError, match=r"ValidationPass\.set_pool: contiguous fp32 device tensors required"):
        DevicePool(good, good.double(), who="ValidationPass.set_pool")


def test_epoch_walk_sizes():
    """EpochWalk takes its size rules from whole_batches (the walk itself needs a device pool)."""
    assert whole_batches(32, 8) == 4
    for numel in (37, 5, 0):
        with pytest.raises(ValueError, match="whole number of batches"):
            whole_batches(numel, 8)
    assert whole_batches(32, 8, keep=(4, 8)) == 4
    for numel, batch in ((24, 8), (32, 4)):                         # a reset with another size
        with pytest.raises(ValueError, match="keeps its order size"):
            whole_batches(numel, batch, keep=(4, 8))
