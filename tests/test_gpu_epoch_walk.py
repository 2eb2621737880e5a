"""The device pool and its epoch walk (bcnf_amd/epoch.py) against index_select, with no model: every gather is a copy,
so every comparison is bit for bit."""
import pytest
import torch

pytestmark = pytest.mark.gpu

DEV = "cuda"
N_ROWS, D, COND, X, BATCH = 37, 19, (30, 3), 90, 8


@pytest.fixture(scope="module")
def data():
    gen = torch.Generator().manual_seed(37)
    y = torch.randn(N_ROWS, D, generator=gen).to(DEV)
    cond = torch.randn(N_ROWS, *COND, generator=gen).to(DEV)
    perm = torch.randperm(N_ROWS, generator=gen).to(DEV)
    return y, cond, perm[:4 * BATCH], perm[4 * BATCH:]        # 4 whole batches and a ragged 5


@pytest.mark.parametrize("row_width", [92, None])
def test_walk_gathers_the_cursors_batch(data, row_width):
    from bcnf_amd import _native as N
    from bcnf_amd.epoch import DevicePool, EpochWalk
    y, cond, order, ragged = data
    pool = DevicePool(y, cond, row_width=row_width)
    width = row_width or X
    assert pool.cond.shape == ((N_ROWS, width) if row_width else (N_ROWS,) + COND)
    assert pool.cond_shape == ((COND, X) if row_width else None)
    walk = EpochWalk(pool, order, BATCH)
    assert (walk.n_batches, walk.batch, walk.host_cursor) == (4, BATCH, 0)
    assert walk.order.data_ptr() != order.data_ptr() and torch.equal(walk.order, order)
    for i in range(4):
        assert walk.cursor.item() == i
        want = order[i * BATCH:(i + 1) * BATCH]
        out = pool.empty_batch(BATCH)
        gy, gc = walk.gather(out)
        assert gy.data_ptr() == out[0].data_ptr() and torch.equal(gy, y[want])
        assert gc.shape == (BATCH,) + COND and torch.equal(gc, cond[want])
        assert gc.data_ptr() == out[1].data_ptr() and gc.stride(0) == width      # a view, no copy
        if row_width:
            assert out[1].shape == (BATCH, 92) and torch.count_nonzero(out[1][:, X:]) == 0
        # the deferred form: the same launch arguments, handed to the pack launch instead
        sy, sc, spec = walk.gather_spec(out)
        assert (sy.data_ptr(), sc.data_ptr()) == (gy.data_ptr(), gc.data_ptr())
        assert (spec.idx, spec.cursor, spec.n) == (walk.order.data_ptr(), walk.cursor.data_ptr(), BATCH)
        assert (spec.src0, spec.cols0, spec.dst0) == (pool.y.data_ptr(), D, out[0].data_ptr())
        assert (spec.src1, spec.cols1, spec.dst1) == (pool.cond.data_ptr(), width, out[1].data_ptr())
        # the walk never advances the cursor: the launch that ends a step does (bcnf_amd/optim.py)
        N.call("bcnf_advance_counters", None, walk.cursor, walk.n_batches, N.stream_handle(pool.device))
    assert walk.cursor.item() == 0

    ry, rc = pool.rows(ragged)
    assert torch.equal(ry, y[ragged]) and torch.equal(rc, cond[ragged])
    idx = order[5:5 + BATCH].contiguous()
    gy, gc = pool.gather_rows(idx)                              # the static-index gather (bcnf_gather_rows2)
    assert torch.equal(gy, y[idx]) and torch.equal(gc, cond[idx]) and gc.stride(0) == width
    _, _, spec = pool.gather_spec(idx, BATCH)
    assert (spec.idx, spec.cursor, spec.n) == (idx.data_ptr(), None, BATCH)

    walk.cursor.fill_(2)
    walk.host_cursor = 2
    walk.reset(order.flip(0))
    assert (walk.cursor.item(), walk.host_cursor) == (0, 0) and torch.equal(walk.order, order.flip(0))
    with pytest.raises(ValueError, match="keeps its order size"):
        walk.reset(order[:2 * BATCH])
    with pytest.raises(IndexError):
        walk.reset(order + N_ROWS)


def test_pool_refuses_other_device_tensors(data):
    from bcnf_amd.epoch import DevicePool, EpochWalk
    y, cond, order, _ = data
    for bad in (cond.double(), cond.transpose(1, 2)):
        with pytest.raises(ValueError, match="contiguous fp32 device tensors required"):
            DevicePool(y, bad)
    with pytest.raises(ValueError, match="whole number of batches"):
        EpochWalk(DevicePool(y, cond), order[:-3], BATCH)
