"""Every dropout mask of a wide-family launch (bcnf_wide.hip) against the host restatement of its two draw rules
(tests/dropout_ref.py wide_keep_bits), bit for bit.

The masks are read from the saved A / G records of one saving training forward (_wide_records of
tests/test_gpu_train_parity.py: kept iff the masked activation or derivative factor is nonzero) and compared with the
restatement over the whole [nv][NH][B][H] array: no unit is skipped and no difference is tolerated. A kept unit reads
as dropped only if its fp32 GELU and GELU' are both exactly zero, which needs a pre-activation far below the O(1) ones
of these weights (_perturb); a mismatch is therefore a finding. What the statistics of
assert_record_masks_are_independent_draws cannot see and this does: a mask that repeats every tile row, a counter
built from a tile-local row or column, a word picked by the wrong row of the group, a draw that depends on the GEMM
tiling the dispatcher picks or on the batch size, and an offset high half that never reaches the key.

Shapes: the WIDE cases the training-parity tests consume; WIDE_EDGE's [150] * 8 at B = 131 (the largest tag, two column
tiles with a ragged last one in every tiling, two row tiles, a ragged last row group); B = 1 and B = 3 (the row group
incomplete from row 0); every forced GEMM tiling; an offset with a nonzero high half (the seeds' high halves are
nonzero already); p = 1e-6, where the truncating threshold is 4294 and nearly every unit is kept, at a B large enough
that the restatement itself drops a few units; the folded forward; one FFTWideStack case."""
import functools
import types

import numpy as np
import pytest
import torch

from dropout_ref import wide_keep_bits
from test_gpu_train_parity import OFFSET, _wide_records, _workspace_records, wide_build, wide_case, wide_seed

pytestmark = pytest.mark.gpu

DEV = "cuda"
HIGH_OFFSET = (5 << 32) + 3
TILINGS = [-1, 0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 10]           # -1: the dispatcher's choice (tests/test_gpu_wide.py)
TILING_IDS = ["auto"] + [f"t{t}" for t in TILINGS[1:]]


@functools.lru_cache(maxsize=None)
def _restated(p, seed, offset, nv, NH, B, H):
    return np.stack([np.stack([wide_keep_bits(p, seed, offset, v, l, B, H) for l in range(NH)]) for v in range(nv)])


def restated(case, offset, B=None):
    """bool [nv][NH][B][H]: the masks of a B-row launch of the case at `offset`, from the host rule alone."""
    s = case.spec
    nv, H = s.n_blocks * (2 if s.two_way else 1), s.nested_sizes[0]
    assert all(h == H for h in s.nested_sizes)
    B = case.y.shape[0] if B is None else B
    return _restated(float(s.dropout), wide_seed(case), offset, nv, len(s.nested_sizes), B, H)


def assert_masks_are(got, want, what):
    """Exact equality of the whole array; on failure, how many units differ and where the first ones are."""
    got = got.cpu().numpy()
    assert got.shape == want.shape and got.dtype == want.dtype == np.bool_, (got.shape, want.shape)
    bad = np.argwhere(got != want)
    assert not len(bad), (what, f"{len(bad)} of {want.size} units differ; first (v, l, row, column):", bad[:8].tolist(),
                          "kept by the kernel only:", int((got & ~want).sum()))


def rows_of(case, B):
    """The case cut to its first B rows (the same model and seed)."""
    return types.SimpleNamespace(name=f"{case.name}-B{B}", m=case.m, spec=case.spec, sd=case.sd, y=case.y[:B],
                                 cond=case.cond[:B], wide=True)


NAMES = ["w96", "w40_two_way", "w24_c13", "fc_large_B64", "w150_nh8"]


@pytest.mark.parametrize("offset", [OFFSET, HIGH_OFFSET], ids=["offset3", "offset_high"])
@pytest.mark.parametrize("name", NAMES)
def test_every_mask_of_the_saving_forward(name, offset):
    """At OFFSET these are the masks the oracle of the training-parity tests is fed. (5 << 32) + 3 has the same low
    half: only through the key's `^ hi32(offset)` can it draw other masks, and the restatement says it does."""
    case = wide_case(name)
    want = restated(case, offset)
    if offset == HIGH_OFFSET:
        p = float(case.spec.dropout)                         # independent draws differ at 2 p (1 - p) of the units
        assert (want != restated(case, OFFSET)).mean() > p * (1 - p)
    got = case.masks if offset == OFFSET else _wide_records(case, offset)
    assert_masks_are(got, want, (name, hex(offset)))


@pytest.mark.parametrize("B", [1, 3])
def test_every_mask_of_a_launch_below_one_row_group(B):
    """B = 1 and B = 3 on w24_c13: the only row group is incomplete, and its draw is still that of rows 0 .. 3 of any
    larger launch (the restatement at B is the first B rows of the restatement at 37)."""
    case = wide_case("w24_c13")
    want = restated(case, OFFSET, B)
    assert np.array_equal(want, restated(case, OFFSET)[:, :, :B])
    assert_masks_are(_wide_records(rows_of(case, B), OFFSET), want, ("w24_c13", B))


@pytest.mark.parametrize("tiling", TILINGS, ids=TILING_IDS)
@pytest.mark.parametrize("name", ["w96", "w150_nh8"])
def test_every_mask_at_every_forced_tiling(name, tiling):
    """BcnfStackDesc.gemm_tiling = t + 1 forces tiling t for the chain GEMMs of the launch (as tests/test_gpu_wide.py
    does). The same step must train on the same masks whatever the dispatcher picks: one restated array for all."""
    case = wide_case(name)
    st = case.m.fused
    st.desc.gemm_tiling = tiling + 1
    try:
        got = _wide_records(case, OFFSET)
    finally:
        st.desc.gemm_tiling = 0
    assert_masks_are(got, restated(case, OFFSET), (name, tiling))


def test_every_mask_at_p_1e_6():
    """p = 1e-6: thresh = 4294 (truncated; 4295 rounded), so a launch that treated so small a p as zero, or as one
    16-bit step, would keep all or drop thousands. [96] * 3, nb = 3 at B = 4096 is 3.5 M units, of which the
    restatement at this (seed, offset) drops a handful -- asserted of the restatement, so the equality is not a
    comparison of two all-ones arrays."""
    shape = dict(size=19, nested_sizes=[96] * 3, n_blocks=3, n_conditions=24, dropout=1e-6, act_norm=True)
    case = wide_build("w96_p1e-6", shape, None, 4096)
    want = restated(case, HIGH_OFFSET)
    drops = want.size - int(want.sum())
    assert 1 <= drops <= 20, drops                           # expected 3.5
    assert_masks_are(_wide_records(case, HIGH_OFFSET), want, "p = 1e-6")


def test_every_mask_of_the_folded_forward():
    """launch_fold_nll_forward (the feature Linear folded into the condition projection) on w96: the fold changes how
    P is formed and nothing of the draw, and its workspace has the saving forward's layout."""
    case = wide_case("w96")
    m, st = case.m, case.m.fused
    y, cond = case.y.to(DEV), case.cond.to(DEV)
    m.train()
    st.rng_state()[1] = OFFSET
    with torch.no_grad():
        fold = m._wide_fold(y, (cond,))
        assert fold is not None
        x, lin = fold
        _, _, _, saved = st.launch_fold_nll_forward(y, x, lin.weight, lin.bias, True)
    assert int(st.rng_state()[1].item()) == OFFSET + 1
    assert_masks_are(_workspace_records(saved[0], case.spec, y.shape[0]), restated(case, OFFSET), "w96 folded")


def test_every_mask_of_an_fft_wide_stack():
    """An FFTWideStack runs the same kernels on its effective weights: cfg175 (H = 175, NH = 5, p = 0.407, B = 64)."""
    from test_gpu_variants_fp64 import fft_train_case
    case = fft_train_case("cfg175")
    assert type(case.m.fused).__name__ == "FFTWideStack"
    assert_masks_are(case.masks, restated(case, OFFSET), "cfg175")
