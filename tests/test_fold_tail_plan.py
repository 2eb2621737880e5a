"""CPU checks of bcnf_fold_tail_plan: the host arithmetic that spreads the folded tail's slab reduce over its three
launches (k_fold_tail, k_fold_gx, k_fold_finish). bcnf_fold_backward_tail computes its grids from the same function,
so a hole or an overlap in the ranges here is a gradient never written or written twice there. No launch, no GPU."""
import ctypes

import pytest

RED_FLOATS = 4 * 32           # slab floats per reduce workgroup (RED_O4 float4, bcnf_stack_tail.hip)

# (nested_sizes, n_blocks, n_conditions, in_features)
DESCS = {
    "fc_small": ([16] * 7, 32, 80, 90),
    "one_block": ([16], 1, 13, 21),
    "two_blocks": ([16], 2, 13, 21),
    "wide_x": ([16] * 3, 5, 96, 237),
}
BATCHES = [1, 16, 17, 128, 129, 4096]


def _plan(nested, nb, C, X, B):
    from bcnf_amd import _native as N
    d = N.make_desc(19, nested, nb, C, 0.1, True)
    out = (ctypes.c_int64 * 14)(*([-1] * 14))
    rc = N.lib().bcnf_fold_tail_plan(ctypes.byref(d), X, B, out)
    return rc, [int(v) for v in out]


@pytest.mark.parametrize("B", BATCHES)
@pytest.mark.parametrize("name", sorted(DESCS))
def test_plan_covers_the_reduce_once(name, B):
    from bcnf_amd import _native as N
    nested, nb, C, X = DESCS[name]
    rc, out = _plan(nested, nb, C, X, B)
    assert rc == N.OK
    n_red, S = out[0], out[1]
    ranges = [(out[2 + 2 * t], out[3 + 2 * t]) for t in range(3)]
    grids, own = out[8:11], out[11:14]
    assert n_red >= 1 and (n_red - 1) * RED_FLOATS < S <= n_red * RED_FLOATS
    # contiguous, in order, [0, n_red) exactly once (empty ranges allowed: fewer reduce workgroups than launches)
    nxt = 0
    for first, count in sorted(ranges):
        assert count >= 0 and first == nxt, ranges
        nxt = first + count
    assert nxt == n_red and sum(c for _, c in ranges) == n_red
    for t in range(3):
        assert own[t] >= 1 and grids[t] == own[t] + ranges[t][1]
    # the launches' own workgroups, from the shapes: split-K (blocks in pairs x 128-row splits) + the copy workgroup,
    # the Gx sum (one thread per element of [nb*16][Xp]), the finish tiles ((nb + Xp/16) x Cp/16)
    Xp, Cp = (X + 1 + 15) // 16 * 16, (C + 15) // 16 * 16
    assert own == [(nb + 1) // 2 * ((B + 127) // 128) + 1, (nb * 16 * Xp + 255) // 256, (nb + Xp // 16) * (Cp // 16)]
    # the slab stride and the reduce's size do not depend on the batch
    assert _plan(nested, nb, C, X, 1)[1][:2] == [n_red, S]


def test_plan_headline_shape():
    """FC_small at B = 4096: 628 reduce workgroups over an 80,384-float stride; 513 / 192 / 190 own workgroups."""
    rc, out = _plan(*DESCS["fc_small"], 4096)
    assert rc == 0 and out[:2] == [628, 80384] and out[11:14] == [513, 192, 190]


def test_plan_rejects_bad_arguments():
    from bcnf_amd import _native as N
    lib = N.lib()
    nested, nb, C, X = DESCS["fc_small"]
    for B in (0, -1):
        assert _plan(nested, nb, C, X, B)[0] == N.ERR_ARG
    out = (ctypes.c_int64 * 14)()
    d = N.make_desc(19, nested, nb, C, 0.1, True)
    assert lib.bcnf_fold_tail_plan(None, X, 16, out) == N.ERR_ARG
    assert lib.bcnf_fold_tail_plan(ctypes.byref(d), X, 16, None) == N.ERR_ARG
    bad = N.make_desc(0, nested, nb, C, 0.1, True)           # no size
    assert lib.bcnf_fold_tail_plan(ctypes.byref(bad), X, 16, out) == N.ERR_ARG
    bad = N.make_desc(19, nested, 0, C, 0.1, True)           # no blocks
    assert lib.bcnf_fold_tail_plan(ctypes.byref(bad), X, 16, out) == N.ERR_ARG
