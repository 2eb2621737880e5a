"""CPU checks that tie the GPU case lists of the feature kernels (tests/test_gpu_dlstm.py, tests/test_gpu_transformer.py,
tests/test_gpu_cnn.py) to the host dispatch and planners restated in tests/feature_plans.py. No launch, no GPU.

 * Work bytes: the restated wgrad_plan and ln_plan against the built library's own byte counts (host functions, called
   as tests/test_fold_tail_plan.py calls its plan). bcnf_conv_block_work_bytes is nwg YS P 4: it shows nwg, YS and P
   (so COP and tpp) but NOT the band height BR nor the chunk width GWC -- those two, and everything derived from them
   (chunks, ragged, bands, shrinks), rest on the restatement alone, as does tile_plan.
 * Arm census: the arms the case lists reach are ALL the arms of LSTM_DISPATCH, ATTN_DISPATCH, LN_DISPATCH and
   CONV_K_DISPATCH, and every registered branch is reached. Taking a case out of a list fails here.
 * Near ties: the float64 activations of every conv case have few enough near-tied pooling windows for the validated
   winners of test_gpu_cnn.py to decide nothing else (its NEAR_TIE_CAP, a condition on the inputs)."""
import pytest

import feature_plans as F
from test_gpu_cnn import CONV_CASES, NEAR_TIE_CAP, conv_reference
from test_gpu_dlstm import LSTM_CASES
from test_gpu_transformer import ATTN_CASES, LN_CAP_CASES, LN_D, LN_NULLABLE_CASE, LN_ROWS

LN_CASES = [(rows, d) for rows in LN_ROWS for d in LN_D] + list(LN_CAP_CASES) + [LN_NULLABLE_CASE]


def conv_id(c):
    return "x".join(map(str, c))


# ------------------------------------------------------------------------------------------ work bytes
@pytest.mark.parametrize("p", [0.0, 0.5])
@pytest.mark.parametrize("case", CONV_CASES, ids=conv_id)
def test_conv_work_bytes_equal_the_restated_plan(case, p):
    from bcnf_amd import _native as N
    plan = F.conv_wgrad_plan(case)
    assert N.query_i64("bcnf_conv_block_work_bytes", *case, p) == plan.nwg * plan.YS * plan.P * 4
    # the restatement's own invariants: the chunks cover GW and the bands 2 HP, within the kernel's LDS
    _, ci, _, _, _, K, _, _ = case
    hp = F.conv_dims(case)[2]
    assert plan.GWC % K == 0 and plan.GW % K == 0 and 1 <= plan.YS <= plan.BR
    assert (plan.chunks - 1) * plan.GWC < plan.GW <= plan.chunks * plan.GWC
    assert (plan.bands - 1) * plan.BR < 2 * hp <= plan.bands * plan.BR
    assert (plan.COP * plan.BR * plan.GWC + ci * (plan.BR + K - 1) * (plan.GWC + K)) * 4 <= F.WGRAD_LDS_BYTES
    assert plan.tpp * plan.YS <= F.CWG and plan.passes * plan.tpp >= (plan.COP // F.WCB) * ci * K


@pytest.mark.parametrize("rows,d", LN_CASES)
def test_layernorm_work_bytes_equal_the_restated_plan(rows, d):
    from bcnf_amd import _native as N
    rpw, nwg = F.ln_plan(rows, d)
    assert N.query_i64("bcnf_add_layernorm_work_bytes", rows, d) == nwg * 2 * d * 4
    assert (nwg - 1) * rpw < rows <= nwg * rpw and nwg <= F.LN_MAX_WG


def test_work_bytes_of_refused_shapes():
    """Where the restated dispatch has no arm the library refuses: the two agree on the limits."""
    from bcnf_amd import _native as N
    assert F.ln_arm(1025) is None and N.query_status("bcnf_add_layernorm_work_bytes", 4, 1025)[0] == N.ERR_ARG
    assert F.ln_arm(1024) == 16 and N.query_status("bcnf_add_layernorm_work_bytes", 4, 1024)[0] == N.OK
    assert F.conv_k_arm(9) is None
    assert N.query_status("bcnf_conv_block_work_bytes", 2, 1, 12, 12, 4, 9, 3, 3, 0.0)[0] == N.ERR_ARG


# ------------------------------------------------------------------------------------------ arm census
def test_lstm_cases_reach_every_arm_and_branch():
    assert len(F.LSTM_ARMS) == 8
    assert {F.lstm_arm(H) for _, _, H, _ in LSTM_CASES} == F.LSTM_ARMS
    for label, reaches in F.LSTM_BRANCHES.items():
        assert any(reaches(c) for c in LSTM_CASES), label
    assert {dirs for *_, dirs in LSTM_CASES} == {1, 2}


def test_attention_cases_reach_every_arm_and_branch():
    assert len(F.ATTN_ARMS) == 8
    assert {F.attn_arm(S, hd) for _, S, _, hd in ATTN_CASES} == F.ATTN_ARMS
    for label, reaches in F.ATTN_BRANCHES.items():
        assert any(reaches(c) for c in ATTN_CASES), label


def test_layernorm_cases_reach_every_arm_and_branch():
    assert len(F.LN_ARMS) == 5
    assert {F.ln_arm(d) for d in LN_D} == F.LN_ARMS                      # the full cross product alone
    for label, reaches in F.LN_BRANCHES.items():
        assert any(reaches(c) for c in LN_CASES), label
    # the cap: above 8192 rows a workgroup's four waves take more than two rows each
    assert len(LN_CAP_CASES) == 2
    for rows, d in LN_CAP_CASES:
        assert F.ln_plan(rows, d) == (9, 911) and rows > F.LN_MAX_WG * F.LN_MIN_RPW
    assert max(F.ln_plan(rows, d)[0] for rows in LN_ROWS for d in LN_D) <= F.LN_MIN_RPW
    assert F.ln_plan(*LN_NULLABLE_CASE) == (8, 8)


def test_conv_cases_reach_every_arm_and_branch():
    assert len(F.CONV_K_ARMS) == 8
    assert {F.conv_k_arm(c[5]) for c in CONV_CASES} == F.CONV_K_ARMS
    for label, (case, reaches) in F.CONV_BRANCHES.items():
        assert case in CONV_CASES, label
        assert reaches(case, F.conv_wgrad_plan(case), F.conv_forward_tiles(case), F.conv_backward_tiles(case)), label


def test_conv_branch_cases_by_their_plan_fields():
    """The plan of each case named for a branch, written out."""
    w = F.conv_wgrad_plan((1025, 1, 4, 5, 3, 2, 0, 1))
    assert (w.nwg, w.chunks, w.bands, w.passes) == (512, 1, 1, 1)       # workgroup 0: images 0, 512, 1024
    w = F.conv_wgrad_plan((1, 32, 8, 160, 32, 3, 1, 1))
    assert (w.GW, w.GWC, w.chunks, w.ragged, w.BR, w.bands, w.passes) == (162, 42, 4, 36, 4, 2, 3)
    assert w.shrinks == ("br", "gwc", "gwc")
    assert F.conv_forward_tiles((1, 32, 8, 160, 32, 3, 1, 1)) == F.TilePlan(4, 16, 5, 1, 24, 2)
    w = F.conv_wgrad_plan((1, 32, 8, 50, 32, 5, 2, 2))
    assert (w.GW, w.GWC, w.chunks, w.ragged, w.passes) == (50, 25, 2, 0, 5) and w.GWC % 2 == 1
    assert F.conv_forward_tiles((1, 32, 8, 50, 32, 5, 2, 2)).rounds == 4
    w = F.conv_wgrad_plan((1, 32, 15, 16, 32, 3, 1, 1))
    assert (w.BR, w.bands, w.chunks) == (7, 2, 1) and w.BR % 2 == 1
    w = F.conv_wgrad_plan((1, 32, 40, 24, 32, 8, 7, 7))
    assert w.shrinks == ("br", "br", "gwc_k") and (w.GWC, w.BR, w.bands, w.passes, w.chunks) == (16, 4, 12, 8, 2)
    case = (1, 20, 37, 150, 32, 7, 3, 3)
    w = F.conv_wgrad_plan(case)
    assert (w.GW, w.GWC, w.chunks, w.ragged, w.bands, w.passes) == (154, 42, 4, 28, 9, 5)
    f, b = F.conv_forward_tiles(case), F.conv_backward_tiles(case)
    assert (f.tiles_y, f.tiles_x, f.rounds) == (5, 5, 2) and (b.tiles_y, b.tiles_x, b.rounds) == (5, 5, 3)
    # the earlier lists' only chunked case splits evenly in two, and nothing in them has tiles and rounds together
    w = F.conv_wgrad_plan((2, 1, 90, 160, 8, 8, 3, 3))
    assert (w.GW, w.GWC, w.chunks, w.ragged) == (160, 80, 2, 0)


# ------------------------------------------------------------------------------------------ near ties
@pytest.mark.parametrize("p", [0.0, 0.5])
@pytest.mark.parametrize("case", CONV_CASES, ids=conv_id)
def test_conv_cases_have_few_near_ties(case, p):
    R = conv_reference(case, p)
    assert R["positive"] > 0 or case[0] * case[4] * R["dy"].shape[2] * R["dy"].shape[3] == 1    # the single window
    assert R["near"] <= NEAR_TIE_CAP * R["positive"], (R["near"], R["positive"])
