"""CPU checks that tie the GPU case lists of the register-resident coupling family (tests/test_gpu_train_parity.py,
test_gpu_dropout.py, test_gpu_parity.py, test_gpu_sample_logprob.py) to the host dispatch restated in
tests/small_arms.py, and that keep their inputs where the gates can see an error. No launch, no GPU.

 * Arm census: the lists reach every k_forward / k_backward / k_inverse / k_inverse_mfma arm the census names at every
   NH = 1 .. 8, and every registered branch; taking any one of the new cases out of its list leaves something unreached.
 * Raw table: bcnf_fold_raw_table_bytes accepts and refuses exactly what small_arms.raw_applicable says, and the
   table it builds gives every float of a forward record to exactly one (thread, slot).
 * Input conditions, on the fp64 oracle with the kernels' masks: every gated gradient tensor of a new training case
   stands clear of its gate's absolute floor, a 1 % change of any one coupling weight matrix moves z or ldj by many
   gates, and fp32 arithmetic reaches every gate with room to spare -- so a failure on the GPU is the kernel's."""
import ctypes

import numpy as np
import pytest
import torch

import small_arms as A
from dropout_ref import SMALL_TRAIN_FOLD_X, SMALL_TRAIN_GAIN, SMALL_TRAIN_RAW, SMALL_TRAIN_SHAPES
from oracle import cnf_oracle as O
from test_gpu_train_parity import (GRAD, INV_TAG, NEW_SMALL, OFFSET, TRAIN_INVERSE, VAL, _ratio, _small_keep, compare,
                                   oracle_run, small_reference)

# The cases this census was written for, by list: each must be needed by it.
NEW_SAMPLE_CASES = ["f_nh4_d24", "g_nh5_d25", "h_nh6_d20", "i_nh1_d23", "j_nh8_d3", "l_nh8_d22"]
NEW_ENTRIES = (
    [("shape", n) for n in SMALL_TRAIN_GAIN]
    + [("SMALL", ("nh6_d20_c129", 133)), ("SMALL", ("nh4_d31_c208", 133))]
    + [("TRAIN_INVERSE", (n, B)) for n, B, _ in TRAIN_INVERSE if n in SMALL_TRAIN_GAIN or n == "d32_nh1"]
    + [("FOLD_EVAL", (n, 37)) for n, raw in SMALL_TRAIN_RAW.items() if raw]
    + [("OTHER_SHAPES", i) for i in (4, 5, 6)]
    + [("CASES", n) for n in NEW_SAMPLE_CASES] + [("POSITION_CASES", n) for n in ("g_nh5_d25", "h_nh6_d20")])


def _without(rs, entry):
    source, key = entry
    if source == "shape":            # a shape taken out of SMALL_TRAIN_SHAPES leaves every training list
        shape = SMALL_TRAIN_SHAPES[key]
        return [r for r in rs if not (r.kind in A.TRAIN_KINDS and r.shape is shape)]
    if source == "SMALL":            # one (shape, B) of SMALL: its steps and its no-save forward
        return [r for r in rs if not (r.source == "SMALL" and r.key == key[0] and r.B == key[1])]
    if source == "CASES":            # a sampling case taken out of CASES leaves the position list too
        return [r for r in rs if not (r.source in ("CASES", "POSITION_CASES") and r.key == key)]
    return [r for r in rs if not (r.source == source and r.key == key)]


# ------------------------------------------------------------------------------------------ arm census
def test_case_lists_reach_every_arm_and_branch():
    assert len(A.required_arms()) == 8 * (4 + 2) + 4 * 2
    assert A.missing(A.runs()) == []


@pytest.mark.parametrize("entry", NEW_ENTRIES, ids=lambda e: f"{e[0]}-{e[1]}")
def test_every_new_case_is_needed(entry):
    rs = A.runs()
    rest = _without(rs, entry)
    assert len(rest) < len(rs), entry
    assert A.missing(rest) != [], entry


def test_new_shapes_are_inside_the_envelope_at_its_edges():
    """layout_supported admits each shape; the record sizes named beside the cases are the restated ones."""
    for name, shape in SMALL_TRAIN_SHAPES.items():
        assert A.layout_supported(A.layout(shape)), name
    L = A.layout(SMALL_TRAIN_SHAPES["nh4_d24_c17"])
    assert (L.Da, L.Db, L.Cp) == (12, 12, 32) and A.perm(L) and not A.vec_rows(L.C)
    L = A.layout(SMALL_TRAIN_SHAPES["nh5_d25_c128"])
    assert (L.Da, L.Db) == (13, 12) and not A.perm(L) and L.C == A.KC
    L = A.layout(SMALL_TRAIN_SHAPES["nh6_d20_c129"])
    assert (L.Da, L.Db, L.NKp, L.C) == (10, 10, 128, A.KC + 1)
    assert A.layout(SMALL_TRAIN_SHAPES["nh4_d31_c208"]).Cp == 208
    from test_gpu_sample_logprob import CASES
    assert A.layout(CASES["l_nh8_d22"][0]).PMB == 3792 <= A.RING
    assert A.layout(CASES["i_nh1_d23"][0]).PMB == 7 * 256 + 96


# ------------------------------------------------------------------------------------------ raw table
def _desc(shape):
    from bcnf_amd import _native as N
    return N.make_desc(shape["size"], list(shape["nested_sizes"]), shape["n_blocks"], shape["n_conditions"],
                       shape.get("dropout", 0.1), shape.get("act_norm", True))


def _raw_status(shape, X):
    from bcnf_amd import _native as N
    nb = ctypes.c_int64(0)
    return N.lib().bcnf_fold_raw_table_bytes(ctypes.byref(_desc(shape)), X, ctypes.byref(nb)), nb.value


def _stack(D, nested, C=80, nb=3, act_norm=True):
    return dict(size=D, nested_sizes=nested, n_blocks=nb, n_conditions=C, dropout=0.1, act_norm=act_norm)


RAW_PAIRS = [        # (accepted, refused) one step apart
    ((_stack(19, [16] * 7), 96), (_stack(19, [16] * 7), 97)),
    ((_stack(19, [16] * 7, C=128), 90), (_stack(19, [16] * 7, C=129), 90)),
    ((_stack(19, [16] * 7, nb=2), 90), (_stack(19, [16] * 7, nb=1), 90)),
    ((_stack(22, [16] * 5), 90), (_stack(23, [16] * 5), 90)),
    ((_stack(19, [16] * 7), 90), (_stack(19, [16] * 7, act_norm=False), 90)),
]


@pytest.mark.parametrize("ok,bad", RAW_PAIRS, ids=["X", "C", "nb", "D", "act_norm"])
def test_raw_table_limits(ok, bad):
    from bcnf_amd import _native as N
    assert _raw_status(*ok)[0] == N.OK and A.raw_applicable(A.layout(ok[0]), ok[1])
    assert _raw_status(*bad)[0] == N.ERR_UNSUPPORTED and not A.raw_applicable(A.layout(bad[0]), bad[1])


@pytest.mark.parametrize("name", list(SMALL_TRAIN_RAW))
def test_raw_table_status_of_the_folded_shapes(name):
    from bcnf_amd import _native as N
    shape, X = SMALL_TRAIN_SHAPES[name], SMALL_TRAIN_FOLD_X[name]
    want = N.OK if SMALL_TRAIN_RAW[name] else N.ERR_UNSUPPORTED
    assert _raw_status(shape, X)[0] == want
    assert A.raw_applicable(A.layout(shape), X) == SMALL_TRAIN_RAW[name]
    nb = ctypes.c_int64(0)                                                         # the fold itself applies to all four
    assert X % 3 == 0 and N.lib().bcnf_fold_bytes(ctypes.byref(_desc(shape)), X, ctypes.byref(nb)) == N.OK


RAW_SWEEP = ([(_stack(D, [w] * NH), 90) for D in range(16, 23) for NH in range(1, 9) for w in (16, 12)]
             + [(SMALL_TRAIN_SHAPES[n], SMALL_TRAIN_FOLD_X[n]) for n, raw in SMALL_TRAIN_RAW.items() if raw])


def test_raw_table_gives_every_record_float_to_one_thread_slot():
    """bcnf_fold_raw_table over the sweep: the library accepts exactly the layouts the restatement accepts; of an
    accepted one, the destinations of the non-padding forward entries are 0 .. 16 RF - 1, each once; a padding entry
    names the last float of the ring slot (and source 0); P sources lie inside one block's parameters, Q sources
    inside one D x D matrix."""
    from bcnf_amd import _native as N
    accepted = 0
    for shape, X in RAW_SWEEP:
        L = A.layout(shape)
        rc, nbytes = _raw_status(shape, X)
        assert (rc == N.OK) == A.raw_applicable(L, X), (shape, rc)
        if rc != N.OK:
            assert rc == N.ERR_UNSUPPORTED
            continue
        accepted += 1
        assert nbytes == 4 * (A.RAW_NSP * A.WG + 16 * L.RB), shape
        raw = np.zeros(nbytes // 4, dtype=np.uint32)
        assert N.lib().bcnf_fold_raw_table(ctypes.byref(_desc(shape)), X, ctypes.c_void_p(raw.ctypes.data)) == N.OK
        t = raw[:A.RAW_NSP * A.WG].reshape(A.WG, A.RAW_NSP)            # [thread][slot]
        assert (t[:, A.RAW_NP + A.RAW_NQ + A.RAW_NZ:] == A.RAW_DUMMY).all()      # the slots past RAW_NS: padding
        t = t[:, :A.RAW_NP + A.RAW_NQ + A.RAW_NZ]
        dst, src = (t & 4095).astype(np.int64), (t >> 12).astype(np.int64)
        live = dst != A.RAW_DUMMY
        assert (src[~live] == 0).all()
        assert np.array_equal(np.sort(dst[live]), np.arange(16 * L.RF)), shape
        n_p, n_q, n_z = A.raw_counts(L)
        p, q, z = slice(0, A.RAW_NP), slice(A.RAW_NP, A.RAW_NP + A.RAW_NQ), slice(A.RAW_NP + A.RAW_NQ, None)
        assert (int(live[:, p].sum()), int(live[:, q].sum()), int(live[:, z].sum())) == (n_p, n_q, n_z), shape
        assert src[:, p][live[:, p]].max() < L.blk_stride
        assert src[:, q][live[:, q]].max() < L.D * L.D
        assert len(np.unique(src[:, p][live[:, p]])) == n_p and len(np.unique(src[:, q][live[:, q]])) == n_q
    assert accepted >= 20, accepted
    # the folded shape at every limit: 484 of the 512 Q slots, the widest record
    L = A.layout(SMALL_TRAIN_SHAPES["fold_nh8_d22"])
    assert A.raw_counts(L)[1] == 484 and L.NH == A.MAX_HIDDEN


# ------------------------------------------------------------------------------------------ input conditions
COND_IDS = [f"{n}-B{B}" for n, B in NEW_SMALL]
MIN_GRAD = 5e-3          # max|ref| of a gated gradient tensor: the 1e-4 floor of its gate is <= 2 % of it
MIN_MOVE = 10.0          # gates z or ldj move by under a 1 % change of one coupling weight matrix
MAX_FP32 = 0.5           # of any gate the float32 oracle may use


@pytest.mark.parametrize("name,B", NEW_SMALL, ids=COND_IDS)
def test_gradients_stand_clear_of_the_gate_floor(name, B):
    ref = small_reference(name, B).ref
    tensors = dict(ref["grads"], dy=ref["dy"], dh=ref["dh"])
    low = {k: float(v.abs().max()) for k, v in tensors.items() if float(v.abs().max()) < MIN_GRAD}
    assert not low, low


@pytest.mark.parametrize("name,B", NEW_SMALL, ids=COND_IDS)
def test_one_percent_of_any_coupling_weight_moves_z_or_ldj(name, B):
    case = small_reference(name, B)
    keep = _small_keep(case, OFFSET, B)
    sd64 = {k: v.double() for k, v in case.sd.items()}
    with torch.no_grad():
        h = O.feature_forward(sd64, case.spec, case.cond.double()) if case.spec.feature_sizes else case.cond.double()
        weights = [k for k, v in sd64.items()
                   if k.startswith("layers.") and v.dim() == 2 and not k.endswith("orthonormal_matrix")]
        assert len(weights) == case.spec.n_blocks * (len(case.spec.nested_sizes) + 1)
        moves = {}
        for k in weights:
            z, ldj = O.model_forward(dict(sd64, **{k: sd64[k] * 1.01}), case.spec, case.y.double(), h, training=True,
                                     keep=keep)
            moves[k] = max(_ratio(z, case.ref["z"], **VAL), _ratio(ldj, case.ref["ldj"], **VAL))
    worst = min(moves, key=moves.get)
    assert moves[worst] >= MIN_MOVE, (worst, moves[worst])


@pytest.mark.parametrize("name,B", NEW_SMALL, ids=COND_IDS)
def test_float32_arithmetic_reaches_every_gate(name, B):
    case = small_reference(name, B)
    rows = compare(oracle_run(case, _small_keep(case, OFFSET, B), dtype=torch.float32), case.ref)
    over = [(k, round(r, 3)) for k, ok, r in rows if not r <= MAX_FP32]
    assert not over, over


NEW_INVERSE = [(n, B, tol) for n, B, tol in TRAIN_INVERSE if n in SMALL_TRAIN_GAIN or n == "d32_nh1"]


@pytest.mark.parametrize("name,B,tol", NEW_INVERSE, ids=[f"{n}-B{B}" for n, B, _ in NEW_INVERSE])
def test_float32_arithmetic_reaches_the_training_inverse_gate(name, B, tol):
    """The training-mode inverse of test_small_training_mode_inverse_vs_fp64_oracle on the oracle in float32, with
    the masks of the inverse's tag: within half the gate of the float64 one."""
    case = small_reference(name, 37)
    spec = case.spec
    zl = torch.randn(B, spec.size, generator=torch.Generator().manual_seed(B))
    keep = _small_keep(case, OFFSET, B, INV_TAG)
    out = {}
    for dt in (torch.float64, torch.float32):
        sd = {k: v.to(dt) for k, v in case.sd.items()}
        with torch.no_grad():
            out[dt] = O.model_inverse(sd, spec, zl.to(dt), case.cond[:B].to(dt), training=True, keep=keep)
    assert _ratio(out[torch.float32], out[torch.float64], tol, tol) <= MAX_FP32
    assert GRAD["floor"] == 1e-4 and VAL["floor"] == 1e-5           # the gates these conditions were worked out for
