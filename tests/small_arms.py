"""The host dispatch of the register-resident coupling family (bcnf_stack*.hip) restated in plain Python: which template
arm a (shape, mode, path) launches -- launch_forward, launch_backward, launch_inverse, launch_inverse_logdet, vec_rows,
raw_applicable with build_raw_table's capacity checks, and the record sizes of make_layout / round_rec they rest on.
No GPU and no library: tests/test_small_arms_cpu.py holds the restatement to the library's own statuses and table, and
holds the GPU files' case lists (imported in runs()) to the arm set and the branch registry below.

NH is the parameter the kernels' compile-time schedules hang on (ActRec<NH>, rf_stage_q<NH>, BwdJobs<NH>, the two
dropout float4, the backward's derivative slot), so every arm of dispatch_nh is different code. A new arm or branch is
registered HERE, and the census then fails until a case of the GPU lists reaches it."""
from collections import namedtuple

KC = 128                       # rows / columns of one split-K chunk (k_hp, dw1h_body, W1H_ROWS_PER_SPLIT)
RING = 4096                    # floats of a record-ring slot (STAGE_REC * BCNF_WG * 4)
WG = 256                       # BCNF_WG
RAW_NP, RAW_NQ, RAW_NZ = 10, 2, 6
RAW_NSP = 20                   # (RAW_NP + RAW_NQ + RAW_NZ + 3) & ~3
RAW_DUMMY = RING - 1
RAW_KP, RAW_TPW = 100, 2
MAX_HIDDEN = 8

Layout = namedtuple("Layout", "D Da Db NH H C Cp nb act_norm p RF RB PMB NKp an_size blk_stride")


def round_rec(n):
    """A multiple of 4 floats with an odd quotient."""
    n = (n + 3) & ~3
    return n + 4 if (n // 4) % 2 == 0 else n


def layout(shape):
    """make_layout of a model-kwargs dict (size, nested_sizes, n_blocks, n_conditions, dropout, act_norm)."""
    D, H, C = shape["size"], list(shape["nested_sizes"]), shape["n_conditions"]
    Da, Db, NH = (D + 1) // 2, D // 2, len(H)
    widths = [Da + C] + H + [2 * Db]                            # Linear l: widths[l - 1] (l = 1: Da + C) -> widths[l]
    ins = [Da + C] + H
    params = sum(i * o + o for i, o in zip(ins, widths[1:]))
    an = 2 * D if shape.get("act_norm") else 0
    rf_t = 24 + 17 * (NH - 1)
    rf_q = (rf_t + 17 + 17 + 3) & ~3
    return Layout(D=D, Da=Da, Db=Db, NH=NH, H=H, C=C, Cp=max(16, (C + 15) // 16 * 16), nb=shape["n_blocks"],
                  act_norm=bool(shape.get("act_norm")), p=float(shape.get("dropout", 0.0)),
                  RF=round_rec(rf_q + 64), RB=round_rec(100 + 16 * (NH - 1) + 16),
                  PMB=(NH + 6) * 256 + (NH - 1) * 16 + 96, NKp=(shape["n_blocks"] * 16 + 63) // 64 * 64,
                  an_size=an, blk_stride=an + params)


def layout_supported(L):
    return (1 <= L.NH <= MAX_HIDDEN and L.Da <= 16 and L.Db <= 16 and all(1 <= h <= 16 for h in L.H)
            and 1 <= L.C and L.Cp <= 256 and 16 * L.RF <= RING and 16 * L.RB <= RING)


# ------------------------------------------------------------------------------------------ dispatch
def fwd_dispatch(L, training, save, raw=False):
    """k_forward<NH, DROP, SAVE, RAW>; the pack-free form always saves."""
    assert save or not raw
    return ("k_forward", L.NH, bool(training and L.p > 0.0), bool(save), bool(raw))


def bwd_dispatch(L):
    return ("k_backward", L.NH)


def perm(L):
    return L.Da <= 12 and L.Db <= 12


def inv_dispatch(L, training):
    """k_inverse<NH> where masks are drawn, else the matrix-core inverse k_inverse_mfma<NH, PERM, false> (layout_matches
    holds the record size and PMB of every layout to the kernel's compile-time offsets)."""
    if training and L.p > 0.0:
        return ("k_inverse", L.NH)
    return ("k_inverse_mfma", L.NH, perm(L), False)


def inv_ldj_dispatch(L):
    return ("k_inverse_mfma", L.NH, perm(L), True)


def vec_rows(ld):
    """float4 row loads of the condition (or, folded, the x) rows: the row stride in floats is a multiple of 4 (a
    torch allocation's base is 16-byte aligned)."""
    return ld % 4 == 0


def raw_counts(L):
    """(P-sourced, Q-sourced, zero) entries of a block's forward record [16 lanes][RF]: the P entries are a block's
    parameters without the W1 condition columns, the Q entries all of Q_k."""
    n_p = L.blk_stride - L.H[0] * L.C
    n_q = L.D * L.D
    return n_p, n_q, 16 * L.RF - n_p - n_q


def raw_applicable(L, X):
    """raw_applicable and the capacity checks of build_raw_table: whether bcnf_fold_raw_table_bytes answers OK."""
    if not (layout_supported(L) and 1 <= X <= RAW_KP - 4 and L.C <= 64 * RAW_TPW and L.nb >= 2 and L.act_norm):
        return False
    n_p, n_q, n_z = raw_counts(L)
    return (16 * L.RF <= RAW_DUMMY and L.an_size <= WG and n_p <= RAW_NP * WG and n_q <= RAW_NQ * WG
            and n_z <= RAW_NZ * WG)


# ------------------------------------------------------------------------------------------ the GPU lists as runs
# One launch group of a GPU test: kind (below), the list entry it comes from (source, key), the model kwargs, rows,
# the path of a training step, the gain on the coupling weights and in_features of a folded feature Linear (or None).
Run = namedtuple("Run", "kind source key shape B path gain X")
TRAIN_KINDS = ("step", "nosave", "masks", "train_inverse", "fold_eval")


def arms(r):
    """The template arms the launches of run r take."""
    L = layout(r.shape)
    if r.kind == "step":            # unfused / fused / folded training step: saving forward + backward
        raw = r.path == "folded_raw" or (r.path == "folded" and raw_applicable(L, r.X))
        return {fwd_dispatch(L, True, True, raw), bwd_dispatch(L)}
    if r.kind == "nosave":          # the training forward with and without grad
        return {fwd_dispatch(L, True, True), fwd_dispatch(L, True, False)}
    if r.kind == "masks":           # launch_forward(training, save)
        return {fwd_dispatch(L, True, True)}
    if r.kind == "train_inverse":
        return {inv_dispatch(L, True)}
    if r.kind == "fold_eval":       # the pack-free folded step of a model in eval mode
        return {fwd_dispatch(L, False, True, True), bwd_dispatch(L)}
    if r.kind == "eval_shape":      # test_other_shapes_vs_oracle: forward with and without grad, backward, inverse
        return {fwd_dispatch(L, False, True), fwd_dispatch(L, False, False), bwd_dispatch(L), inv_dispatch(L, False)}
    if r.kind in ("logprob", "position"):     # stack_inverse with want_ldj True and (logprob) False
        return {inv_ldj_dispatch(L)} | ({inv_dispatch(L, False)} if r.kind == "logprob" else set())
    raise ValueError(r.kind)


def runs():
    """Every small-family run of the GPU case lists, imported from the files that run them."""
    from conftest import FC_SMALL_CFG
    from dropout_ref import SMALL_TRAIN_FOLD_X, SMALL_TRAIN_GAIN, SMALL_TRAIN_SHAPES
    import test_gpu_dropout as TD
    import test_gpu_parity as TP
    import test_gpu_sample_logprob as TS
    import test_gpu_train_parity as TT

    def shape_of(name):
        return FC_SMALL_CFG["model"]["kwargs"] if name == "fc_small" else SMALL_TRAIN_SHAPES[name]

    def train(kind, source, key, name, B, path=None):
        X = 90 if name == "fc_small" else SMALL_TRAIN_FOLD_X.get(name)
        return Run(kind, source, key, shape_of(name), B, path, SMALL_TRAIN_GAIN.get(name, 1.0), X)

    out = [train("step", "SMALL", n, n, B, p) for n, B, p in TT.SMALL_PATHS]
    out += [train("nosave", "SMALL", n, n, B) for n, B in TT.SMALL]
    out += [train("train_inverse", "TRAIN_INVERSE", (n, B), n, B) for n, B, _ in TT.TRAIN_INVERSE]
    out += [train("fold_eval", "FOLD_EVAL", (n, B), n, B, "folded_raw") for n, B in TT.FOLD_EVAL]
    out += [train("masks", "MASK_CASES", n, n, 37) for n in TD.MASK_CASES]
    out += [Run("eval_shape", "OTHER_SHAPES", i, dict(s, dropout=0.0), 37, None, g, None)     # m.eval(): no masks
            for i, (s, g) in enumerate(TP.OTHER_SHAPES)]
    # FC_small in eval mode on the g1 weights: test_ragged_batches_vs_oracle (forward without grad, inverse) and
    # test_eval_grads_match_reference (saving forward, backward)
    out += [Run("eval_shape", "RAGGED_B", B, dict(shape_of("fc_small"), dropout=0.0), B, None, 1.0, None)
            for B in TP.RAGGED_B]
    for n in TS.SMALL:
        kw = shape_of("fc_small") if TS.CASES[n][0] is None else TS.CASES[n][0]
        out += [Run("logprob", "CASES", n, dict(kw, dropout=0.0), B, None, TS.GAIN.get(n, 1.0), None) for B in TS.ROWS[n]]
    for n in TS.POSITION_CASES:
        if n in TS.SMALL:
            kw = shape_of("fc_small") if TS.CASES[n][0] is None else TS.CASES[n][0]
            out.append(Run("position", "POSITION_CASES", n, dict(kw, dropout=0.0), 300, None, TS.GAIN.get(n, 1.0), None))
    return out


# ------------------------------------------------------------------------------------------ what the lists must reach
def required_arms():
    """Every arm the host can dispatch a supported small-family layout to, as far as the census asks for it."""
    need = set()
    for NH in range(1, MAX_HIDDEN + 1):
        need |= {("k_forward", NH, d, s, False) for d in (False, True) for s in (False, True)}
        need |= {("k_backward", NH), ("k_inverse", NH)}
        if NH >= 5:                  # the pack-free form; its table also builds at NH < 5, where no GPU case runs it yet
            need |= {("k_forward", NH, d, True, True) for d in (False, True)}
    return need


def _step(r):
    return r.kind == "step"


def _L(r):
    return layout(r.shape)


# label -> predicate over a Run: the shape edges and input conditions a case list must keep reaching
BRANCHES = {
    "12 / 12 (the last PERM layout) in training, fed rows that are not 16-byte aligned":
        lambda r: _step(r) and r.X is None and (_L(r).Da, _L(r).Db) == (12, 12) and not vec_rows(_L(r).C),
    "13 / 12 (the first non-PERM layout) in training at C = KC":
        lambda r: _step(r) and (_L(r).Da, _L(r).Db) == (13, 12) and _L(r).C == KC,
    "10 / 10 without the broadcast form in training": lambda r: _step(r) and _L(r).D == 20,
    "C = KC + 1 in training": lambda r: _step(r) and _L(r).C == KC + 1 and r.B <= KC,
    "C = KC + 1 in training, past KC rows": lambda r: _step(r) and _L(r).C == KC + 1 and r.B > KC,
    "C = 208 in training": lambda r: _step(r) and _L(r).C == 208 and r.B <= KC,
    "C = 208 in training, past KC rows": lambda r: _step(r) and _L(r).C == 208 and r.B > KC,
    "16 / 15 in training": lambda r: _step(r) and (_L(r).Da, _L(r).Db) == (16, 15),
    "C = 1, Da = 2, Db = 1, no ActNorm in training":
        lambda r: _step(r) and _L(r).C == 1 and _L(r).D == 3 and not _L(r).act_norm,
    "uneven hidden widths at NH = 5 in training": lambda r: _step(r) and _L(r).NH == 5 and len(set(_L(r).H)) > 2,
    "NH = 8 at D = 19 in training at a gain": lambda r: _step(r) and _L(r).NH == 8 and _L(r).D == 19 and r.gain >= 1.5,
    "D = 2 in training at a gain": lambda r: _step(r) and _L(r).D == 2 and r.gain >= 1.5,
    "the pack-free forward at every limit of its table (D = 22, NH = 8, C = 128, X = 96, nb = 2)":
        lambda r: r.path == "folded_raw" and r.kind == "step"
        and (_L(r).D, _L(r).NH, _L(r).C, r.X, _L(r).nb) == (22, 8, 128, 96, 2),
    "the two-launch fold where the table applies, at NH other than 7":
        lambda r: r.path == "folded_two" and raw_applicable(_L(r), r.X) and _L(r).NH != 7,
    "the two-launch fold where the table is refused":
        lambda r: r.path == "folded_two" and not raw_applicable(_L(r), r.X),
    "Da = 2, Db = 1 without ActNorm in the matrix-core inverse":
        lambda r: r.kind == "logprob" and _L(r).D == 3 and not _L(r).act_norm,
    "PMB = 3792 of the ring slot's 4096 floats, at D = 22":
        lambda r: r.kind == "logprob" and _L(r).PMB == 3792 and _L(r).D == 22,
    "a hidden layer of width 1 in the matrix-core inverse": lambda r: r.kind == "logprob" and 1 in _L(r).H,
    "NH = 1 in the matrix-core inverse: no hidden-bias section": lambda r: r.kind == "logprob" and _L(r).NH == 1,
}
BRANCHES.update({f"the training-mode inverse at NH = {NH}, {B} row{'s' * (B > 1)}":
                 (lambda r, NH=NH, B=B: r.kind == "train_inverse" and _L(r).NH == NH and r.B == B)
                 for NH in (4, 5, 6) for B in (1, 37)})
BRANCHES.update({f"row position in the matrix-core inverse at NH = {NH}":
                 (lambda r, NH=NH: r.kind == "position" and _L(r).NH == NH) for NH in (5, 6)})


def missing(rs):
    """What the runs rs do not reach: arms of required_arms, the (NH, LDJ) and (PERM, LDJ) pairs of the matrix-core
    inverse, and labels of BRANCHES. Empty for the lists as they stand."""
    got = set().union(*(arms(r) for r in rs)) if rs else set()
    out = sorted(required_arms() - got, key=str)
    mf = {a[1:] for a in got if a[0] == "k_inverse_mfma"}
    out += [("k_inverse_mfma", NH, "any", ldj) for NH in range(1, MAX_HIDDEN + 1) for ldj in (False, True)
            if not any((NH, pm, ldj) in mf for pm in (False, True))]
    out += [("k_inverse_mfma", "any", pm, ldj) for pm in (False, True) for ldj in (False, True)
            if not any((NH, pm, ldj) in mf for NH in range(1, MAX_HIDDEN + 1))]
    out += [label for label, reaches in BRANCHES.items() if not any(reaches(r) for r in rs)]
    return out
