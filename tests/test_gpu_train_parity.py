"""Training-mode (dropout on) parity of both coupling families against the fp64 oracle fed the kernels' own masks.

Every other training-mode test compares two paths through the same kernels (fused vs unfused, folded vs unfolded,
graph vs eager) or one central difference along the gradient, so an error shared by the paths, or one orthogonal to
the gradient, passes. Here the oracle (oracle/cnf_oracle.py, float64, autograd) runs the same operation with the masks
the launch drew, handed in through its `keep` hook:

  * small family (bcnf_stack*.hip k_forward / k_backward / k_inverse, folded tail): the masks come from the host
    restatement of the draw (tests/dropout_ref.py keep_callable; pinned bit for bit against the saved records at these
    shapes by tests/test_gpu_dropout.py), at the launch's (seed, offset) read from rng_state();
  * wide family (bcnf_wide.hip): the masks come from the host restatement of its two draw rules
    (tests/dropout_ref.py wide_keep_callable; pinned bit for bit against the saved records of every launch form by
    tests/test_gpu_wide_dropout.py), at the launch's (seed, offset). The masks read from the records (a unit is kept
    iff its masked activation or derivative factor is nonzero) remain for the independence checks only. The forward
    that saves nothing, the training-mode inverse and sample(outer=True) in train mode, which leave no records, are
    compared with the oracle under the restated masks as well.

Gates (the eval-mode gates of tests/test_gpu_parity.py / test_gpu_wide.py; dropout adds one fp32 multiply per unit):
z and log|det J| `close` at 1e-5, the loss 1e-5 |ref| + 1e-5, every parameter gradient, dL/dh and dL/dy
`close(rtol=1e-4, floor=1e-4)`; the training-mode inverse 1e-5, 1e-4 at the shape whose eval inverse test uses 1e-4.
Each path is compared with the oracle, never with another path.
"""
import functools
import types

import numpy as np
import pytest
import torch

from conftest import FC_SMALL_CFG, close, golden_sd, load_golden
from dropout_ref import (SMALL_TRAIN_FOLD_X, SMALL_TRAIN_GAIN, SMALL_TRAIN_RAW, SMALL_TRAIN_SHAPES, apply_gain, fold_config,
                         keep_callable, shape_config, wide_keep_callable)
from oracle import cnf_oracle as O

pytestmark = pytest.mark.gpu

DEV = "cuda"
INV_TAG = 0x40000000          # k_inverse<NH>'s draw tag (bcnf_stack_inv.hip)
OFFSET = 3                    # the Philox offset every compared launch runs at
VAL = dict(rtol=1e-5, floor=1e-5)
GRAD = dict(rtol=1e-4, floor=1e-4)


# ------------------------------------------------------------------------------------------ comparison
def _ratio(a, b, rtol, floor):
    """Worst error as a fraction of conftest.close's bound (<= 1 passes): reporting only, `close` decides."""
    a = torch.as_tensor(a, dtype=torch.float64)
    b = torch.as_tensor(b, dtype=torch.float64)
    if not b.numel():
        return 0.0
    scale = max(1.0, float(b.abs().max()))
    return float(((a - b).abs() / (rtol * b.abs() + floor * scale)).max())


def compare(got, ref):
    """[(quantity, passed, fraction of its gate)] for everything the GPU path exposes."""
    rows = []
    for key in ("z", "ldj"):
        if key in got:
            rows.append((key, close(got[key], ref[key], **VAL)[0], _ratio(got[key], ref[key], **VAL)))
    lo, lr = float(got["loss"]), float(ref["loss"])
    bound = 1e-5 * abs(lr) + 1e-5
    rows.append(("loss", abs(lo - lr) <= bound, abs(lo - lr) / bound))
    for key in ("dy", "dh"):
        if got.get(key) is not None:
            rows.append((key, close(got[key], ref[key], **GRAD)[0], _ratio(got[key], ref[key], **GRAD)))
    assert set(got["grads"]) == set(ref["grads"]), set(got["grads"]) ^ set(ref["grads"])
    for name, g in got["grads"].items():
        rows.append(("grad/" + name, close(g, ref["grads"][name], **GRAD)[0], _ratio(g, ref["grads"][name], **GRAD)))
    return rows


def report(case, path, rows):
    """One line per (case, path) with the worst fraction of each gate (run pytest with -s to collect them)."""
    worst = lambda keys: max([r for r in rows if r[0] in keys], key=lambda r: r[2], default=("-", True, 0.0))  # noqa: E731
    gw = max([r for r in rows if r[0].startswith("grad/") or r[0] in ("dy", "dh")], key=lambda r: r[2])
    print(f"\nTRAIN_PARITY {case.name} {path}: z {worst(('z',))[2]:.3f} ldj {worst(('ldj',))[2]:.3f} "
          f"loss {worst(('loss',))[2]:.3f} worst-grad {gw[2]:.3f} ({gw[0]}) of the gate")


def check(case, path, rows):
    report(case, path, rows)
    bad = [(k, round(r, 3)) for k, ok, r in rows if not ok]
    assert not bad, (case.name, path, bad[:8], len(bad))


# ------------------------------------------------------------------------------------------ oracle and GPU runs
def oracle_run(case, keep, dtype=torch.float64, training=True):
    """z, ldj, loss and every gradient of one training step on the oracle with the masks `keep` (training = False:
    of one step in eval mode, no masks)."""
    spec = case.spec
    sdg = {k: v.to(dtype).clone().requires_grad_(not k.endswith("orthonormal_matrix")) for k, v in case.sd.items()}
    y = case.y.to(dtype).requires_grad_(True)
    if spec.feature_sizes:
        h = O.feature_forward(sdg, spec, case.cond.to(dtype))
        h.retain_grad()
    else:
        h = case.cond.to(dtype).requires_grad_(True)
    z, ldj = O.model_forward(sdg, spec, y, h, training=training, keep=keep)
    loss = O.inn_nll_loss(z, ldj)
    loss.backward()
    return dict(z=z.detach(), ldj=ldj.detach(), loss=loss.detach(), dy=y.grad, dh=h.grad,
                grads={k: v.grad for k, v in sdg.items() if v.grad is not None})


def gpu_run(case, path, training=True):
    """One training step of `path` at the case's (seed, OFFSET): what the path exposes of z, ldj, loss, dL/dy, dL/dh
    and the parameter gradients. Asserts the offset advanced by exactly one (training = False: the same step of the
    model in eval mode, which draws no masks and leaves the offset alone)."""
    from bcnf_amd import inn_nll_loss
    m, st = case.m, case.m.fused
    m.zero_grad(set_to_none=True)
    m.train(training)
    st.rng_state()[1] = OFFSET
    y, cond = case.y.to(DEV), case.cond.to(DEV)
    folded = path.startswith("folded")
    feats = []

    def grab(mod, args, out):
        if out.requires_grad and not out.is_leaf:
            out.retain_grad()
        feats.append(out)

    hook = m.feature_network_stack.register_forward_hook(grab)
    out = {}
    try:
        if not folded:
            y.requires_grad_(True)
            if not case.spec.feature_sizes:
                cond.requires_grad_(True)
        if path == "unfused":
            z = m(y, cond, log_det_J=True)
            loss = inn_nll_loss(z, m.log_det_J)
            out.update(z=z.detach().cpu(), ldj=m.log_det_J.detach().cpu())
        else:
            m.fold_features = folded
            if path == "folded_two":
                st.use_raw_forward = False                # on the instance: pack + fold, then the forward
            try:
                if not case.wide:
                    assert (m._foldable_linear(y, (cond,)) is not None) == folded
                if path in ("folded_raw", "folded_two"):
                    assert (st.raw_table(case.spec.feature_sizes[0]) is not None) == (path == "folded_raw")
                loss = m.nll_loss(y, cond)[0]
            finally:
                del m.fold_features
                st.__dict__.pop("use_raw_forward", None)
        loss.backward()
        if case.wide and path == "folded":
            with torch.no_grad():
                assert m._wide_fold(y, (cond,)) is not None
    finally:
        hook.remove()
        m.train()
    assert int(st.rng_state()[1].item()) == OFFSET + int(training), "the RNG offset advances once per step"
    out["loss"] = loss.detach().cpu()
    out["dy"] = y.grad.cpu() if y.grad is not None else None
    out["dh"] = feats[-1].grad.cpu() if feats and feats[-1].grad is not None else None
    if not folded:
        assert out["dy"] is not None and out["dh"] is not None
    out["grads"] = {n: p.grad.detach().cpu().clone() for n, p in m.named_parameters() if p.grad is not None}
    m.zero_grad(set_to_none=True)
    return out


def _perturb(m):
    with torch.no_grad():
        for n, p in m.named_parameters():
            if n.endswith("scale"):
                p.copy_(0.5 + torch.rand_like(p))
            elif n.endswith("bias") and n.count(".") == 2:
                p.copy_(0.1 * torch.randn_like(p))


# ------------------------------------------------------------------------------------------ small family
def small_seed(B):
    """The Philox seed of every launch of a (shape, B) case (FusedStack.set_seed makes it a constant of the test)."""
    return 0x5EED00000000 + B


def small_weights(name):
    """(model on the CPU, oracle spec, fp32 state dict) of a small-family case: no GPU. A shape with a gain
    (SMALL_TRAIN_GAIN) has it applied after _perturb and before the oracle's copy is taken."""
    from bcnf_amd import CondRealNVP_v2
    if name == "fc_small":
        torch.manual_seed(0)
        m = CondRealNVP_v2.from_config(FC_SMALL_CFG)
        m.load_state_dict(golden_sd(load_golden("g1_fc_small.npz")))     # perturbed ActNorm scales
        spec = O.FC_SMALL_SPEC
    else:
        shape = SMALL_TRAIN_SHAPES[name]
        X = SMALL_TRAIN_FOLD_X.get(name)
        torch.manual_seed(7)
        m = CondRealNVP_v2.from_config(shape_config(shape) if X is None else fold_config(shape, X))
        _perturb(m)
        if name in SMALL_TRAIN_GAIN:
            apply_gain(m, SMALL_TRAIN_GAIN[name])
        spec = O.StackSpec(size=shape["size"], nested_sizes=shape["nested_sizes"], n_blocks=shape["n_blocks"],
                           n_conditions=shape["n_conditions"], dropout=shape["dropout"], act_norm=shape["act_norm"],
                           feature_sizes=[] if X is None else [X, shape["n_conditions"]])
    sd = {k: v.detach().clone() for k, v in m.state_dict().items()}
    return m, spec, sd


def _small_keep(case, offset, rows, tag=0):
    s = case.spec
    return keep_callable(s.dropout, case.seed, offset, s.n_blocks, s.nested_sizes, rows, tag=tag)


@functools.lru_cache(maxsize=None)
def small_reference(name, B):
    """A small-family case with its fp64 reference and no GPU: the model still on the CPU, the inputs, the seed the
    launches will run at, and oracle_run with the masks of that seed at OFFSET. tests/test_small_arms_cpu.py checks
    the conditions on the reference here; small_case moves the same object to the GPU."""
    m, spec, sd = small_weights(name)
    g = torch.Generator().manual_seed(1000 + B)
    y = torch.randn(B, spec.size, generator=g)
    if spec.feature_sizes:
        cond = torch.randn(B, spec.feature_sizes[0] // 3, 3, generator=g)
    else:
        cond = torch.randn(B, spec.n_conditions, generator=g)
    case = types.SimpleNamespace(name=f"{name}-B{B}", m=m, spec=spec, sd=sd, y=y, cond=cond, seed=small_seed(B),
                                 wide=False)
    case.ref = oracle_run(case, _small_keep(case, OFFSET, B))
    return case


@functools.lru_cache(maxsize=None)
def small_case(name, B):
    case = small_reference(name, B)
    case.m.to(DEV).train()
    assert type(case.m.fused).__name__ == "FusedStack"
    case.m.fused.set_seed(case.seed)
    assert int(case.m.fused.rng_state()[0].item()) == case.seed    # read from the device state, as the launch does
    return case


# (shape, B): FC_small, the shapes of before, and the new ones -- B = 37 for all, and B = 133 past KC rows of the W1
# split-K for the two widest C
SMALL = ([("fc_small", 1), ("fc_small", 37), ("fc_small", 133), ("fc_small", 517)]
         + [(k, 37) for k in SMALL_TRAIN_SHAPES] + [("nh6_d20_c129", 133), ("nh4_d31_c208", 133)])
NEW_SMALL = [(n, B) for n, B in SMALL if n in SMALL_TRAIN_GAIN]
# folded_raw: the pack-free one-launch forward (bcnf_fold_train_forward); folded_two: pack + fold, then the forward
# (use_raw_forward = False); folded: whichever of the two the library takes (FC_small: the first)
SMALL_PATHS = [(n, B, p) for n, B in SMALL for p in
               ("unfused", "fused") + (("folded",) if n == "fc_small" else ())
               + (("folded_raw",) if SMALL_TRAIN_RAW.get(n) else ()) + (("folded_two",) if n in SMALL_TRAIN_RAW else ())]


@pytest.mark.parametrize("name,B,path", SMALL_PATHS, ids=[f"{n}-B{B}-{p}" for n, B, p in SMALL_PATHS])
def test_small_training_step_vs_fp64_oracle(name, B, path):
    """FC_small (g1 weights, p = 0.383) at B = 1, 37 (ragged: the 11 padded rows of the third workgroup draw masks
    too and must reach no gradient), 133 (past KC = 128 of the W1 condition split-K), 517 (past FIN_KC = 512 of the
    folded tail), and the other small shapes at B = 37 (tests/dropout_ref.py: every NH = 1 .. 8, the split and C
    edges; B = 133 too at C = 129 and C = 208). unfused: m() + inn_nll_loss + autograd; fused: nll_loss with
    fold_features = False; folded (FC_small): nll_loss with the feature Linear folded in, its gradients from
    k_fold_splitk / k_fold_finish. The four fold_* shapes run the folded step in both forms: folded_raw where the
    pack-free forward's table applies (raw_table(X) is not None exactly there), folded_two with the two-launch form
    forced -- each against the oracle, never against the other."""
    case = small_case(name, B)
    if name in SMALL_TRAIN_RAW:
        assert (case.m.fused.raw_table(case.spec.feature_sizes[0]) is not None) == SMALL_TRAIN_RAW[name]
    check(case, path, compare(gpu_run(case, path), case.ref))


FOLD_EVAL = [("fc_small", 37)] + [(n, 37) for n, raw in SMALL_TRAIN_RAW.items() if raw]


@pytest.mark.parametrize("name,B", FOLD_EVAL, ids=[f"{n}-B{B}" for n, B in FOLD_EVAL])
def test_small_folded_eval_step_vs_fp64_oracle(name, B):
    """k_forward<NH, false, true, true>: the pack-free folded step of a model in eval mode (no masks, the record
    still saved for the backward), at every NH the table is run at. Same gates, the oracle in eval mode."""
    case = small_case(name, B)
    assert case.m.fused.raw_table(case.spec.feature_sizes[0]) is not None
    ref = oracle_run(case, None, training=False)
    check(case, "folded_raw-eval", compare(gpu_run(case, "folded_raw", training=False), ref))


@pytest.mark.parametrize("name,B", SMALL, ids=[f"{n}-B{B}" for n, B in SMALL])
def test_small_nosave_training_forward_is_the_saving_forward(name, B):
    """k_forward<NH, true, false> (training forward under no_grad) at the same (seed, offset): z and ldj bit-identical
    to the saving forward's -- the mask rule does not depend on SAVE, and with dropout on the no-save forward takes
    the saving forward's GELU form (mlp_forward_s; the forward-only polynomial it used before differed from it by
    rounding) -- and so within the gate of the oracle."""
    case = small_case(name, B)
    m, st = case.m, case.m.fused
    y, cond = case.y.to(DEV), case.cond.to(DEV)
    st.rng_state()[1] = OFFSET
    z1 = m(y, cond, log_det_J=True)                      # parameters require grad: the saving forward
    l1 = m.log_det_J
    assert z1.requires_grad
    st.rng_state()[1] = OFFSET
    with torch.no_grad():
        z0 = m(y, cond, log_det_J=True)
        l0 = m.log_det_J
    assert int(st.rng_state()[1].item()) == OFFSET + 1
    assert torch.equal(z0, z1.detach()) and torch.equal(l0, l1.detach())
    ok, err = close(z0.cpu(), case.ref["z"])
    assert ok, err
    ok, err = close(l0.cpu(), case.ref["ldj"])
    assert ok, err


TRAIN_INVERSE = [("fc_small", 1, 1e-5), ("fc_small", 37, 1e-5), ("d7_h12_9", 1, 1e-4), ("d7_h12_9", 37, 1e-4),
                 ("nh4_d24_c17", 1, 1e-5), ("nh4_d24_c17", 37, 1e-5), ("nh5_d25_c128", 1, 1e-5),
                 ("nh5_d25_c128", 37, 1e-5), ("nh6_d20_c129", 1, 1e-5), ("nh6_d20_c129", 37, 1e-5),
                 ("d32_nh1", 37, 1e-5), ("nh3_d19_c80", 37, 1e-5), ("nh8_p50_g2", 37, 1e-5)]


@pytest.mark.parametrize("name,B,tol", TRAIN_INVERSE)
def test_small_training_mode_inverse_vs_fp64_oracle(name, B, tol):
    """model.train(); model.inverse(): k_inverse<NH>, masks drawn with tag 0x40000000, at every NH = 1 .. 8. Gate
    as the eval inverse test of the shape (test_ragged_batches_vs_oracle: 1e-5; test_other_shapes_vs_oracle: 1e-4);
    1e-5 at the shapes with a gain and at d32_nh1."""
    case = small_case(name, 37)
    m, st, spec = case.m, case.m.fused, case.spec
    g = torch.Generator().manual_seed(B)
    zl = torch.randn(B, spec.size, generator=g)
    cond = case.cond[:B]
    sd64 = {k: v.double() for k, v in case.sd.items()}
    h64 = O.feature_forward(sd64, spec, cond.double()) if spec.feature_sizes else cond.double()
    ref = O.model_inverse(sd64, spec, zl.double(), h64, training=True, keep=_small_keep(case, OFFSET, B, INV_TAG))
    ref_fwd_tag = O.model_inverse(sd64, spec, zl.double(), h64, training=True, keep=_small_keep(case, OFFSET, B))
    st.rng_state()[1] = OFFSET
    with torch.no_grad():
        inv = m.inverse(zl.to(DEV), cond.to(DEV)).cpu()
    assert int(st.rng_state()[1].item()) == OFFSET + 1, "the offset advances once per inverse launch"
    ok, err = close(inv, ref, rtol=tol, floor=tol)
    print(f"\nTRAIN_PARITY {name}-B{B} inverse: {_ratio(inv, ref, tol, tol):.3f} of the gate")
    assert ok, err
    assert not close(inv, ref_fwd_tag, rtol=tol, floor=tol)[0]     # the forward's masks are not the inverse's


def test_small_training_mode_sample_vs_fp64_oracle():
    """sample(outer=True) of a model left in train mode: the cond_index path of k_inverse<NH>, four launches
    (conditions 4 + 3, samples 3 + 2), each at its own offset; the oracle draws the same CPU z stream by seeding."""
    case = small_case("fc_small", 37)
    m, st, spec = case.m, case.m.fused, case.spec
    traj = case.cond[:7]
    st.rng_state()[1] = OFFSET
    torch.manual_seed(123)
    got = m.sample(5, traj, outer=True, batch_size=4, sample_batch_size=3)
    assert int(st.rng_state()[1].item()) == OFFSET + 4, "the offset advances once per launch"
    sd64 = {k: v.double() for k, v in case.sd.items()}
    torch.manual_seed(123)                                 # the float32 z stream; float64 from the first coupling on
    ref = O.sample(sd64, spec, 5, traj.double(), outer=True, batch_size=4, sample_batch_size=3,
                   keeps=lambda n, rows: _small_keep(case, OFFSET + n, rows, INV_TAG))
    assert got.shape == ref.shape == (5, 7, spec.size)
    ok, err = close(got, ref)
    print(f"\nTRAIN_PARITY fc_small sample: {_ratio(got, ref, **VAL):.3f} of the gate")
    assert ok, err


# ------------------------------------------------------------------------------------------ wide family
WIDE = {
    "w96": (dict(size=19, nested_sizes=[96] * 3, n_blocks=3, n_conditions=80, dropout=0.3, act_norm=True), [90, 80], 257),
    "w40_two_way": (dict(size=19, nested_sizes=[40] * 2, n_blocks=3, n_conditions=24, dropout=0.2, act_norm=True,
                         two_way=True), None, 37),
    "w24_c13": (dict(size=19, nested_sizes=[24] * 2, n_blocks=2, n_conditions=13, dropout=0.2, act_norm=True), None, 37),
    "fc_large_B64": (dict(size=19, nested_sizes=[526] * 5, n_blocks=2, n_conditions=1360, dropout=0.407,
                          act_norm=True), [90, 1360], 64),
    # once at M >= 1024, where the large-M GEMM tilings engage
    "fc_large_B1024": (dict(size=19, nested_sizes=[526] * 5, n_blocks=2, n_conditions=1360, dropout=0.407,
                            act_norm=True), [90, 1360], 1024),
}


# Not in WIDE (the training-step and independence tests keep their cases): the edge shape of the mask and inverse
# tests. NH = 8 reaches the largest draw tag; H = 150 > 128 gives every GEMM tiling at least two column tiles and a
# ragged last one; B = 131 two 128-row tiles and, 131 % 4 = 3, a ragged last row group.
WIDE_EDGE = {
    "w150_nh8": (dict(size=19, nested_sizes=[150] * 8, n_blocks=2, n_conditions=24, dropout=0.5, act_norm=True), None, 131),
}


def _workspace_records(ws, spec, B):
    """bool [nv][NH][B][H] on the device from a saving wide launch's workspace: unit kept iff its saved masked
    activation (A) or masked derivative factor (G) is nonzero. Offsets as carve() in bcnf_wide.hip: P (B nv HP), nllp
    (B), A, G (nv NH B HP each), every region padded to 4 floats plus 64."""
    s = spec
    nv, NH, H = s.n_blocks * (2 if s.two_way else 1), len(s.nested_sizes), s.nested_sizes[0]
    HP = (H + 1 + 3) // 4 * 4
    pad = lambda n: (n + 3) // 4 * 4 + 64  # noqa: E731
    n = nv * NH * B * HP
    a0 = pad(B * nv * HP) + pad(B)
    g0 = a0 + pad(n)
    A = ws[a0: a0 + n].view(nv, NH, B, HP)[..., :H]
    G = ws[g0: g0 + n].view(nv, NH, B, HP)[..., :H]
    return (A != 0) | (G != 0)


def _wide_records(case, offset):
    """_workspace_records of one saving forward launch of the case at `offset`."""
    m, st = case.m, case.m.fused
    st.rng_state()[1] = offset
    with torch.no_grad():
        h = m.feature_network_stack(case.cond.to(DEV))
        _, _, _, (ws, _) = st.launch_forward(case.y.to(DEV), h, True, save=True)
    return _workspace_records(ws, case.spec, case.y.shape[0])


def wide_seed(case):
    """The launch's Philox seed, read from the device state as the launch reads it."""
    return int(case.m.fused.rng_state()[0].item())


def wide_keep(case, offset, rows):
    """The oracle's `keep` for a launch of `rows` rows of the case at `offset`, from the host restatement of both wide
    draw rules (tests/dropout_ref.py): nothing of it comes from the code under test but the seed it was handed."""
    s = case.spec
    return wide_keep_callable(s.dropout, wide_seed(case), offset, s.n_blocks, s.two_way, s.nested_sizes, rows)


def wide_build(name, shape, fsizes, B):
    """A wide-family case on the GPU in train mode, its seed set: model, oracle spec, fp32 state dict, inputs."""
    from bcnf_amd import CondRealNVP_v2
    C = shape["n_conditions"]
    torch.manual_seed(7)
    if fsizes is None:
        cfg = shape_config(shape)
    else:
        cfg = {"global": {"parameter_selection": [f"p{i}" for i in range(shape["size"])]}, "model": {"kwargs": shape},
               "feature_networks": [{"type": "ConcatenateCondition", "kwargs": {"input_size": None, "output_size": 90}},
                                    {"type": "FullyConnected", "kwargs": {"sizes": fsizes, "dropout": 0.0}}]}
    m = CondRealNVP_v2.from_config(cfg)
    _perturb(m)
    sd = {k: v.detach().clone() for k, v in m.state_dict().items()}
    m.to(DEV).train()
    assert type(m.fused).__name__ == "WideStack"
    spec = O.StackSpec(size=shape["size"], nested_sizes=shape["nested_sizes"], n_blocks=shape["n_blocks"],
                       n_conditions=C, dropout=shape["dropout"], act_norm=shape["act_norm"],
                       two_way=shape.get("two_way", False), feature_sizes=list(fsizes or ()))
    g = torch.Generator().manual_seed(2000 + B)
    y = torch.randn(B, spec.size, generator=g)
    cond = torch.randn(B, 30, 3, generator=g) if fsizes else torch.randn(B, C, generator=g)
    m.fused.set_seed(0xA11CE0000 + B)
    return types.SimpleNamespace(name=name, m=m, spec=spec, sd=sd, y=y, cond=cond, wide=True)


@functools.lru_cache(maxsize=None)
def wide_case(name):
    """wide_build of a WIDE / WIDE_EDGE case with the fp64 training step under the restated masks of (seed, OFFSET)."""
    shape, fsizes, B = WIDE.get(name) or WIDE_EDGE[name]
    case = wide_build(name, shape, fsizes, B)
    case.masks = _wide_records(case, OFFSET)          # for assert_record_masks_are_independent_draws; not the oracle's
    case.ref = oracle_run(case, wide_keep(case, OFFSET, B))
    return case


def assert_record_masks_are_independent_draws(case):
    """The masks read from the records: the dropped fraction is within 4 sigma of p (a kept unit whose fp32 activation
    and factor are both exactly zero reads as dropped: no room for many of those), every pair of distinct (block,
    half, layer) masks of the launch agrees at the rate of independent draws, (1 - p)^2 + p^2 within 4 sigma (a tag
    collision would make two of them equal), and the next offset draws other masks. `case`: a wide-family case with
    its `masks` read at OFFSET (wide_case here; the LinearFFTEnriched cases of tests/test_gpu_variants_fp64.py)."""
    p = float(np.float32(case.spec.dropout))
    k = case.masks.flatten(0, 1)                           # [nv * NH][B][H]
    n = k[0].numel()
    drop = 1.0 - k.double().mean().item()
    assert abs(drop - p) <= 4 * np.sqrt(p * (1 - p) / k.numel()), (drop, p)
    q = (1 - p) ** 2 + p ** 2
    kf = k.reshape(k.shape[0], -1).double()
    agree = (kf @ kf.T + (1 - kf) @ (1 - kf).T) / n
    i, j = torch.triu_indices(k.shape[0], k.shape[0], 1)
    dev = (agree[i, j] - q).abs().max().item()
    assert dev <= 4 * np.sqrt(q * (1 - q) / n), (dev, 4 * np.sqrt(q * (1 - q) / n))
    nxt = _wide_records(case, OFFSET + 1)
    a2 = (nxt == case.masks).double().mean().item()
    assert abs(a2 - q) <= 4 * np.sqrt(q * (1 - q) / k.numel()), (a2, q)
    assert torch.equal(_wide_records(case, OFFSET), case.masks)       # and the same offset the same ones


@pytest.mark.parametrize("name", list(WIDE))
def test_wide_record_masks_are_independent_draws(name):
    """assert_record_masks_are_independent_draws at every wide case."""
    assert_record_masks_are_independent_draws(wide_case(name))


WIDE_PATHS = [(n, p) for n in WIDE for p in ("unfused", "fused") + (("folded",) if WIDE[n][1] else ())]


@pytest.mark.parametrize("name,path", WIDE_PATHS, ids=[f"{n}-{p}" for n, p in WIDE_PATHS])
def test_wide_training_step_vs_fp64_oracle(name, path):
    """[96] * 3 with a feature Linear (B = 257), a two_way stack and C = 13 (B = 37), and the FC_large coupling shape
    ([526] * 5, C = 1360, p = 0.407, two blocks) behind a single feature Linear at B = 64 and once at B = 1024.
    unfused / fused as in the small family; folded: the feature Linear folded into the condition projection
    (_wide_fold taken)."""
    case = wide_case(name)
    check(case, path, compare(gpu_run(case, path), case.ref))


@pytest.mark.parametrize("name", ["w96", "w40_two_way"])
def test_wide_nosave_training_forward_vs_fp64_oracle(name):
    """The training forward under no_grad (wide_forward with save = false: the chain on the two A ping-pong buffers,
    no G, no records) at (seed, OFFSET): z and log|det J| against the oracle under the restated masks, at the eval
    gate. It leaves no records, so only the host masks can reach it."""
    case = wide_case(name)
    m, st = case.m, case.m.fused
    m.train()
    st.rng_state()[1] = OFFSET
    with torch.no_grad():
        z = m(case.y.to(DEV), case.cond.to(DEV), log_det_J=True)
        ldj = m.log_det_J
    assert not z.requires_grad
    assert int(st.rng_state()[1].item()) == OFFSET + 1, "the RNG offset advances once per launch"
    rows = [(k, close(g.cpu(), case.ref[k], **VAL)[0], _ratio(g.cpu(), case.ref[k], **VAL))
            for k, g in (("z", z), ("ldj", ldj))]
    print(f"\nTRAIN_PARITY {name} nosave-forward: z {rows[0][2]:.3f} ldj {rows[1][2]:.3f} of the gate")
    assert all(ok for _, ok, _ in rows), rows


def _wide_inverse_inputs(case, B):
    """(latents, conditions, fp64 state dict, fp64 features) of a B-row inverse of the case: the first B conditions."""
    spec = case.spec
    zl = torch.randn(B, spec.size, generator=torch.Generator().manual_seed(B))
    cond = case.cond[:B]
    sd64 = {k: v.double() for k, v in case.sd.items()}
    h64 = O.feature_forward(sd64, spec, cond.double()) if spec.feature_sizes else cond.double()
    return zl, cond, sd64, h64


WIDE_TRAIN_INVERSE = [("w96", 1), ("w96", 257), ("w40_two_way", 37), ("w24_c13", 37), ("w150_nh8", 131),
                      ("fc_large_B64", 64)]


@pytest.mark.parametrize("name,B", WIDE_TRAIN_INVERSE, ids=[f"{n}-B{B}" for n, B in WIDE_TRAIN_INVERSE])
def test_wide_training_mode_inverse_vs_fp64_oracle(name, B):
    """model.train(); model.inverse(): wide_inverse with rng. It draws with the forward's tags (link: 16 v; chain
    GEMM: 16 v + l) in the inverse's block order (two_way: real blocks in reverse, nn_a's half before nn_b's), the
    rows being the latent rows, and saves no records: the oracle's masks are the host restatement. The gate is the
    eval inverse's of tests/test_gpu_wide.py (`close` defaults). Control: the oracle under the masks of OFFSET + 1
    fails the same gate, so the gate sees the masks."""
    case = wide_case(name)
    m, st, spec = case.m, case.m.fused, case.spec
    zl, cond, sd64, h64 = _wide_inverse_inputs(case, B)
    ref = O.model_inverse(sd64, spec, zl.double(), h64, training=True, keep=wide_keep(case, OFFSET, B))
    ref_next = O.model_inverse(sd64, spec, zl.double(), h64, training=True, keep=wide_keep(case, OFFSET + 1, B))
    m.train()
    st.rng_state()[1] = OFFSET
    with torch.no_grad():
        inv = m.inverse(zl.to(DEV), cond.to(DEV)).cpu()
    assert int(st.rng_state()[1].item()) == OFFSET + 1, "the offset advances once per inverse launch"
    ok, err = close(inv, ref, **VAL)
    print(f"\nTRAIN_PARITY {name}-B{B} inverse: {_ratio(inv, ref, **VAL):.3f} of the gate "
          f"(against the masks of the next offset: {_ratio(inv, ref_next, **VAL):.1f})")
    assert ok, err
    assert not close(inv, ref_next, **VAL)[0]              # the next offset's masks are not this launch's


def test_wide_training_mode_sample_vs_fp64_oracle():
    """sample(outer=True) of a wide model left in train mode: the cond_index path of wide_inverse (features once per
    condition, the masks by latent row), four launches (conditions 4 + 3, samples 3 + 2: 12, 8, 9 and 6 rows), each at
    its own offset; the oracle draws the same CPU z stream by seeding."""
    case = wide_case("w96")
    m, st, spec = case.m, case.m.fused, case.spec
    traj = case.cond[:7]
    m.train()
    st.rng_state()[1] = OFFSET
    torch.manual_seed(123)
    got = m.sample(5, traj, outer=True, batch_size=4, sample_batch_size=3)
    assert int(st.rng_state()[1].item()) == OFFSET + 4, "the offset advances once per launch"
    sd64 = {k: v.double() for k, v in case.sd.items()}
    torch.manual_seed(123)                                 # the float32 z stream; float64 from the first coupling on
    ref = O.sample(sd64, spec, 5, traj.double(), outer=True, batch_size=4, sample_batch_size=3,
                   keeps=lambda n, rows: wide_keep(case, OFFSET + n, rows))
    assert got.shape == ref.shape == (5, 7, spec.size)
    ok, err = close(got, ref, **VAL)
    print(f"\nTRAIN_PARITY w96 sample: {_ratio(got, ref, **VAL):.3f} of the gate")
    assert ok, err
