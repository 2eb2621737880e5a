"""The LinearFFTEnriched and AnyGLU coupling stacks against the fp64 oracle (oracle/cnf_oracle.py, whose variant layers
are pinned to the reference's own fixtures by tests/test_oracle_golden.py), at the shapes of tests/variant_cases.py.

What tests/test_gpu_variants.py has is one even-width fixture per layer in eval mode. Here:

  a. FFTWideStack's fold maps on their own: refresh() (canonical -> effective weights, one GEMM per input width) and
     unfold_grad() against W[:, :n] + W[:, n:] F64 and G F64^T, F64 from torch.fft.rfft of the identity, at odd widths,
     three width groups, and a group holding two row counts;
  b. eval parity (z, ldj, log_prob, inverse, every gradient, dL/dy, dL/dh) at those shapes, B = 1 included;
  c. training mode with the launch's masks: the host restatement of the wide draw for the FFT stack (the mechanism
     of tests/test_gpu_train_parity.py), forward hooks on nn.Dropout for the layerwise AnyGLU stack;
  d. TrainStep on an FFT model: graph replay == eager bit for bit, three steps against torch.optim.Adam on the fp64
     oracle (the gradient Adam is handed, in the reference's layout), and no stale effective weights or pack afterwards;
  e. sample() values and log-densities.

Every comparison is a GPU path against the fp64 oracle, never a path against a path, except where "bit for bit" is said.
Gates are the project's existing ones for the same quantities: values `close` at 1e-5 (VAL), the loss 1e-5 |ref| + 1e-5,
gradients `close(rtol=1e-4, floor=1e-4)` (GRAD), the fold GEMMs 2e-6 (|A| |B|) + 1e-6 (tests/test_gpu_wide.py), the
log-density of draws the gate of tests/test_gpu_sample_logprob.py. The oracle in plain fp32 sits at about 1 % of the
value and gradient gates at every case here (cfg175 included), so nothing is gated wider. Each test prints one
VARIANT_FP64 line with the worst fraction of each gate (pytest -s); profiles/variant_fp64_tests.txt holds a run's.
"""
import functools
import types

import numpy as np
import pytest
import torch

import variant_cases as V
from conftest import close
from oracle import cnf_oracle as O
from test_gpu_sample_logprob import _gate_lp, _sample_reference
from test_gpu_train_parity import (GRAD, OFFSET, VAL, _ratio, _wide_records, assert_record_masks_are_independent_draws,
                                   compare, gpu_run, oracle_run, wide_keep)

pytestmark = pytest.mark.gpu

DEV = "cuda"
LR = 1e-3


# ------------------------------------------------------------------------------------------ reporting
def val_row(key, got, ref, gate=VAL):
    return key, close(got, ref, **gate)[0], _ratio(got, ref, **gate)


def settle(name, path, rows):
    """Print one line per (case, path) with the worst fraction of each gate, then assert every row."""
    is_grad = lambda k: k.startswith("grad/") or k in ("dy", "dh")  # noqa: E731
    txt = " ".join(f"{k} {f:.3f}" for k, _, f in rows if not is_grad(k))
    grads = [r for r in rows if is_grad(r[0])]
    if grads:
        gw = max(grads, key=lambda r: r[2])
        txt += f" worst-grad {gw[2]:.3f} ({gw[0]}, {len(grads)} compared)"
    print(f"\nVARIANT_FP64 {name} {path}: {txt} of the gate")
    bad = [(k, round(f, 3)) for k, ok, f in rows if not ok]
    assert not bad, (name, path, bad[:8], len(bad))


# ------------------------------------------------------------------------------------------ cases and references
@functools.lru_cache(maxsize=None)
def case_of(name, B=None):
    """A case of the table on the GPU, built once and left unchanged: model, oracle spec, fp32 state dict, inputs."""
    m, spec, sd = V.build(name)
    y, cond = V.inputs(name, B)
    m.to(DEV).eval()
    wide = V.CASES[name]["layer"] == "LinearFFTEnriched"
    assert type(m.fused).__name__ == V.STACK_CLASS[V.CASES[name]["layer"]]
    if wide:
        m.fused.set_seed(0xFF7000000 + y.shape[0])
    return types.SimpleNamespace(name=f"{name}-B{y.shape[0]}", key=name, m=m, spec=spec, sd=sd, y=y, cond=cond,
                                 wide=wide)


def _sd64(sd):
    return {k: v.detach().cpu().double() for k, v in sd.items()}


def _values64(sd64, spec, y, cond, zl):
    """z, ldj, log_prob of (y, cond) and the inverse of the latents zl on the fp64 oracle."""
    with torch.no_grad():
        h = O.feature_forward(sd64, spec, cond.double())
        z, ldj = O.model_forward(sd64, spec, y.double(), h)
        return dict(z=z, ldj=ldj, log_prob=O.log_prob(z, ldj), inverse=O.model_inverse(sd64, spec, zl.double(), h))


def _latents(case):
    return torch.randn(case.y.shape[0], case.spec.size, generator=torch.Generator().manual_seed(5))


@functools.lru_cache(maxsize=None)
def eval_ref(name, B=None):
    """The fp64 eval-mode step of a case (oracle_run) and its log_prob / inverse, computed once."""
    case = case_of(name, B)
    ref = oracle_run(case, None, training=False)
    ref.update({k: v for k, v in _values64(_sd64(case.sd), case.spec, case.y, case.cond, _latents(case)).items()
                if k in ("log_prob", "inverse")})
    return ref


def _gpu_values(m, y, cond, zl):
    m.eval()
    with torch.no_grad():
        z = m.forward(y.to(DEV), cond.to(DEV), log_det_J=True)
        ldj = m.log_det_J.clone()
        return dict(z=z.cpu(), ldj=ldj.cpu(), log_prob=m.log_prob(y.to(DEV), cond.to(DEV)).cpu(),
                    inverse=m.inverse(zl.to(DEV), cond.to(DEV)).cpu())


def glu_run(case, path, training=True):
    """One step of the layerwise (AnyGLU) model -- what gpu_run of tests/test_gpu_train_parity.py returns for the
    fused families -- and the keep mask of every nn.Dropout call in call order, recorded by forward hooks: a unit is
    kept iff its output is nonzero or its input was zero."""
    from bcnf_amd import inn_nll_loss
    m = case.m
    m.zero_grad(set_to_none=True)
    m.train(training)
    y, cond = case.y.to(DEV).requires_grad_(True), case.cond.to(DEV)
    feats, masks = [], []

    def grab(mod, args, out):
        if out.requires_grad and not out.is_leaf:
            out.retain_grad()
        feats.append(out)

    def record(mod, args, out):
        masks.append(((out != 0) | (args[0] == 0)).detach().cpu())

    hooks = [m.feature_network_stack.register_forward_hook(grab)]
    hooks += [d.register_forward_hook(record) for d in m.layers.modules() if isinstance(d, torch.nn.Dropout)]
    out = {}
    try:
        if not case.spec.feature_sizes:
            cond.requires_grad_(True)
        if path == "unfused":
            z = m(y, cond, log_det_J=True)
            loss = inn_nll_loss(z, m.log_det_J)
            out.update(z=z.detach().cpu(), ldj=m.log_det_J.detach().cpu())
        else:
            loss = m.nll_loss(y, cond)[0]
        loss.backward()
    finally:
        for h in hooks:
            h.remove()
        m.train()
    out["loss"] = loss.detach().cpu()
    out["dy"] = y.grad.cpu()
    out["dh"] = feats[-1].grad.cpu()
    out["grads"] = {n: p.grad.detach().cpu().clone() for n, p in m.named_parameters() if p.grad is not None}
    m.zero_grad(set_to_none=True)
    return out, masks


def _trainable(sd):
    return sum(1 for k in sd if not k.endswith("orthonormal_matrix"))


# ------------------------------------------------------------------------------------------ a. the fold maps
def _f64(n):
    """F (2 (n // 2 + 1) x n) in float64 from torch.fft.rfft of the identity: F x = cat(Re rfft x, Im rfft x)."""
    f = torch.fft.rfft(torch.eye(n, dtype=torch.float64), dim=-1, norm="forward")     # row i: rfft(e_i)
    return torch.cat((f.real, f.imag), dim=-1).T.contiguous()


def _regions(st):
    """[(canonical offset, shape, effective offset, n)] of every trainable tensor, laid out here from the canonical
    parameter order and the table's widths (tests/test_variant_cases_cpu.py ties fft_n to the table)."""
    out, o, e = [], 0, 0
    for p, n in zip(st.trainable, st.fft_n):
        out.append((o, tuple(p.shape), e, n))
        o += p.numel()
        e += p.numel() if n is None else p.shape[0] * n
    return out, o, e


@pytest.mark.parametrize("name", ["odd", "two_way", "collide", "cfg175"])
def test_fft_fold_and_unfold_maps_vs_fp64(name):
    """refresh(): every region of the effective buffer -- ActNorm and biases bit-exact copies, an FFT weight against
    W[:, :n] + W[:, n:] F64 at 2e-6 (|W[:, :n]| + |W[:, n:]| |F64|) + 1e-6. unfold_grad(G) of a random
    effective-layout G: dW[:, :n] is G bit for bit, dW[:, n:] against G F64^T at the same form, every other entry a
    bit-exact copy; the result has canon's size and every element of it is compared, so every element is written
    (the allocation it lands in is filled with NaN first, as far as the caching allocator hands the block back)."""
    case = case_of(name)
    st = case.m.fused
    regions, n_canon, n_eff = _regions(st)
    assert st.canon.numel() == n_canon and st.flat.numel() == n_eff and st.flat_param.data_ptr() == st.canon.data_ptr()
    assert [n for _, _, _, n in regions if n is not None] == [n for n, _ in V.fft_weights(name)]
    st.flat.fill_(float("nan"))
    st.refresh()
    flat, canon = st.flat.detach().cpu(), st.canon.detach().cpu()
    assert not torch.isnan(flat).any()
    G = torch.randn(n_eff, generator=torch.Generator().manual_seed(9))
    poison = torch.full_like(st.canon, float("nan"))
    del poison
    g = st.unfold_grad(G.to(DEV))
    assert g.shape == st.canon.shape and g.dtype == torch.float32
    g = g.cpu()
    assert not torch.isnan(g).any()
    worst_fold = worst_unfold = 0.0
    for o, shape, e, n in regions:
        k = int(np.prod(shape))
        if n is None:
            assert torch.equal(flat[e:e + k], canon[o:o + k]), (name, o)
            assert torch.equal(g[o:o + k], G[e:e + k]), (name, o)
            continue
        rows, width = shape
        assert width == n + 2 * (n // 2 + 1)
        F = _f64(n)
        W = canon[o:o + k].view(rows, width).double()
        ref = W[:, :n] + W[:, n:] @ F
        tol = 2e-6 * (W[:, :n].abs() + W[:, n:].abs() @ F.abs()) + 1e-6
        err = (flat[e:e + rows * n].view(rows, n).double() - ref).abs()
        worst_fold = max(worst_fold, float((err / tol).max()))
        assert bool((err <= tol).all()), (name, "fold", o, n, float(err.max()))
        Gi = G[e:e + rows * n].view(rows, n)
        dW = g[o:o + k].view(rows, width)
        assert torch.equal(dW[:, :n], Gi), (name, "unfold identity part", o)
        ref = Gi.double() @ F.T
        tol = 2e-6 * (Gi.double().abs() @ F.T.abs()) + 1e-6
        err = (dW[:, n:].double() - ref).abs()
        worst_unfold = max(worst_unfold, float((err / tol).max()))
        assert bool((err <= tol).all()), (name, "unfold", o, n, float(err.max()))
    print(f"\nVARIANT_FP64 {case.name} fold-maps: refresh {worst_fold:.3f} unfold_grad {worst_unfold:.3f} of the gate "
          f"({len(V.fft_groups(name))} width groups)")


# ------------------------------------------------------------------------------------------ b. eval parity
EVAL = [(n, None) for n in V.CASES] + [("odd", 1), ("glu_odd", 1)]


@pytest.mark.parametrize("name,B", EVAL, ids=[f"{n}-B{B or V.CASES[n]['B']}" for n, B in EVAL])
def test_eval_step_vs_fp64_oracle(name, B):
    """Eval mode at every case (feat / glu_feat through O.feature_forward): z, ldj, log_prob and the inverse at VAL,
    every parameter gradient, dL/dy and dL/dh at GRAD; as many gradients compared as the state dict has trainable
    entries."""
    case, ref = case_of(name, B), eval_ref(name, B)
    got = gpu_run(case, "unfused", training=False) if case.wide else glu_run(case, "unfused", training=False)[0]
    rows = compare(got, ref)
    assert len(got["grads"]) == _trainable(case.sd) == sum(1 for r in rows if r[0].startswith("grad/"))
    vals = _gpu_values(case.m, case.y, case.cond, _latents(case))
    rows += [val_row(k, vals[k], ref[k]) for k in ("log_prob", "inverse")]
    settle(case.name, "eval", rows)


# ------------------------------------------------------------------------------------------ c. training mode
FFT_TRAIN = ["odd", "two_way", "cfg175", "feat"]


@functools.lru_cache(maxsize=None)
def fft_train_case(name):
    """The case with the fp64 training step under the host restatement of the masks of a launch at (seed, OFFSET)
    (wide_case of tests/test_gpu_train_parity.py for an FFTWideStack, which runs the same kernels), and the masks of
    one saving forward launch read from its records for the independence checks."""
    case = case_of(name)
    case.m.train()
    case.masks = _wide_records(case, OFFSET)
    case.ref = oracle_run(case, wide_keep(case, OFFSET, case.y.shape[0]))
    return case


@pytest.mark.parametrize("name", FFT_TRAIN)
def test_fft_record_masks_are_independent_draws(name):
    """The condition that keeps a degenerate mask read from hiding a failure, at the FFT cases."""
    assert_record_masks_are_independent_draws(fft_train_case(name))


@pytest.mark.parametrize("path", ["unfused", "fused"])
@pytest.mark.parametrize("name", FFT_TRAIN)
def test_fft_training_step_vs_fp64_oracle(name, path):
    """Dropout on, the launch's own masks handed to the oracle. unfused: m() + inn_nll_loss + autograd (the backward
    through unfold_grad); fused: nll_loss. An FFTWideStack takes no feature fold: stated for `feat`, not assumed."""
    case = fft_train_case(name)
    if name == "feat":
        with torch.no_grad():
            assert case.m.fold_features and case.m._wide_fold(case.y.to(DEV), (case.cond.to(DEV),)) is None
    rows = compare(gpu_run(case, path), case.ref)
    assert sum(1 for r in rows if r[0].startswith("grad/")) == _trainable(case.sd)
    settle(case.name, path + "-train", rows)


@pytest.mark.parametrize("path", ["unfused", "fused"])
@pytest.mark.parametrize("name", ["glu_odd", "glu_identity"])
def test_anyglu_training_step_vs_fp64_oracle(name, path):
    """The layerwise stack's dropout is nn.Dropout: each module's keep mask is recorded by a forward hook and fed to
    the oracle in its (coupling, half, layer) order, which is the call order. unfused: m() + inn_nll_loss; fused: the
    layerwise nll_loss."""
    case = case_of(name)
    s = case.spec
    got, masks = glu_run(case, path)
    S, NH = (2 if s.two_way else 1), len(s.nested_sizes)
    assert len(masks) == s.n_blocks * S * NH
    assert all(tuple(k.shape) == (case.y.shape[0], s.nested_sizes[0]) for k in masks)
    kept = torch.stack(masks).double()
    p = s.dropout
    assert abs(1.0 - kept.mean().item() - p) <= 4 * np.sqrt(p * (1 - p) / kept.numel())
    ref = oracle_run(case, lambda k, half, li: masks[(k * S + (half == "b")) * NH + li])
    rows = compare(got, ref)
    assert sum(1 for r in rows if r[0].startswith("grad/")) == _trainable(case.sd)
    settle(case.name, path + "-train", rows)


# ------------------------------------------------------------------------------------------ d. TrainStep, FFT model
def _train_model(dropout=None):
    m, spec, sd = V.build("feat", dropout=dropout)
    assert type(m.fused).__name__ == "FFTWideStack"
    return m.to(DEV).train(), spec, sd


def test_fft_trainstep_graph_replay_equals_eager():
    """HIP-graph TrainStep on an FFT model == eager TrainStep over 3 dropout steps, bit for bit: losses, every
    parameter, RNG offset 3. refresh() runs before every launch, so it has to be part of the captured step: a graph
    that replayed the kernels on the effective weights of capture time would train on stale weights from step 2 on."""
    from bcnf_amd.train import TrainStep
    gen = torch.Generator().manual_seed(11)
    B = V.CASES["feat"]["B"]
    pool_y = torch.randn(256, 19, generator=gen).to(DEV)
    pool_t = torch.randn(256, 30, 3, generator=gen).to(DEV)
    idxs = [torch.randperm(256, generator=gen)[:B].to(DEV) for _ in range(3)]
    res = []
    for capture in (False, True):
        m, _, _ = _train_model()
        assert m.dropout == 0.3
        m.fused.set_seed(77)
        st = TrainStep(m, lr=2e-4, capture=capture)
        assert st.capture == capture and not st.layerwise
        st.set_pool(pool_y, pool_t)
        losses = [st.step_indexed(i) for i in idxs]
        res.append((losses, [p.detach().clone() for p in m.parameters()], int(m.fused.rng_state()[1].item())))
    (l0, p0, r0), (l1, p1, r1) = res
    assert l0 == l1 and r0 == r1 == 3, (l0, l1, r0, r1)
    assert all(np.isfinite(v) for step in l0 for v in step) and len(set(step[0] for step in l0)) == 3
    for a, b in zip(p0, p1):
        assert torch.equal(a, b)


@functools.lru_cache(maxsize=None)
def _adam_reference():
    """Three Trainer steps (O.train_step_cpu) on `feat` with dropout 0 in float64 with torch.optim.Adam(lr = LR) on
    the reference-layout parameters, the same batch each step: the losses, the clipped gradients step 1 leaves in
    .grad, and the unclipped gradients at the initial weights."""
    _, spec, sd = V.build("feat", dropout=0.0)
    y, traj = V.inputs("feat")
    case = types.SimpleNamespace(spec=spec, sd=sd, y=y, cond=traj)
    unclipped = oracle_run(case, None, training=False)["grads"]
    sdp = {k: v.double().clone().requires_grad_(not k.endswith("orthonormal_matrix")) for k, v in sd.items()}
    opt = torch.optim.Adam([p for p in sdp.values() if p.requires_grad], lr=LR)
    losses, clipped = [], None
    for step in range(3):
        losses.append(O.train_step_cpu(sdp, spec, y.double(), traj.double(), opt)[0])
        if step == 0:
            clipped = {k: v.grad.clone() for k, v in sdp.items() if v.grad is not None}
    return types.SimpleNamespace(spec=spec, sd=sd, y=y, traj=traj, losses=losses, clipped=clipped, unclipped=unclipped)


def _loss_gate(ref):
    return 1e-5 * abs(ref) + 1e-5


def _left_grads(m):
    """{state_dict name: .grad} as a TrainStep leaves it: the coupling stack's one flat leaf cut along the canonical
    parameter order, the feature network's parameters as they are."""
    st = m.fused
    names = {id(p): n for n, p in m.named_parameters()}
    flat = st.flat_param.grad
    assert flat is not None and flat.numel() == sum(p.numel() for p in st.trainable)
    out, off = {}, 0
    for p in st.trainable:
        out[names[id(p)]] = flat[off:off + p.numel()].view(p.shape).detach().cpu().clone()
        off += p.numel()
    for n, p in m.feature_network_stack.named_parameters():
        if p.requires_grad:
            out["feature_network_stack." + n] = p.grad.detach().cpu().clone()
    return out


@pytest.mark.parametrize("capture", [False, True], ids=["eager", "graph"])
def test_fft_trainstep_vs_fp64_adam_and_nothing_stale_after(capture):
    """TrainStep (FusedAdam on the canonical flat leaf, clip after the step) on `feat` with dropout 0, three steps on
    one batch, against _adam_reference:
      * each step's loss within 1e-5 |ref| + 1e-5 -- steps 2 and 3 see the updated weights only if refresh() ran on
        them;
        the reference's own loss moves by >= 100 x that gate from step 1 to step 2 (asserted on the reference alone);
      * after step 1 every parameter's .grad (clipped on both sides) at GRAD per state_dict name: the layout Adam got;
      * after step 1, wherever the oracle's unclipped |g| > 1e-3 max|g| of its tensor, the parameter moved by LR within
        1 % against the sign of g (Adam's first step is lr g / (|g| + 1e-8)).
    Then, with no call in between, the model's current state_dict goes into the fp64 oracle and eval-mode log_prob,
    inverse and sample() (which runs inside reuse_pack()) match it at VAL: no stale effective weights or pack."""
    from bcnf_amd.train import TrainStep
    ref = _adam_reference()
    assert abs(ref.losses[1] - ref.losses[0]) >= 100 * _loss_gate(ref.losses[0]), ref.losses
    m, spec, sd = _train_model(0.0)
    ts = TrainStep(m, lr=LR, capture=capture)
    assert ts.capture == capture and not ts.layerwise
    y, traj = ref.y.to(DEV), ref.traj.to(DEV)
    rows = []
    for step in range(3):
        loss, nll, mse = ts.step(y, traj)
        assert nll == loss and mse == 0.0
        bound = _loss_gate(ref.losses[step])
        rows.append((f"loss{step + 1}", abs(loss - ref.losses[step]) <= bound, abs(loss - ref.losses[step]) / bound))
        if step == 0:
            grads = _left_grads(m)
            assert set(grads) == set(ref.clipped)
            rows += [("grad/" + k, close(g, ref.clipped[k], **GRAD)[0], _ratio(g, ref.clipped[k], **GRAD))
                     for k, g in grads.items()]
            now = {k: v.detach().cpu() for k, v in m.state_dict().items()}
            moved, checked = 0.0, 0
            for k, g in ref.unclipped.items():
                big = g.abs() > 1e-3 * g.abs().max()
                dev = ((now[k].double() - sd[k].double()) + LR * g.sign()).abs()[big]
                moved, checked = max(moved, float(dev.max()) / (0.01 * LR)), checked + int(big.sum())
            assert checked > 0.9 * sum(g.numel() for g in ref.unclipped.values())
            rows.append(("adam-first-step", moved <= 1.0, moved))
    # nothing in between: the parameters were last touched by the optimizer's in-place update
    sd64 = _sd64(m.state_dict())
    zl = torch.randn(y.shape[0], spec.size, generator=torch.Generator().manual_seed(5))
    want = _values64(sd64, spec, ref.y, ref.traj, zl)
    vals = _gpu_values(m, ref.y, ref.traj, zl)
    kw = dict(outer=True, batch_size=2, sample_batch_size=5)
    torch.manual_seed(321)
    vals["sample"] = m.sample(8, ref.traj[:3], **kw)
    torch.manual_seed(321)
    want["sample"] = O.sample(sd64, spec, 8, ref.traj[:3].double(), **kw)
    assert vals["sample"].shape == want["sample"].shape == (8, 3, spec.size)
    rows += [val_row(k, vals[k], want[k]) for k in ("z", "ldj", "log_prob", "inverse", "sample")]
    # the trained weights are not the initial ones by far more than the gate, or the comparison above shows nothing
    before = _values64(_sd64(sd), spec, ref.y, ref.traj, zl)
    assert all(not close(before[k], want[k], **VAL)[0] for k in ("z", "ldj", "inverse"))
    settle("feat-B%d" % y.shape[0], "trainstep-" + ("graph" if capture else "eager"), rows)


@pytest.mark.parametrize("first", ["forward", "inverse", "sample"])
def test_fft_inplace_weight_update_reaches_every_entry_point(first):
    """The same staleness check without a TrainStep: after forward, inverse and sample() have run once (every pack and
    the effective buffer built), one FFT weight is scaled in place by 1.01 and `first` is the first call after it --
    launch_forward's refresh(), launch_inverse's (outside a frozen pack) or reuse_pack()'s has to pick the change up on
    its own, since any of them run earlier would hide a stale one. That call and then the others match the oracle on the
    new weights at VAL. The change moves the oracle's own z, ldj, inverse and samples by >= 10 x the gate."""
    m, spec, sd = V.build("odd")
    m.to(DEV).eval()
    y, cond = V.inputs("odd")
    zl = torch.randn(y.shape[0], spec.size, generator=torch.Generator().manual_seed(5))
    kw = dict(outer=True, batch_size=2, sample_batch_size=5)

    def sample(model_or_sd):
        torch.manual_seed(321)
        if isinstance(model_or_sd, dict):
            return O.sample(model_or_sd, spec, 8, cond[:3].double(), **kw)
        return model_or_sd.sample(8, cond[:3], **kw)

    _gpu_values(m, y, cond, zl)
    sample(m)
    name = "layers.3.nn_a.nn.0.linear.weight"
    with torch.no_grad():
        dict(m.named_parameters())[name].mul_(1.01)
    vals = {}
    if first == "sample":
        vals["sample"] = sample(m)
    elif first == "inverse":
        with torch.no_grad():
            vals["inverse"] = m.inverse(zl.to(DEV), cond.to(DEV)).cpu()
    vals = {**_gpu_values(m, y, cond, zl), **vals}
    vals.setdefault("sample", sample(m))
    sd64 = _sd64(m.state_dict())
    assert not torch.equal(sd64[name], sd[name].double())
    assert all(torch.equal(v, sd[k].double()) for k, v in sd64.items() if k != name)
    want, before = _values64(sd64, spec, y, cond, zl), _values64(_sd64(sd), spec, y, cond, zl)
    want["sample"], before["sample"] = sample(sd64), sample(_sd64(sd))
    for k in ("z", "ldj", "inverse", "sample"):
        assert _ratio(before[k], want[k], **VAL) >= 10.0, (k, _ratio(before[k], want[k], **VAL))
    settle("odd-B%d" % y.shape[0], f"inplace-update-{first}-first",
           [val_row(k, vals[k], want[k]) for k in ("z", "ldj", "log_prob", "inverse", "sample")])


# ------------------------------------------------------------------------------------------ e. sampling
@pytest.mark.parametrize("name", ["odd", "glu_odd"])
def test_sample_and_its_log_prob_vs_fp64_oracle(name):
    """sample(outer=True) over 5 conditions in chunks of 3, 12 draws in chunks of 5, against O.sample under the same
    torch.manual_seed at VAL; with return_log_prob=True the same draws bit for bit, and their log-density against the
    oracle's log_prob at its own inverse, at the gate of tests/test_gpu_sample_logprob.py (its condition on the inputs
    included: the couplings move ldj by >= 100 x what the gate lets through)."""
    case = case_of(name)
    m, spec = case.m.eval(), case.spec
    cond = case.cond[:5]
    kw = dict(outer=True, batch_size=3, sample_batch_size=5)
    torch.manual_seed(123)
    got = m.sample(12, cond, **kw)
    torch.manual_seed(123)
    want = O.sample(_sd64(case.sd), spec, 12, cond.double(), **kw)
    assert got.shape == want.shape == (12, 5, spec.size)
    torch.manual_seed(123)
    s, lp = m.sample(12, cond, return_log_prob=True, **kw)
    assert torch.equal(s, got) and lp.shape == (12, 5)
    ref = _sample_reference(case.sd, spec, cond, 123, 12, 3, 5, True)
    rows = [val_row("sample", got, want), val_row("sample-vs-replayed-stream", got, ref["y64"])]
    settle(case.name, "sample", rows)
    _gate_lp(f"VARIANT_FP64 {case.name} sample-log_prob", lp.reshape(-1),
             {k: v.reshape(-1, *v.shape[2:]) for k, v in ref.items()})
