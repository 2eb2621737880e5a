"""GPU tests of the fused hybrid (NLL + prediction-head MSE) training step: the head kernels against torch fp64,
CondRealNVP_v2.hybrid_loss and TrainStep(hybrid_weight=w) against the reference's fixture
(tests/golden/g15_hybrid.npz, cases a / b / c of tests/golden/make_golden_hybrid.py), the fused route against the
generic one, run_epoch against the per-step loop, and the divergence guard on the combined loss.

Gates. Values (r, mse, the three logged values): 1e-5, the project's forward gate. Gradients: the project's
close(rtol=1e-4, floor=1e-4) and, because the head's gradients are ~1e-3 (far below that gate's floor), also
max|a - b| <= 1e-4 * max|b|, relative to the tensor's own scale. torch's own fp32 result on the CPU meets the head
test's gates against fp64 at every shape used here with a factor >= 20 to spare (worst: r at K = 1360, 0.047 of the
gate), so the gates are not set by what the kernels give."""
import ctypes

import numpy as np
import pytest
import torch

from conftest import close, golden_sd, load_golden
from test_hybrid_cpu import CASES, Case, case_config

pytestmark = pytest.mark.gpu

DEV = "cuda"


def t(x):
    return torch.from_numpy(np.ascontiguousarray(x)).to(DEV)


@pytest.fixture(scope="module")
def g15():
    return load_golden("g15_hybrid.npz")


def scale_close(a, b, rel=1e-4):
    """max|a - b| <= rel * max|b| (b: the reference)."""
    a = torch.as_tensor(a, dtype=torch.float64)
    b = torch.as_tensor(b, dtype=torch.float64)
    err = float((a - b).abs().max())
    return err <= rel * float(b.abs().max()), err


def case_model(c, train=False, seed=0):
    from bcnf_amd import CondRealNVP_v2
    torch.manual_seed(seed)
    m = CondRealNVP_v2.from_config(case_config(c.cfg))
    m.load_state_dict(golden_sd(c.d))
    m.to(DEV)
    m.train(train)
    return m


# ------------------------------------------------------------------------------------------ head kernels
HEAD_SHAPES = [(1, 1, 2, 1), (17, 5, 3, 5), (50, 32, 21, 32), (17, 37, 19, 40), (300, 512, 21, 512),
               (64, 1360, 32, 1360)]


def _head_run(x, W, bias, y, w, dloss, dx_init, accumulate):
    """One forward + finalize + backward through the C-ABI; returns (r, vals, dW, dbias, dx, workspace)."""
    from bcnf_amd import _native as N
    from bcnf_amd import fused as F
    B, D = y.shape
    K = W.shape[1]
    work = F.head_workspace(B, K, D, x.device)
    work.fill_(float("nan"))
    xk = x[:, :K]                                      # rows ldx apart
    F.launch_head_forward(xk, W, bias, y, work)
    vals = torch.tensor([3.0, 3.0, 0.0], device=x.device)          # what the stack's finalize leaves: [nll, nll, 0]
    F.launch_hybrid_finalize(vals, work, B, D, w, None)
    dW = torch.full_like(W, float("nan"))
    db = torch.full((D,), float("nan"), device=x.device)
    dx = dx_init.clone()
    N.check(N.lib().bcnf_head_mse_backward(N.ptr(x), x.stride(0), K, N.ptr(W), N.ptr(work), N.ptr(dloss),
                                           ctypes.c_float(w), B, D, N.ptr(dW), N.ptr(db), N.ptr(dx), dx.stride(0),
                                           int(accumulate), N.stream_handle(x.device)), "bcnf_head_mse_backward")
    torch.cuda.synchronize()
    return work[:B * D].view(B, D).clone(), vals, dW, db, dx, work


@pytest.mark.parametrize("with_bias", [True, False])
@pytest.mark.parametrize("B,K,D,ldx", HEAD_SHAPES)
def test_head_kernels_match_fp64(B, K, D, ldx, with_bias):
    """r, mse / loss, dW, dbias and dx (overwriting and accumulating into a random buffer of dx's own scale) against
    torch fp64; x's padding columns K .. ldx hold NaN and must reach no output; two calls are bit-identical."""
    gen = torch.Generator().manual_seed(1000 + B + K + D)
    x = torch.randn(B, ldx, generator=gen)
    W = torch.randn(D, K, generator=gen) / K ** 0.5
    bias = 0.1 * torch.randn(D, generator=gen)
    y = torch.randn(B, D, generator=gen)
    w = 0.5
    dloss = torch.tensor([0.7, 0.3, 0.2])
    g = 0.7 * w / (1 + w) + 0.2
    x64, W64, y64 = x[:, :K].double(), W.double(), y.double()
    r64 = x64 @ W64.T + (bias.double() if with_bias else 0.0) - y64
    mse64 = (r64 * r64).mean()
    e64 = (2 * g / (B * D)) * r64
    dW64, db64, dx64 = e64.T @ x64, e64.sum(0), e64 @ W64
    buf = torch.randn(B, ldx, generator=gen) * float(dx64.abs().max())
    x[:, K:] = float("nan")
    buf[:, K:] = 7.0
    xg, Wg, yg, bg = x.to(DEV), W.to(DEV), y.to(DEV), (bias.to(DEV) if with_bias else None)
    dl = dloss.to(DEV)
    outs = []
    for accumulate in (False, True, True):
        init = buf.to(DEV) if accumulate else torch.full((B, ldx), 7.0, device=DEV)
        outs.append(_head_run(xg, Wg, bg, yg, w, dl, init, accumulate))
    for accumulate, (r, vals, dW, db, dx, _) in zip((False, True), outs[:2]):
        checks = [("r", r, r64, 1e-5 * max(1.0, float(r64.abs().max()))),
                  ("mse", vals[2], mse64, 1e-5 * max(1.0, float(mse64))),
                  ("loss", vals[0], (3.0 + w * mse64) / (1 + w), 1e-5 * max(1.0, float((3.0 + w * mse64) / (1 + w)))),
                  ("dW", dW, dW64, 1e-4 * float(dW64.abs().max())),
                  ("dbias", db, db64, 1e-4 * float(db64.abs().max())),
                  ("dx", dx[:, :K], dx64 + (buf[:, :K].double() if accumulate else 0.0),
                   1e-4 * float((dx64 + (buf[:, :K].double() if accumulate else 0.0)).abs().max()))]
        for name, got, ref, lim in checks:
            got = got.detach().double().cpu()
            assert torch.isfinite(got).all(), (name, accumulate)
            err = float((got - ref).abs().max())
            print(f"{name} accumulate={accumulate}: err {err:.3e} limit {lim:.3e}")
            assert err <= lim, (name, accumulate, err, lim)
        assert float(vals[1]) == 3.0
        assert torch.equal(dx[:, K:], torch.full((B, ldx - K), 7.0, device=DEV))      # padding columns untouched
    # the same launches on the same inputs: the same bits, the workspace (residual + every partial) included
    for a, b in zip(outs[1][:5], outs[2][:5]):
        assert torch.equal(a, b)
    wa, wb = outs[1][5], outs[2][5]
    assert torch.equal(torch.nan_to_num(wa, nan=-1.0), torch.nan_to_num(wb, nan=-1.0))


def test_head_null_cotangent_and_nullable_outputs():
    """dloss = NULL means [1, 0, 0]; each output alone equals the same output of the full call, bit for bit."""
    from bcnf_amd import _native as N
    from bcnf_amd import fused as F
    B, K, D = 50, 32, 21
    gen = torch.Generator().manual_seed(5)
    x, W, y = (torch.randn(s, generator=gen).to(DEV) for s in ((B, K), (D, K), (B, D)))
    work = F.head_workspace(B, K, D, DEV)
    F.launch_head_forward(x, W, None, y, work)
    L, st = N.lib(), N.stream_handle(torch.device(DEV))

    def bwd(dloss, dW, db, dx):
        N.check(L.bcnf_head_mse_backward(N.ptr(x), K, K, N.ptr(W), N.ptr(work), N.ptr(dloss), ctypes.c_float(1.0), B,
                                         D, N.ptr(dW), N.ptr(db), N.ptr(dx), K, 0, st), "bcnf_head_mse_backward")

    full = [torch.empty(D, K, device=DEV), torch.empty(D, device=DEV), torch.empty(B, K, device=DEV)]
    bwd(torch.tensor([1.0, 0.0, 0.0], device=DEV), *full)
    null = [torch.empty_like(v) for v in full]
    bwd(None, *null)
    for a, b in zip(full, null):
        assert torch.equal(a, b)
    for i in range(3):
        only = [None, None, None]
        only[i] = torch.empty_like(full[i])
        bwd(None, *only)
        assert torch.equal(only[i], full[i]), i
    bwd(None, None, None, None)
    torch.cuda.synchronize()


# ------------------------------------------------------------------------------------------ hybrid_loss
@pytest.mark.parametrize("name", ["a", "b", "c"])
def test_hybrid_loss_matches_reference(g15, name):
    """vals = [loss, nll, mse] and every gradient (dL/dh included) of the reference's hybrid step, eval mode."""
    c = Case(g15, name)
    m = case_model(c)
    feats = []

    def keep_features(mod, inp, out):       # h, with its gradient kept (returns None: the output is not replaced)
        out.retain_grad()
        feats.append(out)

    hook = m.feature_network_stack.register_forward_hook(keep_features)
    vals = m.hybrid_loss(t(c["y"]), t(c["traj"]), hybrid_weight=c.cfg["w"])
    hook.remove()
    v = vals.detach().cpu()
    for i, key in enumerate(("loss", "nll", "mse")):
        ref = float(c[key])
        print(f"{key}: {v[i].item():.7f} ref {ref:.7f}")
        assert abs(v[i].item() - ref) <= 1e-5 * abs(ref) + 1e-5, (key, v[i].item(), ref)
    torch.autograd.backward(vals, torch.tensor([1.0, 0.0, 0.0], device=DEV))
    assert torch.equal(vals.detach().cpu(), v)              # not deferred: the backward leaves the values alone
    (h,) = feats
    ok, err = close(h.grad.cpu(), c["dh"], rtol=1e-4, floor=1e-4)
    assert ok, f"dL/dh max err {err}"
    ok, err = scale_close(h.grad.cpu(), c["dh"])
    assert ok, f"dL/dh (own scale) max err {err}"
    named = dict(m.named_parameters())
    n_checked = 0
    for k in c.keys():
        if not k.startswith("grad/"):
            continue
        pname = k[5:]
        got = named[pname].grad.cpu()
        ok, err = close(got, c[k], rtol=1e-4, floor=1e-4)
        assert ok, (pname, err)
        if pname.startswith("prediction_head."):
            ok, err = scale_close(got, c[k])
            assert ok, (pname, "own scale", err)
        n_checked += 1
    assert n_checked == len([k for k in c.keys() if k.startswith("grad/")]) > 20
    # no_grad: the finalized validation triple, no RNG advance in eval mode
    off = int(m.fused.rng_state()[1].item())
    with torch.no_grad():
        v2 = m.hybrid_loss(t(c["y"]), t(c["traj"]), hybrid_weight=c.cfg["w"])
    assert torch.equal(v2.cpu(), v) and int(m.fused.rng_state()[1].item()) == off


# ------------------------------------------------------------------------------------------ TrainStep
@pytest.mark.parametrize("capture", [False, True])
@pytest.mark.parametrize("name", ["a", "b", "c"])
def test_trainstep_hybrid_matches_reference_step(g15, name, capture):
    """One TrainStep(hybrid_weight=w) == the reference's backward + Adam(lr 2e-4).step() + clip_grad_norm_(1.0)."""
    from bcnf_amd.train import TrainStep
    c = Case(g15, name)
    m = case_model(c)
    st = TrainStep(m, lr=2e-4, hybrid_weight=c.cfg["w"], capture=capture)
    assert st.hybrid
    loss, nll, mse = st.step(t(c["y"]), t(c["traj"]))
    for got, key in ((loss, "loss"), (nll, "nll"), (mse, "mse")):
        ref = float(c[key])
        assert abs(got - ref) <= 1e-5 * abs(ref) + 1e-5, (key, got, ref)
    named = dict(m.named_parameters())
    n = 0
    for k in c.keys():
        if k.startswith("after/"):
            ok, err = close(named[k[6:]].detach().cpu(), c[k], rtol=1e-5, floor=1e-5)
            assert ok, (k, err)
            n += 1
    assert n == len(named)
    ref_norm = float(c["clip_total_norm"])
    assert abs(float(st.last_clip_norm) - ref_norm) <= 1e-4 * ref_norm, (float(st.last_clip_norm), ref_norm)


@pytest.mark.parametrize("name", ["a", "c"])
def test_fused_step_equals_unfused_step_with_dropout(g15, name):
    """Train mode, dropout 0.5, same seed: one step on the generic route (fuse_hybrid off: torch nn.Linear + MSELoss +
    autograd) and one on the fused route from the same state: logged values to 1e-5 relative, parameters within
    close(1e-5, 1e-5), the same Philox offset afterwards (hence the same masks)."""
    from bcnf_amd.train import TrainStep
    c = Case(g15, name)
    res = []
    for fuse in (False, True):
        m = case_model(c, train=True)
        m.fused.set_seed(1234)
        st = TrainStep(m, lr=2e-4, hybrid_weight=c.cfg["w"], capture=False)
        st.fuse_hybrid = fuse
        assert st.hybrid == fuse
        vals = st.step(t(c["y"]), t(c["traj"]))
        res.append((vals, [p.detach().cpu() for p in m.parameters()], int(m.fused.rng_state()[1].item())))
    (v0, p0, r0), (v1, p1, r1) = res
    assert r0 == r1 == 1
    for a, b in zip(v0, v1):
        assert abs(a - b) <= 1e-5 * abs(a), (v0, v1)
    assert v0[2] > 0.0
    for a, b in zip(p0, p1):
        ok, err = close(b, a, rtol=1e-5, floor=1e-5)
        assert ok, err


@pytest.mark.parametrize("unroll", [8, 3])
def test_hybrid_run_epoch_equals_per_step_loop(g15, unroll):
    """Case c model, train mode, pool of 768 rows, batch 48: run_epoch (multi-step graphs, hidden clips, one sync) ==
    the step_epoch loop bit for bit: the 16 logged triples, parameters, Adam state, RNG offset, cursor."""
    from bcnf_amd.train import TrainStep
    c = Case(g15, "c")
    gen = torch.Generator().manual_seed(21)
    py = torch.randn(768, 19, generator=gen).to(DEV)
    pt = torch.randn(768, 30, 3, generator=gen).to(DEV)
    order = torch.randperm(768, generator=gen).to(DEV)
    res = []
    for batched in (False, True):
        m = case_model(c, train=True)
        m.fused.set_seed(5)
        st = TrainStep(m, lr=2e-4, hybrid_weight=1.0)
        st.epoch_unroll = unroll
        st.set_pool(py, pt)
        st.set_epoch(order, 48)
        if batched:
            st.prepare_epoch(15)
            assert len(st._cap.multi) > 0                    # the multi-step graphs exist: hybrid takes the epoch path
            vals = st.run_epoch(1) + st.run_epoch()
        else:
            vals = [st.step_epoch() for _ in range(16)]
        state = [v.clone() for s in st.opt.state.values() for v in s.values()]
        res.append((vals, [p.detach().clone() for p in m.parameters()], state, m.fused.rng_state().clone(),
                    st.walk.cursor.item()))
    (v0, p0, s0, r0, c0), (v1, p1, s1, r1, c1) = res
    assert v0 == v1 and len(v1) == 16
    assert all(v[2] > 0.0 and abs(v[0] - 0.5 * (v[1] + v[2])) <= 1e-5 * abs(v[0]) for v in v1)
    assert c0 == c1 == 0 and torch.equal(r0, r1) and int(r1[1]) == 16
    for i, (a, b) in enumerate(zip(p0 + s0, p1 + s1)):
        assert torch.equal(a, b), (i, float((a.float() - b.float()).abs().max()))


def test_guard_judges_the_combined_loss(g15):
    """prediction_head.bias = 1e4: mse ~ 1e8 and loss > 1e5 while nll stays near 10. The reference judges loss
    (trainer.py:168), so run_epoch(check_divergence=True) halts after batch 0's update with the model, optimizer, RNG
    offset and cursor of exactly one update (a guard that judged nll would run the whole epoch)."""
    from bcnf_amd.train import TrainStep, TrainingDivergedError
    c = Case(g15, "a")
    gen = torch.Generator().manual_seed(33)
    py = torch.randn(200, 21, generator=gen).to(DEV)
    pt = (2.0 * torch.randn(200, 20, 3, generator=gen)).to(DEV)
    order = torch.randperm(200, generator=gen).to(DEV)
    res = []
    for mode in ("eager_one_step", "epoch"):
        m = case_model(c, train=True)
        with torch.no_grad():
            m.prediction_head.bias.fill_(1e4)
        m.fused.set_seed(9)
        st = TrainStep(m, lr=2e-4, hybrid_weight=1.0, capture=mode == "epoch")
        st.epoch_unroll = 2
        st.set_pool(py, pt)
        st.set_epoch(order, 50)
        if mode == "epoch":
            with pytest.raises(TrainingDivergedError, match="at batch 0"):
                st.run_epoch(check_divergence=True)
            assert st.walk.host_cursor == 1
        else:
            loss, nll, mse = st.step_epoch()
            assert loss > 1e5 and nll < 1e3 and mse > 1e7, (loss, nll, mse)
        state = [v.clone() for s in st.opt.state.values() for v in s.values()]
        res.append(([p.detach().clone() for p in m.parameters()], state, m.fused.rng_state().clone(),
                    st.walk.cursor.item()))
    (p0, s0, r0, c0), (p1, s1, r1, c1) = res
    assert c0 == c1 == 1 and torch.equal(r0, r1) and int(r1[1]) == 1
    for a, b in zip(p0 + s0, p1 + s1):
        assert torch.equal(a, b)
    assert float(s1[0]) == 1.0                               # Adam step count: one update applied


@pytest.mark.parametrize("capture", [False, True])
def test_zero_weight_leaves_the_head_alone(g15, capture):
    """hybrid=True model, TrainStep(hybrid_weight=0.0): the fused NLL step as before -- mse == 0, loss == nll, and the
    head's parameters get no gradient (FusedAdam skips parameters whose .grad is None) and no update."""
    from bcnf_amd.train import TrainStep
    c = Case(g15, "c")
    m = case_model(c)
    head0 = [p.detach().clone() for p in m.prediction_head.parameters()]
    st = TrainStep(m, lr=2e-4, hybrid_weight=0.0, capture=capture)
    assert not st.hybrid and st.fused_loss
    for _ in range(2):
        loss, nll, mse = st.step(t(c["y"]), t(c["traj"]))
        assert mse == 0.0 and loss == nll
    assert abs(nll - float(c["nll"])) > 0.0                  # the second step ran on updated parameters
    for p, p0 in zip(m.prediction_head.parameters(), head0):
        assert p.grad is None and torch.equal(p.detach(), p0)
    assert m.fused.flat_param.grad is not None
