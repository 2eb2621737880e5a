"""GPU tests of the DualDomainLSTM feature network on the fused LSTM layer kernels of bcnf_lstm.hip: the recurrence
(bcnf_lstm_forward / bcnf_lstm_backward) alone against a float64 nn.LSTM, the refused shapes and their fallback, the
VerboseLSTM module against torch's own LSTM, the networks and a full model against the reference's fixture
(tests/golden/g17_dlstm*.npz), the folded `fc` Linear against the unfolded path, TrainStep (captured against eager, the
t_DLSTM_large shape, a hybrid step) and sample() with its log-density. Values are held to close(1e-5, 1e-5), gradients
to close(1e-4, 1e-4) (tests/conftest.py).

LSTM_CASES reaches all eight arms of LSTM_DISPATCH (H = 16 ... 128), forward and backward, each also in the forward's
gates = NULL form; tests/test_feature_plans_cpu.py enforces it on the CPU against tests/feature_plans.py, so a case
taken out of the list fails there."""
import copy
import math

import pytest
import torch
from torch import nn

from conftest import close, golden_sd
from gpu_guard import DEV, canaries_alive, guarded
from test_dlstm_cpu import MODEL_CFG, build, dlstm_cfg, golden

pytestmark = pytest.mark.gpu


def t(a):
    return torch.from_numpy(a).to(DEV)


# ------------------------------------------------------------------------------------------ the kernels alone
def recurrence_f64(P, W, b, reverse):
    """torch's LSTM cell (i, f, g, o) restated in float64 for the per-step c the module does not return; the test
    holds its h to the float64 nn.LSTM's."""
    B, S, H4 = P.shape
    H = H4 // 4
    h = P.new_zeros(B, H)
    c = P.new_zeros(B, H)
    hs, cs = [None] * S, [None] * S
    for s in (range(S - 1, -1, -1) if reverse else range(S)):
        i, f, g, o = (P[:, s] + h @ W.T + b).split(H, dim=1)
        c = torch.sigmoid(f) * c + torch.sigmoid(i) * torch.tanh(g)
        h = torch.sigmoid(o) * torch.tanh(c)
        hs[s], cs[s] = h, c
    return torch.stack(hs, 1), torch.stack(cs, 1)


LSTM_CASES = [(1, 1, 16, 1),         # a lone row, one step
              (12, 30, 16, 2),       # a partial tile
              (17, 16, 32, 2),       # one tile plus one row; the frequency branch's S
              (33, 30, 48, 1),       # H not a power of two; three tiles
              (16, 2, 64, 2),        # a full tile
              (5, 30, 128, 2),       # the widest form: 128 weight registers per lane
              (40, 16, 128, 1),
              (17, 3, 80, 2),        # the arms of LSTM_DISPATCH no shipped config takes: H = 80,
              (5, 4, 96, 1),         # 96
              (20, 2, 112, 2),       # and 112
              (3, 1, 32, 2)]         # one step in both directions


def lstm_inputs(B, S, H, dirs):
    gen = torch.Generator().manual_seed(100 * H + S + B)
    P = (2.0 * torch.randn(dirs, B, S, 4 * H, generator=gen)).float()
    W = (3.0 * (2.0 * torch.rand(dirs, 4 * H, H, generator=gen) - 1.0) / math.sqrt(H)).float()   # some gates saturate
    b = (0.1 * torch.randn(dirs, 4 * H, generator=gen)).float()
    dout = torch.randn(B, S, dirs * H, generator=gen).float()
    return P, W, b, dout


def lstm_reference(P, W, b, dout):
    """float64 nn.LSTM over the fp32 values the kernel sees: its input is [P_fwd | P_rev] and W_ih selects each
    direction's block (an exact product), so the gradient of the input IS dP."""
    dirs, B, S, H4 = P.shape
    H = H4 // 4
    ref = nn.LSTM(dirs * H4, H, bidirectional=dirs == 2, batch_first=True).double()
    with torch.no_grad():
        for d, suffix in enumerate(("", "_reverse")[:dirs]):
            sel = torch.zeros(H4, dirs * H4, dtype=torch.float64)
            sel[:, d * H4:(d + 1) * H4] = torch.eye(H4, dtype=torch.float64)
            getattr(ref, "weight_ih_l0" + suffix).copy_(sel)
            getattr(ref, "bias_ih_l0" + suffix).zero_()
            getattr(ref, "weight_hh_l0" + suffix).copy_(W[d].double())
            getattr(ref, "bias_hh_l0" + suffix).copy_(b[d].double())
    x = torch.cat(list(P.double()), dim=-1).requires_grad_(True)
    out = ref(x)[0]
    out.backward(dout.double())
    cells = []
    for d in range(dirs):
        h, c = recurrence_f64(P[d].double(), W[d].double(), b[d].double(), reverse=d == 1)
        assert float((h - out.detach()[..., d * H:(d + 1) * H]).abs().max()) <= 1e-12
        cells.append(c)
    return out.detach(), torch.stack(cells), torch.stack(x.grad.split(H4, dim=-1))


@pytest.mark.parametrize("B,S,H,dirs", LSTM_CASES)
def test_lstm_kernels_against_float64(B, S, H, dirs):
    from bcnf_amd import _native as N
    P, W, b, dout = lstm_inputs(B, S, H, dirs)
    out_ref, c_ref, dp_ref = lstm_reference(P, W, b, dout)
    rows = B * S
    st = N.stream_handle(torch.device(DEV, torch.cuda.current_device()))
    Wd, bd = W.to(DEV), b.to(DEV)
    rev = dirs - 1                                                       # index of the second direction, or the first
    for pad in (0, 5):
        ldp, ldo = 4 * H + pad, dirs * H + pad
        Pg = [guarded(rows, 4 * H, ldp, P[d].reshape(rows, 4 * H).to(DEV))[1] for d in range(dirs)]
        dg = guarded(rows, dirs * H, ldo, dout.reshape(rows, dirs * H).to(DEV))[1]
        runs = []
        for _ in range(2):
            ob, ov = guarded(rows, dirs * H, ldo)
            gb, gv = guarded(dirs * rows, 4 * H)
            cb, cv = guarded(dirs * rows, H)
            dps = [guarded(rows, 4 * H, ldp) for _ in range(dirs)]
            N.call("bcnf_lstm_forward", Pg[0], Pg[rev] if dirs == 2 else None, ldp, Wd[0],
                   Wd[rev] if dirs == 2 else None, bd[0], bd[rev] if dirs == 2 else None, B, S, H, dirs, ov, ldo, gv,
                   cv, st)
            N.call("bcnf_lstm_backward", dg, ldo, gv, cv, Wd[0], Wd[rev] if dirs == 2 else None, B, S, H, dirs,
                   dps[0][1], dps[rev][1] if dirs == 2 else None, ldp, st)
            torch.cuda.synchronize()
            assert canaries_alive(ob, rows, dirs * H, ldo), (pad, "out canary")
            assert canaries_alive(gb, dirs * rows, 4 * H) and canaries_alive(cb, dirs * rows, H), (pad, "save canary")
            for buf, _ in dps:
                assert canaries_alive(buf, rows, 4 * H, ldp), (pad, "dP canary")
            runs.append([ov.clone(), gv.clone(), cv.clone()] + [v.clone() for _, v in dps])
        for a, c in zip(*runs):
            assert torch.equal(a, c)                                     # fixed-order sums: the same bits
        ov, gv, cv, *dpv = runs[0]
        ok, err = close(ov.cpu(), out_ref.reshape(rows, dirs * H))
        print(f"out pad={pad} err={err:.3e}")
        assert ok, ("out", pad, err)
        ok, err = close(cv.cpu().view(dirs, B, S, H), c_ref)
        print(f"c pad={pad} err={err:.3e}")
        assert ok, ("c", pad, err)
        for d in range(dirs):
            ok, err = close(dpv[d].cpu().view(B, S, 4 * H), dp_ref[d], rtol=1e-4, floor=1e-4)
            print(f"dP[{d}] pad={pad} err={err:.3e}")
            assert ok, ("dP", d, pad, err)
        # the module's no_grad form (gates = cells = NULL) saves nothing and gives the same bits
        ob, o2 = guarded(rows, dirs * H, ldo)
        N.call("bcnf_lstm_forward", Pg[0], Pg[rev] if dirs == 2 else None, ldp, Wd[0], Wd[rev] if dirs == 2 else None,
               bd[0], bd[rev] if dirs == 2 else None, B, S, H, dirs, o2, ldo, None, None, st)
        torch.cuda.synchronize()
        assert canaries_alive(ob, rows, dirs * H, ldo), (pad, "out canary, no saves")
        assert torch.equal(o2, ov), (pad, "out without saves")


def against_float64_copy(net, x, what):
    """values and every gradient (input included) of net on the GPU against its float64 CPU copy."""
    ref = copy.deepcopy(net).double().cpu()
    xg = x.clone().requires_grad_(True)
    y = net(xg)[0]
    gen = torch.Generator().manual_seed(9)
    w = torch.randn(y.shape, generator=gen)
    (y * w.to(DEV)).sum().backward()
    xr = x.detach().double().cpu().requires_grad_(True)
    yr = ref(xr)[0]
    (yr * w.double()).sum().backward()
    ok, err = close(y.detach().cpu(), yr.detach())
    assert ok, (what, "out", err)
    ok, err = close(xg.grad.cpu(), xr.grad, rtol=1e-4, floor=1e-4)
    assert ok, (what, "dx", err)
    refp = dict(ref.named_parameters())
    for name, p in net.named_parameters():
        assert p.grad is not None, name
        ok, err = close(p.grad.cpu(), refp[name].grad, rtol=1e-4, floor=1e-4)
        assert ok, (what, name, err)


@pytest.mark.parametrize("B,S,H,dirs", LSTM_CASES)
def test_layer_function_gradients_against_float64(B, S, H, dirs, monkeypatch):
    """dW_hh, db_hh, dW_ih, db_ih and dx of one layer through the autograd Function, W_hh at the kernel test's scale."""
    from bcnf_amd import feature_network as F
    torch.manual_seed(1000 + H + S)
    net = F.VerboseLSTM(5, H, 1, bidirectional=dirs == 2)
    with torch.no_grad():
        for name, p in net.named_parameters():
            if "weight_hh" in name:
                p.copy_(3.0 * (2.0 * torch.rand_like(p) - 1.0) / math.sqrt(H))
    net.to(DEV)
    calls = []
    orig = F._LSTMLayerFn.apply
    monkeypatch.setattr(F._LSTMLayerFn, "apply", lambda *a: (calls.append(1), orig(*a))[1])
    against_float64_copy(net, 2.0 * torch.randn(B, S, 5, device=DEV), (B, S, H, dirs))
    assert len(calls) == 1                                               # the kernels ran, not the nn.LSTM


# ------------------------------------------------------------------------------------------ refused shapes
@pytest.mark.parametrize("H", [20, 144])
def test_hidden_outside_the_limits_is_refused(H):
    from bcnf_amd import _native as N
    B, S = 3, 4
    x = torch.zeros(B * S * 4 * H, device=DEV)
    w = torch.zeros(4 * H * H, device=DEV)
    st = N.stream_handle(x.device)
    assert N.call_raw("bcnf_lstm_forward", x, None, 4 * H, w, None, None, None, B, S, H, 1, x, H, None, None,
                      st) == N.ERR_ARG
    assert N.call_raw("bcnf_lstm_backward", x, H, x, x, w, None, B, S, H, 1, x, None, 4 * H, st) == N.ERR_ARG


def test_row_stride_below_the_row_is_refused():
    from bcnf_amd import _native as N
    B, S, H = 3, 4, 16
    x = torch.zeros(B * S * 4 * H, device=DEV)
    w = torch.zeros(4 * H * H, device=DEV)
    st = N.stream_handle(x.device)
    for ldp, ldo in ((4 * H - 1, H), (4 * H, H - 1)):
        assert N.call_raw("bcnf_lstm_forward", x, None, ldp, w, None, None, None, B, S, H, 1, x, ldo, None, None,
                          st) == N.ERR_ARG
        assert N.call_raw("bcnf_lstm_backward", x, ldo, x, x, w, None, B, S, H, 1, x, None, ldp, st) == N.ERR_ARG
    # two directions: the output row is 2 H wide
    assert N.call_raw("bcnf_lstm_forward", x, x, 4 * H, w, w, None, None, B, S, H, 2, x, 2 * H - 1, None, None,
                      st) == N.ERR_ARG
    torch.cuda.synchronize()


def test_verbose_lstm_outside_the_limits_falls_back(monkeypatch):
    from bcnf_amd import feature_network as F
    torch.manual_seed(6)
    net = F.VerboseLSTM(3, 20, 2, bidirectional=True).to(DEV)
    monkeypatch.setattr(F._LSTMLayerFn, "apply", lambda *a: pytest.fail("H = 20 must not reach the kernels"))
    against_float64_copy(net, torch.randn(4, 30, 3, device=DEV), "H=20")


# ------------------------------------------------------------------------------------------ module, fused vs torch
@pytest.mark.parametrize("args,kwargs,B,S", [((3, 128, 4), dict(dropout=0.5, bidirectional=True), 9, 30),
                                             ((6, 16, 1), dict(bidirectional=False), 5, 16)],
                         ids=["H128x4-bidirectional", "H16x1"])
def test_module_fused_equals_torch_ops_in_eval_mode(args, kwargs, B, S):
    """VerboseLSTM with the kernels on and forced off (fused = False, the nn.LSTM modules): the same values, h and
    gradients, in EVAL mode -- the fused backward needs no training mode."""
    from bcnf_amd.feature_network import VerboseLSTM
    torch.manual_seed(7)
    net = VerboseLSTM(*args, **kwargs).to(DEV).eval()
    res = []
    for fused in (True, False):
        net.fused = fused
        net.zero_grad()
        x = torch.randn(B, S, args[0], device=DEV, generator=torch.Generator(DEV).manual_seed(1)).requires_grad_(True)
        if fused:
            y, h = net(x)
            (y * y).sum().backward()
        else:
            net.train()                  # torch's GPU LSTM refuses a backward in eval mode; no dropout runs here:
            for m in net.lstm:           # the Dropout modules stay in eval mode
                if isinstance(m, nn.Dropout):
                    m.eval()
            y, h = net(x)
            (y * y).sum().backward()
            net.eval()
        assert h.shape == (B, args[2], S, y.shape[-1])
        res.append([y.detach().cpu(), h.detach().cpu(), x.grad.cpu()] + [p.grad.cpu() for p in net.parameters()])
    del net.fused
    for a, b in zip(res[0][:2], res[1][:2]):
        ok, err = close(a, b)
        assert ok, err
    assert len(res[0]) == 3 + len(list(net.parameters()))
    for a, b in zip(res[0][2:], res[1][2:]):
        ok, err = close(a, b, rtol=1e-4, floor=1e-4)
        assert ok, err


# ------------------------------------------------------------------------------------------ networks vs the fixture
@pytest.mark.parametrize("name", ["l1", "l2", "l2x5", "l3"])
def test_networks_match_the_reference(name):
    g = golden(name)
    net = build(name[:2])
    net.load_state_dict(golden_sd(g, f"{name[:2]}/sd/"))
    net.to(DEV).eval()
    h = net(t(g[f"{name}/traj"]))
    ok, err = close(h.detach().cpu(), g[f"{name}/h"])
    assert ok, err
    (h * t(g[f"{name[:2]}/w"])).sum().backward()
    n = 0
    for pname, p in net.named_parameters():
        ok, err = close(p.grad.cpu(), g[f"{name}/grad/{pname}"], rtol=1e-4, floor=1e-4)
        assert ok, (pname, err)
        n += 1
    assert n == sum(k.startswith(f"{name}/grad/") for k in g.keys())


def test_network_runs_on_the_kernels(monkeypatch):
    """The fused path is the one taken: l2 (two layers, both domains) calls the layer Function four times; with
    `fused` off it is not touched and the values agree."""
    from bcnf_amd import feature_network as F
    g = golden("l2")
    net = build("l2").to(DEV).eval()
    x = t(g["l2/traj"])
    calls = []
    orig = F._LSTMLayerFn.apply
    monkeypatch.setattr(F._LSTMLayerFn, "apply", lambda *a: (calls.append(1), orig(*a))[1])
    with torch.no_grad():
        h1 = net(x)
        assert len(calls) == 4
        calls.clear()
        monkeypatch.setattr(F.VerboseLSTM, "fused", False)
        h0 = net(x)
    assert not calls
    ok, err = close(h1.cpu(), h0.cpu())
    assert ok, err


def full_model(train=False, **model_kwargs):
    from bcnf_amd import CondRealNVP_v2
    cfg = copy.deepcopy(MODEL_CFG)
    cfg["model"]["kwargs"].update(model_kwargs)
    torch.manual_seed(0)
    m = CondRealNVP_v2.from_config(cfg)
    m.load_state_dict(golden_sd(golden("m"), "m/sd/"))
    return m.to(DEV).train(train)


def check_grads(named, g):
    n = 0
    for pname, grad in named.items():
        ok, err = close(grad.cpu(), g[f"m/grad/{pname}"], rtol=1e-4, floor=1e-4)
        assert ok, (pname, err)
        n += 1
    return n


def test_full_model_matches_the_reference_unfolded():
    from bcnf_amd import inn_nll_loss
    g = golden("m")
    m = full_model()
    y, traj = t(g["m/y"]), t(g["m/traj"])
    z, h = m(y, traj, log_det_J=True, return_features=True)
    for got, key in ((h, "m/h"), (z, "m/z"), (m.log_det_J, "m/ldj")):
        ok, err = close(got.detach().cpu(), g[key])
        assert ok, (key, err)
    nll = inn_nll_loss(z, m.log_det_J)
    assert abs(nll.item() - float(g["m/nll"])) <= 1e-5 * abs(float(g["m/nll"])) + 1e-5
    nll.backward()
    grads = {n: p.grad for n, p in m.named_parameters() if p.requires_grad}
    assert check_grads(grads, g) == sum(k.startswith("m/grad/") for k in g.keys())
    with torch.no_grad():
        inv = m.inverse(t(g["m/z"]), traj)
    ok, err = close(inv.cpu(), g["m/inv"])
    assert ok, ("inverse", err)


def nll_grads(m, y, traj, fold):
    m.fold_features = fold
    m.zero_grad(set_to_none=True)
    vals = m.nll_loss(y, traj)
    torch.autograd.backward(vals, torch.tensor([1.0, 0.0, 0.0], device=DEV))
    return vals.detach().cpu(), {n: p.grad.clone() for n, p in m.named_parameters() if p.grad is not None}


def test_full_model_folded_fc_linear():
    """nll_loss folds the last (here the only) Linear of `fc` into the condition projection: the fixture's NLL and
    gradients, and the folded launch against the unfolded one."""
    g = golden("m")
    m = full_model()
    y, traj = t(g["m/y"]), t(g["m/traj"])
    fn = m.feature_network_stack.feature_networks[1]
    fold = m._wide_fold(y, (traj,))
    assert fold is not None and fold[1] is fn.fc.nn[-1]
    assert fold[0].shape == (12, 2 * 32 * 2)
    m.fold_features = False
    assert m._wide_fold(y, (traj,)) is None
    vf, gf = nll_grads(m, y, traj, True)
    vu, gu = nll_grads(m, y, traj, False)
    ref = float(g["m/nll"])
    assert abs(vf[0].item() - ref) <= 1e-5 * abs(ref) + 1e-5 and vf[0].item() == vf[1].item()
    ok, err = close(vf, vu, rtol=1e-5, floor=1e-5)
    assert ok, ("vals", err)
    assert set(gf) == set(gu)
    assert check_grads(gf, g) == sum(k.startswith("m/grad/") for k in g.keys())
    for name in gf:
        ok, err = close(gf[name].cpu(), gu[name].cpu(), rtol=1e-4, floor=1e-4)
        assert ok, (name, err)


# ------------------------------------------------------------------------------------------ TrainStep, sample
def test_trainstep_graph_equals_eager_steps():
    """All dropouts 0: three captured-and-replayed steps equal three eager steps on a deep copy, bit for bit."""
    from bcnf_amd import CondRealNVP_v2
    from bcnf_amd.train import TrainStep
    g = golden("m")
    cfg = copy.deepcopy(MODEL_CFG)
    cfg["model"]["kwargs"].update(dropout=0.0)
    cfg["feature_networks"][1]["kwargs"].update(dropout=0.0, fc_dropout=0.0)
    torch.manual_seed(11)
    m1 = CondRealNVP_v2.from_config(cfg).to(DEV).train()
    m2 = copy.deepcopy(m1)
    s1 = TrainStep(m1, lr=2e-4, capture=True)
    s2 = TrainStep(m2, lr=2e-4, capture=False)
    y, traj = t(g["m/y"]), t(g["m/traj"])
    before = [p.detach().clone() for p in m1.parameters()]
    for _ in range(3):
        v1 = s1.step(y, traj)
        v2 = s2.step(y, traj)                                          # capture=False: eager_step
        assert v1 == v2 and all(math.isfinite(v) for v in v1)
    torch.cuda.synchronize()
    for (n1, p1), (n2, p2), p0 in zip(m1.named_parameters(), m2.named_parameters(), before):
        assert n1 == n2 and torch.equal(p1, p2), n1
        assert not p1.requires_grad or not torch.equal(p1, p0), n1        # every trainable tensor was updated
    fn = m2.feature_network_stack.feature_networks[1]
    assert fn.frequency_lstm.lstm[1].weight_hh_l0_reverse.grad is not None


def finite_step(cfg, B, **kw):
    from bcnf_amd import CondRealNVP_v2
    from bcnf_amd.train import TrainStep
    torch.manual_seed(13)
    m = CondRealNVP_v2.from_config(cfg).to(DEV).train()
    gen = torch.Generator().manual_seed(5)
    y, traj = torch.randn(B, 21, generator=gen).to(DEV), torch.randn(B, 30, 3, generator=gen).to(DEV)
    vals = TrainStep(m, lr=2e-4, capture=False, **kw).step(y, traj)
    torch.cuda.synchronize()
    assert all(math.isfinite(v) for v in vals), vals
    # the optimizer's view: ONE flat leaf for the coupling stack, then the feature network's (and head's) tensors
    for i, p in enumerate(m.flat_parameters()):
        assert p.grad is not None and bool(torch.isfinite(p.grad).all()), i
    assert float(m.fused.flat_param.grad.abs().max()) > 0.0
    for name, p in m.feature_network_stack.named_parameters():
        assert p.grad is not None and float(p.grad.abs().max()) > 0.0, name
    return vals


def test_trainstep_of_the_large_shape():
    """t_DLSTM_large as shipped (H = 128, 4 bidirectional layers, [512] * 4, 32 blocks), one eager step at B = 16:
    66 feature tensors, so TrainStep packs them."""
    vals = finite_step(dlstm_cfg([512] * 4, 32, 128, 4), 16)
    assert vals[0] == vals[1]


def test_hybrid_step_of_the_xsmall_shape():
    vals = finite_step(dlstm_cfg([32] * 5, 32, 16, 1, hybrid=True), 16, hybrid_weight=1.0)
    assert vals[2] > 0.0


def test_sample_with_log_prob():
    from bcnf_amd import CondRealNVP_v2
    torch.manual_seed(2)
    m = CondRealNVP_v2.from_config(dlstm_cfg([32] * 5, 32, 16, 1)).to(DEV).eval()
    traj = torch.randn(5, 30, 3, device=DEV)
    torch.manual_seed(21)
    draws, lp = m.sample(7, traj, outer=True, return_log_prob=True)
    assert draws.shape == (7, 5, 21) and lp.shape == (7, 5)
    with torch.no_grad():
        ref = torch.stack([m.log_prob(draws[i].to(DEV), traj) for i in range(7)]).cpu()
    ok, err = close(lp, ref)
    assert ok, err
