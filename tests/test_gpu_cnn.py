"""GPU tests of the CNN feature network on the fused convolution-block kernels of bcnf_conv.hip: the kernels alone
against the float64 torch chain (tests/cnn_ref.py; the kernel's own winners validated, then used for the float64
gradients), the refused shapes and the fallback, the module against its torch-op form, the networks and a full model
against the reference's fixture (tests/golden/g18_cnn*.npz), one training-mode pass against float64 with the restated
masks, TrainStep (captured against eager), a [ConcatenateCondition, CNN, LSTM] step, a trailing camera-parameter
condition, and sample() with its log-density. Values are held to close(1e-5, 1e-5), gradients to close(1e-4, 1e-4)
(tests/conftest.py).

CONV_CASES reaches every arm of CONV_K_DISPATCH (K = 1 ... 8, three kernels each) and every branch of wgrad_plan,
k_conv_wgrad's chunk / band / image loops and k_conv_tile's tile x round loop that tests/feature_plans.py registers;
tests/test_feature_plans_cpu.py enforces both on the CPU, so a case taken out of the list fails there."""
import copy
import math

import pytest
import torch

from cnn_ref import block_f64, conv_keep, near_tie_census, validate_code, windows
from conftest import close
from gpu_guard import DEV, canaries_alive1, guarded1

pytestmark = pytest.mark.gpu

SEED, OFFSET, SALT = 0x1234_5678_9ABC_DEF0 & ((1 << 62) - 1), (3 << 32) + 11, 260
BYTE_CANARY = 0xA5
NEAR_TIE_CAP = 1e-3


def t(a):
    return torch.from_numpy(a).to(DEV)


# (N, c_in, H, W, c_out, K, pad_h, pad_w)
CONV_CASES = [(1, 1, 2, 2, 1, 1, 0, 0),          # a single window
              (3, 1, 26, 40, 8, 8, 3, 3),        # even K; odd Hc and Wc: the unpooled last row and column
              (2, 8, 12, 19, 16, 5, 3, 3),       # padding > (K - 1) / 2
              (2, 16, 7, 10, 32, 3, 2, 2),       # padding = K - 1
              (5, 5, 9, 11, 10, 3, 1, 1),        # channels that are not powers of two
              (2, 10, 8, 8, 15, 5, 1, 1),        # shrinking output
              (33, 3, 6, 70, 4, 3, 0, 2),        # pad_h != pad_w; many images; a wide row
              (1, 32, 5, 5, 32, 8, 7, 7),        # every limit at once
              (2, 1, 90, 160, 8, 8, 3, 3),       # the real frame size
              # the remaining arms of CONV_K_DISPATCH
              (2, 3, 9, 12, 5, 2, 1, 0),         # K = 2
              (2, 6, 10, 13, 9, 4, 3, 2),        # K = 4
              (2, 7, 11, 9, 12, 6, 5, 2),        # K = 6
              (2, 4, 9, 14, 6, 7, 3, 6),         # K = 7, pad_w = K - 1
              # the branches of wgrad_plan / k_conv_wgrad / k_conv_tile (feature_plans.CONV_BRANCHES has the fields)
              (1025, 1, 4, 5, 3, 2, 0, 1),       # 512 workgroups: workgroup 0 walks three images, the others two
              (1, 32, 8, 160, 32, 3, 1, 1),      # four x chunks of 42, the last ragged (36); two bands, three passes;
                                                 # forward tiles (1 x 5) x 2 rounds
              (1, 32, 8, 50, 32, 5, 2, 2),       # chunk width 25: the window of columns 24, 25 straddles two chunks
              (1, 32, 15, 16, 32, 3, 1, 1),      # band height 7: the window of rows 6, 7 straddles two bands
              (1, 32, 40, 24, 32, 8, 7, 7),      # the GWC > K halving: chunks of 16 = 2 K, 12 bands, 8 passes
              (1, 20, 37, 150, 32, 7, 3, 3)]     # K = 7 at scale: 4 chunks (ragged 28), 9 bands, 5 passes, 5 x 5 tiles
                                                 # x 2 (forward) and 3 (input gradient) rounds


def conv_inputs(case):
    N, ci, H, W, co, K, ph, pw = case
    gen = torch.Generator().manual_seed(1000 * K + 10 * co + N)
    x = torch.randn(N, ci, H, W, generator=gen)
    w = (2.0 * torch.rand(co, ci, K, K, generator=gen) - 1.0) / math.sqrt(ci * K * K)
    b = 0.1 * torch.randn(co, generator=gen)
    hc, wc = H + 2 * ph - K + 1, W + 2 * pw - K + 1
    dy = torch.randn(N, co, hc // 2, wc // 2, generator=gen)
    return x, w, b, dy, (hc, wc)


def conv_reference(case, p):
    """float64 activations of the case (CPU only) and the near-tie census the cap is asserted on."""
    N, ci, H, W, co, K, ph, pw = case
    x, w, b, dy, (hc, wc) = conv_inputs(case)
    keep = torch.from_numpy(conv_keep(p, SEED, OFFSET, SALT, (N, co, hc, wc)))
    x64, w64, b64 = (v.double().requires_grad_(True) for v in (x, w, b))
    scaled, a = block_f64(x64, w64, b64, (ph, pw), p, keep)
    tol = 1e-5 * max(float(a.detach().abs().max()), 1e-30)
    positive, near = near_tie_census(a, tol)
    return dict(x=x, w=w, b=b, dy=dy, x64=x64, w64=w64, b64=b64, scaled=scaled, a=a, tol=tol, positive=positive,
                near=near)


def byte_guarded(n):
    buf = torch.full((n + 128,), BYTE_CANARY, dtype=torch.uint8, device=DEV)
    return buf, buf[64:64 + n]


def byte_canaries_alive(buf, n):
    return bool((buf[:64] == BYTE_CANARY).all()) and bool((buf[64 + n:] == BYTE_CANARY).all())


@pytest.mark.parametrize("p", [0.0, 0.5])
@pytest.mark.parametrize("case", CONV_CASES, ids=lambda c: "x".join(map(str, c)))
def test_conv_kernels_against_float64(case, p):
    from bcnf_amd import _native as N
    n_img, ci, H, W, co, K, ph, pw = case
    R = conv_reference(case, p)
    # before the GPU is touched: near-tie windows are rare enough that the validated winners decide nothing else
    assert R["near"] <= NEAR_TIE_CAP * max(R["positive"], 1), (R["near"], R["positive"])
    shape = R["dy"].shape
    ny = R["dy"].numel()
    st = N.stream_handle(torch.device(DEV, torch.cuda.current_device()))
    rng = torch.tensor([SEED, OFFSET], dtype=torch.int64, device=DEV)
    args = (n_img, ci, H, W, co, K, ph, pw)
    wbytes = N.query_i64("bcnf_conv_block_work_bytes", *args, p)
    assert wbytes > 0 and wbytes % 4 == 0
    xb, xv = guarded1(R["x"].numel(), R["x"].reshape(-1))
    wb, wv = guarded1(R["w"].numel(), R["w"].reshape(-1))
    bb, bv = guarded1(co, R["b"])
    db_, dyv = guarded1(ny, R["dy"].reshape(-1))
    runs = []
    for _ in range(2):
        yb, yv = guarded1(ny)
        cb, cv = byte_guarded(ny)
        dxb, dxv = guarded1(R["x"].numel())
        dwb, dwv = guarded1(R["w"].numel())
        dbb, dbv = guarded1(co)
        kb, kv = guarded1(wbytes // 4)
        N.call("bcnf_conv_block_forward", xv, wv, bv, *args, p, rng, SALT, yv, cv, st)
        N.call("bcnf_conv_block_backward", xv, wv, dyv, cv, *args, p, dxv, dwv, dbv, kv, st)
        torch.cuda.synchronize()
        assert canaries_alive1(yb, ny) and byte_canaries_alive(cb, ny), "forward canary"
        assert canaries_alive1(dxb, R["x"].numel()) and canaries_alive1(dwb, R["w"].numel()), "dx / dw canary"
        assert canaries_alive1(dbb, co) and canaries_alive1(kb, wbytes // 4, written=False), "db / work canary"
        for buf, n in ((xb, R["x"].numel()), (wb, R["w"].numel()), (bb, co), (db_, ny)):
            assert canaries_alive1(buf, n)
        runs.append([yv.clone(), cv.clone(), dxv.clone(), dwv.clone(), dbv.clone()])
    for a, c in zip(*runs):
        assert torch.equal(a, c)                                         # fixed-order sums: the same bits
    yv, cv, dxv, dwv, dbv = (v.cpu() for v in runs[0])
    m64 = windows(R["a"].detach()).max(dim=-1).values
    ok, err = close(yv.view(shape), m64)
    print(f"y err={err:.3e}")
    assert ok, ("y", err)
    win, alive = validate_code(cv.view(shape), R["a"], R["tol"])
    # float64 gradients along the kernel's own (validated) winners
    sel = windows(R["scaled"]).gather(-1, win.unsqueeze(-1)).squeeze(-1) * alive
    (sel * R["dy"].double()).sum().backward()
    for name, got, ref in (("dx", dxv.view(R["x"].shape), R["x64"].grad), ("dw", dwv.view(R["w"].shape), R["w64"].grad),
                           ("db", dbv, R["b64"].grad)):
        ok, err = close(got, ref, rtol=1e-4, floor=1e-4)
        print(f"{name} err={err:.3e}")
        assert ok, (name, err)
    # (an odd last row or column of the convolution output is in no window of `sel`: its float64 gradient is zero)

    # inference (code = NULL) gives the same y; dx = NULL leaves the parameter gradients alone
    yb, y2 = guarded1(ny)
    N.call("bcnf_conv_block_forward", xv, wv, bv, *args, p, rng, SALT, y2, None, st)
    dwb, dw2 = guarded1(R["w"].numel())
    dbb, db2 = guarded1(co)
    kb, kv = guarded1(wbytes // 4)
    N.call("bcnf_conv_block_backward", xv, wv, dyv, runs[0][1], *args, p, None, dw2, db2, kv, st)
    torch.cuda.synchronize()
    assert canaries_alive1(yb, ny) and canaries_alive1(dwb, R["w"].numel()) and canaries_alive1(dbb, co)
    assert torch.equal(y2.cpu(), yv) and torch.equal(dw2.cpu(), dwv) and torch.equal(db2.cpu(), dbv)


# ------------------------------------------------------------------------------------------ refused shapes
#                          N  ci  H   W  co  K  ph pw  p
@pytest.mark.parametrize("args", [(2, 1, 12, 12, 4, 9, 3, 3, 0.0),       # K = 9
                                  (2, 33, 12, 12, 4, 3, 1, 1, 0.0),      # c_in = 33
                                  (2, 4, 12, 12, 33, 3, 1, 1, 0.0),      # c_out = 33
                                  (2, 4, 12, 12, 4, 3, 3, 1, 0.0),       # pad_h = K
                                  (2, 4, 12, 12, 4, 3, 1, 3, 0.0),       # pad_w = K
                                  (2, 4, 3, 12, 4, 3, 0, 1, 0.0),        # Hc = 1
                                  (2, 4, 12, 3, 4, 3, 1, 0, 0.0),        # Wc = 1
                                  (2, 4, 12, 12, 4, 3, 1, 1, 1.0),       # p = 1
                                  (0, 4, 12, 12, 4, 3, 1, 1, 0.0)],      # no image
                         ids=["K9", "cin33", "cout33", "padh", "padw", "Hc1", "Wc1", "p1", "N0"])
def test_shapes_outside_the_limits_are_refused(args):
    from bcnf_amd import _native as N
    buf = torch.zeros(1 << 16, device=DEV)
    code = torch.zeros(1 << 16, dtype=torch.uint8, device=DEV)
    rng = torch.tensor([1, 2], dtype=torch.int64, device=DEV)
    st = N.stream_handle(buf.device)
    shape, p = args[:8], args[8]
    assert N.call_raw("bcnf_conv_block_forward", buf, buf, buf, *shape, p, rng, 0, buf, code, st) == N.ERR_ARG
    assert N.query_status("bcnf_conv_block_work_bytes", *shape, p)[0] == N.ERR_ARG
    assert N.call_raw("bcnf_conv_block_backward", buf, buf, buf, code, *shape, p, buf, buf, buf, buf, st) == N.ERR_ARG
    torch.cuda.synchronize()
    assert float(buf.abs().max()) == 0.0                                 # nothing was launched


def against_float64_copy(net, x, what):
    """values and every gradient (input included) of net on the GPU against its float64 CPU copy."""
    ref = copy.deepcopy(net).double().cpu()
    xg = x.clone().requires_grad_(True)
    y = net(xg)
    w = torch.randn(y.shape, generator=torch.Generator().manual_seed(9))
    (y * w.to(DEV)).sum().backward()
    xr = x.detach().double().cpu().requires_grad_(True)
    yr = ref(xr)
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


def test_cnn_outside_the_limits_falls_back(monkeypatch):
    from bcnf_amd import CNN, cnn
    torch.manual_seed(6)
    net = CNN([4, 6], [3, 3], [2, 1], 8, 8, [26, 40], dropout_prob=0.0).to(DEV).eval()
    monkeypatch.setattr(cnn._ConvBlockFn, "apply", lambda *a: pytest.fail("stride 2 must not reach the kernels"))
    against_float64_copy(net, torch.randn(2, 2, 3, 26, 40, device=DEV), "stride 2")


# ------------------------------------------------------------------------------------------ module, fused vs torch
@pytest.mark.parametrize("name", ["c1", "c2"])
def test_module_fused_equals_torch_ops_in_eval_mode(name):
    from test_cnn_cpu import build
    torch.manual_seed(7)
    net = build(name).to(DEV).eval()
    res = []
    for fused in (True, False):
        net.fused = fused
        net.zero_grad()
        x = torch.randn(3, 2, 4, 26, 40, device=DEV, generator=torch.Generator(DEV).manual_seed(1)).requires_grad_(True)
        y = net(x)
        (y * y).sum().backward()
        res.append([y.detach().cpu(), x.grad.cpu()] + [p.grad.cpu() for p in net.parameters()])
    del net.fused
    ok, err = close(res[0][0], res[1][0])
    assert ok, err
    assert len(res[0]) == 2 + len(list(net.parameters()))
    for a, b in zip(res[0][1:], res[1][1:]):
        ok, err = close(a, b, rtol=1e-4, floor=1e-4)
        assert ok, err


# ------------------------------------------------------------------------------------------ networks vs the fixture
@pytest.mark.parametrize("name,launches", [("c1", 3), ("c2", 6)])
def test_networks_match_the_reference_on_the_kernels(name, launches, monkeypatch):
    from bcnf_amd import cnn
    from test_cnn_cpu import golden, grads_of, loaded
    g = golden(name)
    net = loaded(name).to(DEV).eval()
    calls = []
    orig = cnn._ConvBlockFn.apply
    monkeypatch.setattr(cnn._ConvBlockFn, "apply", lambda *a: (calls.append(1), orig(*a))[1])
    h = net(t(g["videos"]))
    assert len(calls) == launches                                        # the kernels ran, not the torch modules
    ok, err = close(h.detach().cpu(), g[f"{name}/h"])
    assert ok, err
    (h * t(g[f"{name}/w"])).sum().backward()
    ref = grads_of(name)
    n = 0
    for pname, p in net.named_parameters():
        ok, err = close(p.grad.cpu(), ref[pname], rtol=1e-4, floor=1e-4)
        assert ok, (pname, err)
        n += 1
    assert n == len(ref)
    calls.clear()
    monkeypatch.setattr(cnn.CNN, "fused", False)
    with torch.no_grad():
        h0 = net(t(g["videos"]))
    assert not calls
    ok, err = close(h.detach().cpu(), h0.cpu())
    assert ok, err


def full_model(train=False):
    from test_cnn_cpu import loaded
    return loaded("m").to(DEV).train(train)


def test_full_model_matches_the_reference():
    from bcnf_amd import inn_nll_loss
    from test_cnn_cpu import golden
    g = golden("m")
    m = full_model()
    y, videos = t(g["m/y"]), t(golden("c1")["videos"])
    z, h = m(y, videos, log_det_J=True, return_features=True)
    for got, key in ((h, "m/h"), (z, "m/z"), (m.log_det_J, "m/ldj")):
        ok, err = close(got.detach().cpu(), g[key])
        assert ok, (key, err)
    nll = inn_nll_loss(z, m.log_det_J)
    assert abs(nll.item() - float(g["m/nll"])) <= 1e-5 * abs(float(g["m/nll"])) + 1e-5
    nll.backward()
    n = 0
    for pname, p in m.named_parameters():
        if not p.requires_grad:
            continue
        ok, err = close(p.grad.cpu(), g[f"m/grad/{pname}"], rtol=1e-4, floor=1e-4)
        assert ok, (pname, err)
        n += 1
    assert n == sum(k.startswith("m/grad/") for k in g.keys())
    with torch.no_grad():
        inv = m.inverse(t(g["m/z"]), videos)
    ok, err = close(inv.cpu(), g["m/inv"])
    assert ok, ("inverse", err)
    # nll_loss folds the FullyConnected's only Linear into the condition projection: the same NLL
    vals = m.nll_loss(y, videos)
    assert abs(vals[0].item() - float(g["m/nll"])) <= 1e-5 * abs(float(g["m/nll"])) + 1e-5


# ------------------------------------------------------------------------------------------ training mode
def test_training_mode_against_float64_with_the_restated_masks(monkeypatch):
    """One training-mode forward + backward of c1 on its own Philox state against float64 with the kernels' masks
    restated on the host (salt = the Conv2d's module index; images in the input's (batch, camera, frame) order). The
    three launches' code tensors are picked up on their way into the library and validated against the float64
    activations as in the kernel test; the float64 chain then pools along those winners. The offset advances by
    one."""
    from bcnf_amd import _native as N
    from test_cnn_cpu import build
    torch.manual_seed(31)
    net = build("c1").to(DEV).train()
    p = net.cnn_layers[0][2].p
    gen = torch.Generator().manual_seed(3)
    x = torch.randn(3, 2, 4, 26, 40, generator=gen)
    w = torch.randn(3, 4, 24, generator=gen)
    seed, offset = (int(v) for v in net.rng_state(torch.device(DEV, torch.cuda.current_device())).tolist())
    launches = []
    orig = N.call

    def spy(name, *args):
        if name == "bcnf_conv_block_forward":
            launches.append(args)
        return orig(name, *args)
    monkeypatch.setattr(N, "call", spy)
    xg = x.to(DEV).requires_grad_(True)
    h = net(xg)
    (h * w.to(DEV)).sum().backward()
    monkeypatch.undo()
    assert net.rng_state(xg.device).tolist() == [seed, offset + 1]
    assert [a[13] for a in launches] == [0, 4, 8] and all(a[11] == p for a in launches)     # a salt per layer
    # float64 on the host, along the kernels' validated winners
    ref = copy.deepcopy(net).double().cpu()
    xr = x.double().requires_grad_(True)
    a = xr.reshape(-1, 1, 26, 40)
    positive = near = 0
    for i, launch in zip((0, 4, 8), launches):
        conv = ref.cnn_layers[0][i]
        code = launch[15].cpu()
        hc, wc = (a.shape[d] + 2 * conv.padding[d - 2] - conv.kernel_size[d - 2] + 1 for d in (2, 3))
        keep = torch.from_numpy(conv_keep(p, seed, offset, i, (a.shape[0], conv.out_channels, hc, wc)))
        scaled, act = block_f64(a, conv.weight, conv.bias, conv.padding, p, keep)
        tol = 1e-5 * float(act.detach().abs().max())
        census = near_tie_census(act, tol)
        positive, near = positive + census[0], near + census[1]
        win, alive = validate_code(code, act, tol)
        a = windows(scaled).gather(-1, win.unsqueeze(-1)).squeeze(-1) * alive
    assert near <= NEAR_TIE_CAP * positive, (near, positive)
    feats = a.flatten(1).view(3, 2, 4, -1)
    hr = ref.final_layer(feats.reshape(3, 4, -1))
    (hr * w.double()).sum().backward()
    ok, err = close(h.detach().cpu(), hr.detach())
    assert ok, ("h", err)
    ok, err = close(xg.grad.cpu(), xr.grad, rtol=1e-4, floor=1e-4)
    assert ok, ("dx", err)
    refp = dict(ref.named_parameters())
    for name, prm in net.named_parameters():
        ok, err = close(prm.grad.cpu(), refp[name].grad, rtol=1e-4, floor=1e-4)
        assert ok, (name, err)
    # the next forward draws other masks
    with torch.no_grad():
        assert not torch.equal(net(xg), h)


# ------------------------------------------------------------------------------------------ TrainStep, sample
def test_trainstep_graph_equals_eager_steps():
    """All dropouts 0: three captured-and-replayed steps equal three eager steps on a deep copy, bit for bit."""
    from bcnf_amd import CondRealNVP_v2
    from bcnf_amd.train import TrainStep
    from test_cnn_cpu import MODEL_CFG, golden
    g = golden("m")
    cfg = copy.deepcopy(MODEL_CFG)
    cfg["model"]["kwargs"].update(dropout=0.0)
    cfg["feature_networks"][1]["kwargs"].update(dropout_prob=0.0)
    torch.manual_seed(11)
    m1 = CondRealNVP_v2.from_config(cfg).to(DEV).train()
    m2 = copy.deepcopy(m1)
    s1 = TrainStep(m1, lr=2e-4, capture=True)
    s2 = TrainStep(m2, lr=2e-4, capture=False)
    y, videos = t(g["m/y"]), t(golden("c1")["videos"])
    before = [p.detach().clone() for p in m1.parameters()]
    for _ in range(3):
        v1 = s1.step(y, videos)
        v2 = s2.step(y, videos)                                        # capture=False: eager_step
        assert v1 == v2 and all(math.isfinite(v) for v in v1)
    torch.cuda.synchronize()
    for (n1, p1), (n2, p2), p0 in zip(m1.named_parameters(), m2.named_parameters(), before):
        assert n1 == n2 and torch.equal(p1, p2), n1
        assert not p1.requires_grad or not torch.equal(p1, p0), n1        # every trainable tensor was updated


def test_trainstep_of_cnn_and_lstm():
    """[ConcatenateCondition, CNN c1, LSTM(pool_dim=1)], training mode with the CNN's and the flow's dropout on: one
    finite eager step; every feature gradient is non-zero."""
    from bcnf_amd import CondRealNVP_v2
    from bcnf_amd.train import TrainStep
    from test_cnn_cpu import CNN_LSTM_CFG
    torch.manual_seed(13)
    m = CondRealNVP_v2.from_config(CNN_LSTM_CFG).to(DEV).train()
    gen = torch.Generator().manual_seed(5)
    y, videos = torch.randn(4, 21, generator=gen).to(DEV), torch.randn(4, 2, 4, 26, 40, generator=gen).to(DEV)
    vals = TrainStep(m, lr=2e-4, capture=False).step(y, videos)
    torch.cuda.synchronize()
    assert all(math.isfinite(v) for v in vals), vals
    for i, p in enumerate(m.flat_parameters()):
        assert p.grad is not None and bool(torch.isfinite(p.grad).all()), i
    for name, p in m.feature_network_stack.named_parameters():
        assert p.grad is not None and float(p.grad.abs().max()) > 0.0, name


def test_nll_loss_with_a_trailing_camera_condition():
    """videos_CNN_LSTM_large's tail: a ConcatenateCondition(dim=-1) appends 7 camera values to the LSTM's output;
    nll_loss takes both conditions, is finite and reaches the first convolution's weight."""
    from bcnf_amd import CondRealNVP_v2
    from test_cnn_cpu import CNN_LSTM_CFG
    cfg = copy.deepcopy(CNN_LSTM_CFG)
    cfg["model"]["kwargs"]["n_conditions"] = 23
    cfg["feature_networks"].append({"type": "ConcatenateCondition",
                                    "kwargs": {"input_size": 16, "output_size": 23, "dim": -1}})
    torch.manual_seed(14)
    m = CondRealNVP_v2.from_config(cfg).to(DEV).train()
    gen = torch.Generator().manual_seed(6)
    y, videos = torch.randn(4, 21, generator=gen).to(DEV), torch.randn(4, 2, 4, 26, 40, generator=gen).to(DEV)
    cams = torch.randn(4, 7, generator=gen).to(DEV)
    vals = m.nll_loss(y, videos, cams)
    torch.autograd.backward(vals, torch.tensor([1.0, 0.0, 0.0], device=DEV))
    assert bool(torch.isfinite(vals).all())
    g0 = m.feature_network_stack.feature_networks[1].cnn_layers[0][0].weight.grad
    assert g0 is not None and bool(torch.isfinite(g0).all()) and float(g0.abs().max()) > 0.0


def test_sample_with_log_prob():
    from bcnf_amd import CondRealNVP_v2
    from test_cnn_cpu import CNN_LSTM_CFG
    torch.manual_seed(2)
    m = CondRealNVP_v2.from_config(CNN_LSTM_CFG).to(DEV).eval()
    videos = torch.randn(5, 2, 4, 26, 40, device=DEV)
    torch.manual_seed(21)
    draws, lp = m.sample(7, videos, outer=True, return_log_prob=True)
    assert draws.shape == (7, 5, 21) and lp.shape == (7, 5)
    with torch.no_grad():
        ref = torch.stack([m.log_prob(draws[i].to(DEV), videos) for i in range(7)]).cpu()
    ok, err = close(lp, ref)
    assert ok, err
