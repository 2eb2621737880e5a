"""GPU tests of the Transformer feature networks on the fused kernels of bcnf_attn.hip: the attention core
(bcnf_attn_forward / bcnf_attn_backward) and residual + LayerNorm (bcnf_add_layernorm_*) alone against float64 torch
restatements, the networks and a full model against the reference's fixture (tests/golden/g16_transformer.npz), the
folded `output` Linear against the unfolded path, graph-captured TrainStep against eager steps, and sample() with its
log-density. Values are held to close(1e-5, 1e-5), gradients to close(1e-4, 1e-4) (tests/conftest.py).

ATTN_CASES reaches all 2 x 4 arms of ATTN_DISPATCH, and LN_D x LN_ROWS with LN_CAP_CASES all five arms of LN_DISPATCH
and the LN_MAX_WG cap of ln_plan; tests/test_feature_plans_cpu.py enforces it on the CPU against the restatement in
tests/feature_plans.py, so a case taken out of a list fails there."""
import copy
import math

import pytest
import torch

from conftest import close, golden_sd, load_golden
from gpu_guard import DEV, canaries_alive, guarded
from test_transformer_cpu import MODEL_CFG, T1, build

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def g16():
    return load_golden("g16_transformer.npz")


def t(a):
    return torch.from_numpy(a).to(DEV)


# ------------------------------------------------------------------------------------------ attention core
def attn_f64(q, k, v, heads):
    B, S, d = q.shape
    hd = d // heads
    qh, kh, vh = (x.view(B, S, heads, hd).transpose(1, 2) for x in (q, k, v))
    p = torch.softmax(qh @ kh.transpose(-2, -1) / math.sqrt(hd), dim=-1)
    return (p @ vh).transpose(1, 2).reshape(B, S, d)


ATTN_CASES = [(3, 30, 4, 8), (2, 16, 8, 21), (2, 30, 4, 25), (2, 30, 8, 32), (1, 1, 1, 4),
              (3, 30, 1, 16),        # three (sample, head) pairs leave a workgroup partly empty
              (2, 33, 2, 6),         # first S past the two-heads-per-wave form
              (1, 64, 2, 64),        # both limits
              # the remaining arms of ATTN_DISPATCH and the edges of its buckets
              (2, 30, 2, 33),        # <32,64> at its first head_dim
              (2, 32, 3, 9),         # the last S of the two-slot form; the first head_dim past 8
              (1, 40, 3, 17),        # <64,32>
              (1, 64, 1, 16),        # <64,16> at its upper edge
              (5, 2, 1, 1)]          # head_dim 1


@pytest.mark.parametrize("B,S,heads,hd", ATTN_CASES)
def test_attention_core_against_float64(B, S, heads, hd):
    from bcnf_amd import _native as N
    d, rows = heads * hd, B * S
    gen = torch.Generator().manual_seed(1000 * S + hd)
    q, k, v, dout = (torch.randn(B, S, d, generator=gen, dtype=torch.float64) for _ in range(4))
    q, k = 1.5 * q, 1.5 * k
    q, k, v, dout = (x.float().double() for x in (q, k, v, dout))       # the fp32 values the kernel sees
    qr, kr, vr = (x.clone().requires_grad_(True) for x in (q, k, v))
    out_ref = attn_f64(qr, kr, vr, heads)
    out_ref.backward(dout)
    st = N.stream_handle(torch.device(DEV, torch.cuda.current_device()))
    for ld in (d, d + 5):
        ins = [guarded(rows, d, ld, x.view(rows, d).float().to(DEV))[1] for x in (q, k, v, dout)]
        runs = []
        for _ in range(2):
            (ob, ov), (qb, qv), (kb, kv), (vb, vv) = (guarded(rows, d, ld) for _ in range(4))
            lb, lv = guarded(B * heads, S)
            N.call("bcnf_attn_forward", ins[0], ins[1], ins[2], B, S, heads, hd, ld, ov, lv, st)
            N.call("bcnf_attn_backward", ins[0], ins[1], ins[2], ov, lv, ins[3], B, S, heads, hd, ld, qv, kv, vv, st)
            torch.cuda.synchronize()
            for buf in (ob, qb, kb, vb):
                assert canaries_alive(buf, rows, d, ld), (ld, "canary")
            assert canaries_alive(lb, B * heads, S)
            runs.append([x.clone() for x in (ov, lv, qv, kv, vv)])
        for a, b in zip(*runs):
            assert torch.equal(a, b)                                     # fixed-order sums: the same bits
        ov, lv, qv, kv, vv = runs[0]
        ok, err = close(ov.cpu(), out_ref.detach().view(rows, d))
        assert ok, ("out", ld, err)
        qh = q.view(B, S, heads, hd).transpose(1, 2)
        kh = k.view(B, S, heads, hd).transpose(1, 2)
        lse_ref = torch.logsumexp(qh @ kh.transpose(-2, -1) / math.sqrt(hd), dim=-1)
        ok, err = close(lv.cpu().view(B, heads, S), lse_ref)
        assert ok, ("lse", ld, err)
        for got, ref, what in ((qv, qr.grad, "dq"), (kv, kr.grad, "dk"), (vv, vr.grad, "dv")):
            ok, err = close(got.cpu(), ref.view(rows, d), rtol=1e-4, floor=1e-4)
            assert ok, (what, ld, err)


@pytest.mark.parametrize("S,heads,hd", [(65, 2, 8), (30, 1, 65)])
def test_attention_outside_the_limits_is_refused_and_falls_back(S, heads, hd):
    from bcnf_amd import _native as N
    from bcnf_amd.feature_network import MultiHeadAttention
    B, d = 2, heads * hd
    x = torch.randn(B * S, d, device=DEV)
    out, lse = torch.empty_like(x), torch.empty(B * heads * S, device=DEV)
    st = N.stream_handle(x.device)
    assert N.call_raw("bcnf_attn_forward", x, x, x, B, S, heads, hd, d, out, lse, st) == N.ERR_ARG
    assert N.call_raw("bcnf_attn_backward", x, x, x, out, lse, x, B, S, heads, hd, d, out, out, out, st) == N.ERR_ARG
    low = heads * min(hd, 64) - 1                                        # a row stride below heads * head_dim
    assert N.call_raw("bcnf_attn_forward", x, x, x, B, 30, heads, min(hd, 64), low, out, lse, st) == N.ERR_ARG
    torch.manual_seed(3)
    mha = MultiHeadAttention(d, heads).to(DEV)
    xin = torch.randn(B, S, d, device=DEV, requires_grad=True)
    y = mha(xin, xin, xin)
    y.sum().backward()
    ref = copy.deepcopy(mha).double().cpu()
    xr = xin.detach().double().cpu().requires_grad_(True)
    yr = ref(xr, xr, xr)
    yr.sum().backward()
    ok, err = close(y.detach().cpu(), yr.detach())
    assert ok, err
    ok, err = close(xin.grad.cpu(), xr.grad, rtol=1e-4, floor=1e-4)
    assert ok, err


def test_attention_module_fused_equals_torch_ops():
    """MultiHeadAttention with the kernel on and forced off (fused = False): the same values and gradients."""
    from bcnf_amd.feature_network import MultiHeadAttention
    torch.manual_seed(5)
    mha = MultiHeadAttention(42, 2).to(DEV)                              # head_dim 21
    res = []
    for fused in (True, False):
        mha.fused = fused
        mha.zero_grad()
        x = torch.randn(3, 30, 42, device=DEV, generator=torch.Generator(DEV).manual_seed(1)).requires_grad_(True)
        y = mha(x, x, x)
        (y * y).sum().backward()
        res.append([y.detach().cpu(), x.grad.cpu()] + [p.grad.cpu() for p in mha.parameters()])
    del mha.fused
    ok, err = close(res[0][0], res[1][0])
    assert ok, err
    for a, b in zip(res[0][1:], res[1][1:]):
        ok, err = close(a, b, rtol=1e-4, floor=1e-4)
        assert ok, err


# ------------------------------------------------------------------------------------------ residual + LayerNorm
LN_D = [6, 16, 100, 168, 256, 1024,
        65, 257, 300, 512]           # T = 2 at its first d; T = 8 (257 ... 512) at both ends and inside
LN_ROWS = [1, 63, 257,
           9]                        # two workgroups of five and four rows: a wave with two rows, three with one
LN_CAP_CASES = [(8193, 6), (8193, 100)]      # past LN_MAX_WG workgroups: nine rows each, three for one of the waves
LN_NULLABLE_CASE = (63, 100)


def ln_inputs(rows, d):
    gen = torch.Generator().manual_seed(rows * 2048 + d)
    x = (2.0 * torch.randn(rows, d, generator=gen) + 0.5).float()
    r = torch.randn(rows, d, generator=gen).float()
    gamma = (0.7 + 0.6 * torch.rand(d, generator=gen)).float()
    beta = (0.1 * torch.randn(d, generator=gen)).float()
    dy = torch.randn(rows, d, generator=gen).float()
    return x, r, gamma, beta, dy


@pytest.mark.parametrize("d", LN_D)
@pytest.mark.parametrize("rows", LN_ROWS)
def test_add_layernorm_against_float64(rows, d):
    add_layernorm_against_float64(rows, d)


@pytest.mark.parametrize("rows,d", LN_CAP_CASES)
def test_add_layernorm_past_the_workgroup_cap(rows, d):
    """More than LN_MAX_WG * LN_MIN_RPW = 8192 rows: the backward's workgroups stay at the cap and take nine rows
    each (911 workgroups; tests/feature_plans.py), so a wave sums three rows into its column partials."""
    add_layernorm_against_float64(rows, d)


def add_layernorm_against_float64(rows, d):
    from bcnf_amd import _native as N
    x, r, gamma, beta, dy = ln_inputs(rows, d)
    eps = 1e-5
    xr, rr, gr, br = (a.double().requires_grad_(True) for a in (x, r, gamma, beta))
    yr = torch.nn.functional.layer_norm(xr + rr, (d,), gr, br, eps)
    yr.backward(dy.double())
    assert torch.equal(xr.grad, rr.grad)
    st = N.stream_handle(torch.device(DEV, torch.cuda.current_device()))
    xd, rd, gd, bd, dyd = (a.to(DEV) for a in (x, r, gamma, beta, dy))
    wb = N.query_i64("bcnf_add_layernorm_work_bytes", rows, d)
    runs = []
    for _ in range(2):
        (yb, yv), (dxb, dxv) = guarded(rows, d), guarded(rows, d)
        (mb, mv), (sb, sv) = guarded(1, rows), guarded(1, rows)
        (dgb, dgv), (dbb, dbv) = guarded(1, d), guarded(1, d)
        wbuf, wv = guarded(1, wb // 4)
        N.call("bcnf_add_layernorm_forward", xd, rd, gd, bd, rows, d, eps, yv, mv, sv, st)
        N.call("bcnf_add_layernorm_backward", xd, rd, gd, mv, sv, dyd, rows, d, dxv, dgv, dbv, wv, st)
        torch.cuda.synchronize()
        for buf, shape in ((yb, (rows, d)), (dxb, (rows, d)), (mb, (1, rows)), (sb, (1, rows)), (dgb, (1, d)),
                           (dbb, (1, d)), (wbuf, (1, wb // 4))):
            assert canaries_alive(buf, *shape)
        runs.append([a.clone() for a in (yv, mv, sv, dxv, dgv, dbv)])
    for a, b in zip(*runs):
        assert torch.equal(a, b)
    yv, mv, sv, dxv, dgv, dbv = runs[0]
    z = x.double() + r.double()
    for got, ref, what in ((yv, yr.detach(), "y"), (mv.view(-1), z.mean(-1), "mean"),
                           (sv.view(-1), 1.0 / torch.sqrt(z.var(-1, unbiased=False) + eps), "rstd")):
        ok, err = close(got.cpu(), ref)
        assert ok, (what, err)
    for got, ref, what in ((dxv, xr.grad, "dx"), (dgv.view(-1), gr.grad, "dgamma"), (dbv.view(-1), br.grad, "dbeta")):
        ok, err = close(got.cpu(), ref, rtol=1e-4, floor=1e-4)
        assert ok, (what, err)


def test_add_layernorm_nullable_outputs():
    """What the module passes for frozen parameters and a detached input: beta = NULL on the forward is a zero beta;
    the backward with dx = NULL, with dgamma only and with dbeta only gives the full call's matching outputs bit for
    bit, and its partials stay inside `work`."""
    from bcnf_amd import _native as N
    rows, d = LN_NULLABLE_CASE
    x, r, gamma, beta, dy = ln_inputs(rows, d)
    eps = 1e-5
    st = N.stream_handle(torch.device(DEV, torch.cuda.current_device()))
    xd, rd, gd, bd, dyd = (a.to(DEV) for a in (x, r, gamma, beta, dy))
    wb = N.query_i64("bcnf_add_layernorm_work_bytes", rows, d)

    def forward(b):
        (yb, yv), (mb, mv), (sb, sv) = guarded(rows, d), guarded(1, rows), guarded(1, rows)
        N.call("bcnf_add_layernorm_forward", xd, rd, gd, b, rows, d, eps, yv, mv, sv, st)
        torch.cuda.synchronize()
        assert canaries_alive(yb, rows, d) and canaries_alive(mb, 1, rows) and canaries_alive(sb, 1, rows)
        return yv, mv, sv

    def backward(want_dx, want_dg, want_db):
        outs = [guarded(rows, d) if want_dx else None, guarded(1, d) if want_dg else None,
                guarded(1, d) if want_db else None]
        wbuf, wv = guarded(1, wb // 4)
        N.call("bcnf_add_layernorm_backward", xd, rd, gd, mv, sv, dyd, rows, d,
               *[None if o is None else o[1] for o in outs], wv, st)
        torch.cuda.synchronize()
        for o, shape in zip(outs, ((rows, d), (1, d), (1, d))):
            assert o is None or canaries_alive(o[0], *shape)
        # the guards of `work` hold; inside, the partials are written iff a parameter gradient was asked for
        assert bool(torch.isnan(wbuf[:64]).all()) and bool(torch.isnan(wbuf[64 + wb // 4:]).all())
        assert bool(torch.isfinite(wv).all()) if want_dg or want_db else bool(torch.isnan(wv).all())
        return [None if o is None else o[1] for o in outs]

    yv, mv, sv = forward(bd)
    y0, m0, s0 = forward(None)
    yz, _, _ = forward(torch.zeros(d, device=DEV))
    assert torch.equal(y0, yz) and torch.equal(m0, mv) and torch.equal(s0, sv)
    ok, err = close((yv - y0).cpu(), beta.double().expand(rows, d))
    assert ok, ("beta", err)
    dx, dg, db = backward(True, True, True)
    z = x.double() + r.double()
    xh = (z - z.mean(-1, keepdim=True)) / torch.sqrt(z.var(-1, unbiased=False, keepdim=True) + eps)
    for got, ref, what in ((dg.view(-1), (dy.double() * xh).sum(0), "dgamma"), (db.view(-1), dy.double().sum(0), "dbeta")):
        ok, err = close(got.cpu(), ref, rtol=1e-4, floor=1e-4)
        assert ok, (what, err)
    _, dg1, db1 = backward(False, True, True)
    assert torch.equal(dg1, dg) and torch.equal(db1, db)
    dx2, dg2, _ = backward(True, True, False)
    assert torch.equal(dx2, dx) and torch.equal(dg2, dg)
    dx3, _, db3 = backward(True, False, True)
    assert torch.equal(dx3, dx) and torch.equal(db3, db)
    dx4, _, _ = backward(True, False, False)                             # both parameters frozen: no partials at all
    assert torch.equal(dx4, dx)


def test_add_layernorm_outside_the_limit_is_refused_and_falls_back():
    from bcnf_amd import _native as N
    from bcnf_amd.feature_network import TransformerBlock
    d = 1028
    x = torch.randn(4, d, device=DEV)
    s = torch.empty(4, device=DEV)
    st = N.stream_handle(x.device)
    assert N.call_raw("bcnf_add_layernorm_forward", x, x, x[0], x[0], 4, d, 1e-5, x, s, s, st) == N.ERR_ARG
    assert N.call_raw("bcnf_add_layernorm_backward", x, x, x[0], s, s, x, 4, d, x, None, None, None, st) == N.ERR_ARG
    rc, _ = N.query_status("bcnf_add_layernorm_work_bytes", 4, d)
    assert rc == N.ERR_ARG
    torch.manual_seed(2)
    blk = TransformerBlock(d, 257, 8, dropout=0.0).to(DEV)              # head_dim 4; the norms exceed 1024
    xin = 0.5 * torch.randn(2, 5, d, device=DEV)
    y = blk(xin)
    with torch.no_grad():
        yr = copy.deepcopy(blk).double().cpu()(xin.double().cpu())
    ok, err = close(y.detach().cpu(), yr)
    assert ok, err


# ------------------------------------------------------------------------------------------ networks vs the fixture
@pytest.mark.parametrize("name", ["t1", "t2", "d1"])
def test_networks_match_the_reference(g16, name):
    net = build(name)
    net.load_state_dict(golden_sd(g16, f"{name}/sd/"))
    net.to(DEV).eval()
    h = net(t(g16[f"{name}/traj"]))
    ok, err = close(h.detach().cpu(), g16[f"{name}/h"])
    assert ok, err
    if name == "t2":
        return
    (h * t(g16[f"{name}/w"])).sum().backward()
    for pname, p in net.named_parameters():
        ok, err = close(p.grad.cpu(), g16[f"{name}/grad/{pname}"], rtol=1e-4, floor=1e-4)
        assert ok, (pname, err)


def test_network_runs_on_the_kernels(g16, monkeypatch):
    """The fused path is the one taken: two blocks call the attention Function twice and the residual + LayerNorm
    Function four times; with `fused` off on both classes neither is touched and the values agree."""
    from bcnf_amd import feature_network as F
    net = build("t1").to(DEV).eval()
    x = t(g16["t1/traj"])
    calls = []

    def spy(name, orig):
        def run(*a):
            calls.append(name)
            return orig(*a)
        return run
    monkeypatch.setattr(F._AttnFn, "apply", spy("attn", F._AttnFn.apply))
    monkeypatch.setattr(F._AddLayerNormFn, "apply", spy("ln", F._AddLayerNormFn.apply))
    h1 = net(x)
    assert calls.count("attn") == 2 and calls.count("ln") == 4
    calls.clear()
    monkeypatch.setattr(F.MultiHeadAttention, "fused", False)
    monkeypatch.setattr(F.TransformerBlock, "fused", False)
    h0 = net(x)
    assert not calls
    ok, err = close(h1.detach().cpu(), h0.detach().cpu())
    assert ok, err


def full_model(g16, train=False, **model_kwargs):
    from bcnf_amd import CondRealNVP_v2
    cfg = copy.deepcopy(MODEL_CFG)
    cfg["model"]["kwargs"].update(model_kwargs)
    torch.manual_seed(0)
    m = CondRealNVP_v2.from_config(cfg)
    m.load_state_dict(golden_sd(g16, "m/sd/"), strict=not model_kwargs.get("hybrid", False))
    return m.to(DEV).train(train)


def check_grads(named, g16, skip=()):
    n = 0
    for pname, g in named.items():
        if pname in skip:
            continue
        ok, err = close(g.cpu(), g16[f"m/grad/{pname}"], rtol=1e-4, floor=1e-4)
        assert ok, (pname, err)
        n += 1
    return n


def test_full_model_matches_the_reference_unfolded(g16):
    from bcnf_amd import inn_nll_loss
    m = full_model(g16)
    y, traj = t(g16["m/y"]), t(g16["m/traj"])
    z, h = m(y, traj, log_det_J=True, return_features=True)
    for got, key in ((h, "m/h"), (z, "m/z"), (m.log_det_J, "m/ldj")):
        ok, err = close(got.detach().cpu(), g16[key])
        assert ok, (key, err)
    nll = inn_nll_loss(z, m.log_det_J)
    assert abs(nll.item() - float(g16["m/nll"])) <= 1e-5 * abs(float(g16["m/nll"])) + 1e-5
    nll.backward()
    grads = {n: p.grad for n, p in m.named_parameters() if p.requires_grad}
    assert check_grads(grads, g16) == sum(k.startswith("m/grad/") for k in g16.keys())
    with torch.no_grad():
        inv = m.inverse(t(g16["m/z"]), traj)
    ok, err = close(inv.cpu(), g16["m/inv"])
    assert ok, ("inverse", err)


def nll_grads(m, y, traj, fold):
    m.fold_features = fold
    m.zero_grad(set_to_none=True)
    vals = m.nll_loss(y, traj)
    torch.autograd.backward(vals, torch.tensor([1.0, 0.0, 0.0], device=DEV))
    return vals.detach().cpu(), {n: p.grad.clone() for n, p in m.named_parameters() if p.grad is not None}


def test_full_model_folded_output_linear(g16):
    """nll_loss folds the Transformer's `output` Linear into the condition projection: the fixture's NLL and
    gradients, and the gates of the LSTM fold (tests/test_gpu_configs.py) against the unfolded launch."""
    m = full_model(g16)
    y, traj = t(g16["m/y"]), t(g16["m/traj"])
    fold = m._wide_fold(y, (traj,))
    assert fold is not None and fold[1] is m.feature_network_stack.feature_networks[1].output
    assert fold[0].shape == (12, 32)
    vf, gf = nll_grads(m, y, traj, True)
    vu, gu = nll_grads(m, y, traj, False)
    ref = float(g16["m/nll"])
    assert abs(vf[0].item() - ref) <= 1e-5 * abs(ref) + 1e-5 and vf[0].item() == vf[1].item()
    ok, err = close(vf, vu, rtol=1e-5, floor=1e-5)
    assert ok, ("vals", err)
    assert set(gf) == set(gu)
    assert check_grads(gf, g16) == sum(k.startswith("m/grad/") for k in g16.keys())
    for name in gf:
        ok, err = close(gf[name].cpu(), gu[name].cpu(), rtol=1e-4, floor=1e-4)
        assert ok, (name, err)


def test_dual_domain_fold_takes_the_last_fc_linear():
    from bcnf_amd import CondRealNVP_v2
    cfg = copy.deepcopy(MODEL_CFG)
    cfg["feature_networks"][1] = {"type": "DualDomainTransformer",
                                  "kwargs": dict(input_size=3, trf_size=32, n_heads=4, ff_size=32, n_blocks=1,
                                                 fc_sizes=[24, 16], fc_dropout=0.0, dropout=0.0, trf_dropout=0.0)}
    torch.manual_seed(1)
    m = CondRealNVP_v2.from_config(cfg).to(DEV).eval()
    gen = torch.Generator().manual_seed(4)
    y, traj = torch.randn(9, 21, generator=gen).to(DEV), torch.randn(9, 30, 3, generator=gen).to(DEV)
    fn = m.feature_network_stack.feature_networks[1]
    fold = m._wide_fold(y, (traj,))
    assert fold is not None and fold[1] is fn.fc.nn[-1] and fold[0].shape == (9, 24)
    vf, gf = nll_grads(m, y, traj, True)
    vu, gu = nll_grads(m, y, traj, False)
    ok, err = close(vf, vu, rtol=1e-5, floor=1e-5)
    assert ok, ("vals", err)
    assert set(gf) == set(gu)
    for name in gf:
        ok, err = close(gf[name].cpu(), gu[name].cpu(), rtol=1e-4, floor=1e-4)
        assert ok, (name, err)


# ------------------------------------------------------------------------------------------ TrainStep, sample
@pytest.mark.parametrize("hybrid", [False, True])
def test_trainstep_graph_equals_eager_steps(g16, hybrid):
    """All dropouts 0: three captured-and-replayed steps equal three eager steps on a deep copy, bit for bit. Three
    blocks = 52 feature-network tensors, more than one Adam / clip launch takes (48): TrainStep packs them into one
    flat parameter, and the members stay views of it with the clipped gradient as their .grad."""
    from bcnf_amd import CondRealNVP_v2
    from bcnf_amd.train import TrainStep
    cfg = copy.deepcopy(MODEL_CFG)
    cfg["model"]["kwargs"].update(dropout=0.0, hybrid=hybrid)
    cfg["feature_networks"][1]["kwargs"] = dict(T1, n_blocks=3, dropout=0.0, trf_dropout=0.0)
    torch.manual_seed(11)
    m1 = CondRealNVP_v2.from_config(cfg).to(DEV).train()
    m2 = copy.deepcopy(m1)
    kw = dict(hybrid_weight=1.0) if hybrid else {}
    s1 = TrainStep(m1, lr=2e-4, capture=True, **kw)
    s2 = TrainStep(m2, lr=2e-4, capture=False, **kw)
    assert s1._packed is not None and len(s1.params) == (4 if hybrid else 2)
    y, traj = t(g16["m/y"]), t(g16["m/traj"])
    before = [p.detach().clone() for p in m1.parameters()]
    for _ in range(3):
        v1 = s1.step(y, traj)
        v2 = s2.step(y, traj)                                          # capture=False: eager_step
        assert v1 == v2 and all(math.isfinite(v) for v in v1)
        assert (v1[2] > 0.0) == hybrid
    torch.cuda.synchronize()
    for (n1, p1), (n2, p2), p0 in zip(m1.named_parameters(), m2.named_parameters(), before):
        assert n1 == n2 and torch.equal(p1, p2), n1
        assert not p1.requires_grad or not torch.equal(p1, p0), n1        # every trainable tensor was updated
    fn = m2.feature_network_stack.feature_networks[1]
    total = torch.sqrt(sum((p.grad.double() ** 2).sum() for p in m2.parameters() if p.grad is not None))
    assert fn.layers[2].norm2.weight.grad is not None and float(total) <= 1.0 + 1e-4   # .grad shows the clipped gradient


def test_sample_with_log_prob(g16):
    m = full_model(g16)
    traj = t(g16["m/traj"])[:5]
    torch.manual_seed(21)
    draws, lp = m.sample(7, traj, outer=True, return_log_prob=True)
    assert draws.shape == (7, 5, 21) and lp.shape == (7, 5)
    with torch.no_grad():
        ref = torch.stack([m.log_prob(draws[i].to(DEV), traj) for i in range(7)]).cpu()
    ok, err = close(lp, ref)
    assert ok, err


def test_packed_trainstep_equals_adam_then_clip(g16):
    """The packed optimizer path (52 feature tensors in one flat parameter) against the Trainer's own sequence on a deep
    copy: backward, torch.optim.Adam(lr 2e-4).step(), clip_grad_norm_(1.0) over the per-tensor parameters."""
    from bcnf_amd import CondRealNVP_v2
    from bcnf_amd.train import TrainStep
    cfg = copy.deepcopy(MODEL_CFG)
    cfg["model"]["kwargs"].update(dropout=0.0)
    cfg["feature_networks"][1]["kwargs"] = dict(T1, n_blocks=3, dropout=0.0, trf_dropout=0.0)
    torch.manual_seed(12)
    m1 = CondRealNVP_v2.from_config(cfg).to(DEV).train()
    m2 = copy.deepcopy(m1)
    y, traj = t(g16["m/y"]), t(g16["m/traj"])
    s1 = TrainStep(m1, lr=2e-4, capture=False)
    assert s1._packed is not None
    loss, nll, _ = s1.step(y, traj)
    params = [p for p in m2.parameters() if p.requires_grad]
    start = [p.detach().clone() for p in params]
    vals = m2.nll_loss(y, traj)
    torch.autograd.backward(vals, torch.tensor([1.0, 0.0, 0.0], device=DEV))
    torch.optim.Adam(params, lr=2e-4).step()
    norm = torch.nn.utils.clip_grad_norm_(params, max_norm=1.0)
    assert abs(loss - vals[0].item()) <= 1e-5 * abs(vals[0].item()) + 1e-5 and loss == nll
    assert abs(float(s1.last_clip_norm) - float(norm)) <= 1e-4 * float(norm)
    named1 = dict(m1.named_parameters())
    for (name, p2), p0 in zip(((n, p) for n, p in m2.named_parameters() if p.requires_grad), start):
        ok, err = close(named1[name].detach().cpu(), p2.detach().cpu(), rtol=1e-5, floor=1e-5)
        assert ok, (name, err)
        assert not torch.equal(p2.detach(), p0), name
        if name.startswith("feature_network_stack."):                   # the packed members show the clipped gradient
            ok, err = close(named1[name].grad.cpu(), p2.grad.cpu(), rtol=1e-4, floor=1e-4)
            assert ok, (name, "grad", err)
