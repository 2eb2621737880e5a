"""GPU tests of the feature-Linear GEMM kernels of bcnf_train.hip (k_lin, k_gemm, k_gemm_wt, k_wt_reduce) through
their five entry points, bcnf_linear_forward / _backward, bcnf_linear_gelu_forward / _backward and
bcnf_linear_work_bytes, driven directly (N.call / N.call_raw) at the kernels' tile, slab, dispatch and split edges.

The reference is float64 on the host from the fp32 inputs the kernel sees: x W^T + b, the exact-erf GELU, and, in
training mode, the kernel's own dropout mask restated on the host (dropout_ref.feature_keep) times 1 / (1 - p);
gradients are autograd's on that float64 graph with the mask a constant. Values are held to close(1e-5, 1e-5),
gradients to close(1e-4, 1e-4) (tests/conftest.py); every output and the work buffer sit in NaN-guarded buffers."""
import functools
import math

import pytest
import torch

from conftest import close
from dropout_ref import feature_keep
from gpu_guard import DEV, canaries_alive, guarded

pytestmark = pytest.mark.gpu

SEED, OFFSET, SALT = 0x123456789ABCDEF, 2**32 + 5, 3

# (rows, in_features K, out_features N). The forward reduces over K, dX over N; LN_RMAX = 1024 is the largest
# reduction k_lin stages (larger: k_gemm); split_rows gives 128-row splits up to 4096 rows, then steps of 32.
CASES = [
    (1, 1, 1),              # smallest of everything
    (5, 3, 32),             # R < 4 (the Transformer Linears' in_features)
    (37, 90, 33),           # Nc one past the 32-column tile; K tail
    (65, 129, 47),          # M one past the 64-row workgroup; R = 16 * 8 + 1
    (129, 144, 17),         # second split of one row; R = 16 * 9 forwarded; dX reduction R = N = 17
    (161, 16, 16),          # a split ending in a 32-step plus a 1-row tail
    (64, 1024, 40),         # largest LDS slab
    (33, 1040, 20),         # first k_gemm reduction with a whole tail
    (33, 1027, 20),         # k_gemm tail with K % 4 = 3
    (20, 24, 1030),         # dX reduction R = N > 1024
    (4096, 8, 8),           # exactly 32 splits
    (4097, 8, 8),           # first split_rows step past 4096
]
SPLITS = {1: 1, 5: 1, 37: 1, 65: 1, 129: 2, 161: 2, 64: 1, 33: 1, 20: 1, 4096: 32, 4097: 26}

# mode -> (dropout p, salt, Philox offset); None: the plain Linear
MODES = {"linear": None, "gelu": (0.0, SALT, OFFSET), "train": (0.5, SALT, OFFSET), "train_p111": (0.111, 0, 0)}


def phi64(x):
    return 0.5 * torch.special.erfc(-x / math.sqrt(2.0))            # no cancellation for x < 0


def gelu64(x):
    return x * phi64(x)


def dgelu64(x):
    return phi64(x) + x * torch.exp(-0.5 * x * x) / math.sqrt(2.0 * math.pi)


@functools.lru_cache(maxsize=None)
def inputs(rows, K, Nf):
    """float64 x, W, b, dy holding fp32 values; pre-activations of about unit scale at every K."""
    gen = torch.Generator().manual_seed(rows * 1_000_003 + K * 1009 + Nf)
    x = torch.randn(rows, K, generator=gen, dtype=torch.float64)
    w = (2.0 * torch.rand(Nf, K, generator=gen, dtype=torch.float64) - 1.0) * (0.8 * math.sqrt(3.0 / K))
    b = 0.1 * torch.randn(Nf, generator=gen, dtype=torch.float64)
    dy = torch.randn(rows, Nf, generator=gen, dtype=torch.float64)
    return tuple(t.float().double() for t in (x, w, b, dy))


def keep_scale(mode, rows, Nf):
    """(bool keep mask, float64 mask x 1 / (1 - p)) the kernel applies in this mode."""
    p, salt, offset = MODES[mode]
    keep = torch.from_numpy(feature_keep(p, SEED, offset, salt, rows, Nf))
    p32 = float(torch.tensor(p, dtype=torch.float32))
    return keep, keep.double() / (1.0 - p32)


@functools.lru_cache(maxsize=None)
def reference(rows, K, Nf, mode, bias=True):
    x, w, b, dy = inputs(rows, K, Nf)
    xr, wr, br = (t.clone().requires_grad_(True) for t in (x, w, b))
    pre = xr @ wr.T + (br if bias else 0.0)
    pre.retain_grad()                                   # db of a layer without bias: the column sums of dL/dpre
    ref = {"pre": pre.detach()}
    if MODES[mode] is None:
        out = pre
    else:
        ref["keep"], m = keep_scale(mode, rows, Nf)
        out = gelu64(pre) * m
        ref["g"] = dgelu64(pre.detach()) * m
    out.backward(dy)
    ref.update(out=out.detach(), dx=xr.grad, dw=wr.grad, db=br.grad if bias else pre.grad.sum(0))
    return ref


def stream(N):
    return N.stream_handle(torch.device(DEV, torch.cuda.current_device()))


def rng_state(mode):
    return torch.tensor([SEED, MODES[mode][2]], dtype=torch.int64, device=DEV)


def launch(N, rows, K, Nf, mode, bias=True, want=("dx", "dw", "db"), backward=True):
    """One forward (+ backward) of the case in guarded buffers: {name: clone of the output}; the canaries are
    checked here. `want` names the gradients asked for; dweight without dbias leaves the work buffer's bias partials
    unwritten, and no dweight takes no work buffer."""
    x, w, b, dy = (t.float().to(DEV) for t in inputs(rows, K, Nf))
    st = stream(N)
    bd = b if bias else None
    ob, ov = guarded(rows, Nf)
    gb = gv = None
    if MODES[mode] is None:
        N.call("bcnf_linear_forward", x, w, bd, rows, K, Nf, ov, st)
    else:
        gb, gv = guarded(rows, Nf)
        p, salt, _ = MODES[mode]
        N.call("bcnf_linear_gelu_forward", x, w, bd, rows, K, Nf, p, rng_state(mode), salt, ov, gv, st)
    bufs = [("out", ob, ov, (rows, Nf))] + ([("g", gb, gv, (rows, Nf))] if gv is not None else [])
    if backward:
        dxb, dxv = guarded(rows, K) if "dx" in want else (None, None)
        dwb, dwv = guarded(Nf, K) if "dw" in want else (None, None)
        dbb, dbv = guarded(1, Nf) if "db" in want else (None, None)
        wfl = N.call_raw("bcnf_linear_work_bytes", rows, K, Nf) // 4
        assert wfl == SPLITS[rows] * (Nf * K + Nf)
        wb, wv = guarded(1, wfl) if "dw" in want else (None, None)
        if MODES[mode] is None:
            N.call("bcnf_linear_backward", x, w, dy, rows, K, Nf, dxv, dwv, dbv, wv, st)
        else:
            N.call("bcnf_linear_gelu_backward", x, w, dy, gv, rows, K, Nf, dxv, dwv, dbv, wv, st)
        bufs += [(n, bf, v, s) for n, bf, v, s in (("dx", dxb, dxv, (rows, K)), ("dw", dwb, dwv, (Nf, K)),
                                                   ("db", dbb, dbv, (1, Nf))) if bf is not None]
        if wb is not None:                    # without dbias the bias partials (the buffer's tail) stay NaN
            bufs.append(("work", wb, wv, (1, wfl if "db" in want else wfl - SPLITS[rows] * Nf)))
    torch.cuda.synchronize()
    for name, buf, _, shape in bufs:
        assert canaries_alive(buf, *shape), (name, "canary")
    return {name: v.clone() for name, _, v, _ in bufs if name != "work"}


def check(got, ref, names=("out", "g", "dx", "dw", "db")):
    for name in names:
        if name not in got:
            continue
        tight = name in ("out", "g")
        r = ref[name].view(got[name].shape)
        ok, err = close(got[name].cpu(), r, rtol=1e-5 if tight else 1e-4, floor=1e-5 if tight else 1e-4)
        print(f"{name}: max |err| {err:.3e} (max |ref| {float(r.abs().max()):.3e})")
        assert ok, (name, err)


def check_pattern(got, ref):
    """g != 0, and a != 0, are the host mask bit for bit: GELU' and GELU are nowhere near 0 on the reference, so a
    zero is a dropped unit."""
    assert bool((dgelu64(ref["pre"]).abs() > 1e-6).all()) and bool((gelu64(ref["pre"]).abs() > 1e-6).all())
    assert torch.equal(got["g"].cpu() != 0, ref["keep"])
    assert torch.equal(got["out"].cpu() != 0, ref["keep"])


@pytest.mark.parametrize("mode", ["linear", "gelu", "train"])
@pytest.mark.parametrize("rows,K,Nf", CASES)
def test_linear_against_float64(rows, K, Nf, mode):
    from bcnf_amd import _native as N
    ref = reference(rows, K, Nf, mode)
    runs = [launch(N, rows, K, Nf, mode) for _ in range(2)]
    assert set(runs[0]) == {"out", "dx", "dw", "db"} | ({"g"} if mode != "linear" else set())
    for name in runs[0]:
        assert torch.equal(runs[0][name], runs[1][name]), name          # fixed-order sums: the same bits
    check(runs[0], ref)
    if mode != "linear":
        check_pattern(runs[0], ref)


def test_linear_training_p111_salt0_offset0():
    from bcnf_amd import _native as N
    rows, K, Nf = 65, 129, 47
    ref = reference(rows, K, Nf, "train_p111")
    assert 0 < int((~ref["keep"]).sum()) < ref["keep"].numel() // 4
    got = launch(N, rows, K, Nf, "train_p111")
    check(got, ref)
    check_pattern(got, ref)


def test_mask_is_the_same_in_k_lin_and_k_gemm():
    """The same rows, N, salt and state at K = 1024 (k_lin) and K = 1040 (k_gemm): one kept pattern."""
    from bcnf_amd import _native as N
    rows, Nf = 33, 20
    pats = []
    for K in (1024, 1040):
        ref = reference(rows, K, Nf, "train")
        got = launch(N, rows, K, Nf, "train", backward=False)
        check(got, ref)
        check_pattern(got, ref)
        pats.append(got["g"] != 0)
    assert torch.equal(pats[0], pats[1])
    assert 0 < int(pats[0].sum()) < pats[0].numel()


@pytest.mark.parametrize("mode", ["linear", "train"])
@pytest.mark.parametrize("variant", ["no_bias", "no_dx", "no_dbias", "dx_only"])
@pytest.mark.parametrize("rows,K,Nf", [(37, 90, 33), (33, 1040, 20), (20, 24, 1030)])
def test_optional_arguments(rows, K, Nf, variant, mode):
    from bcnf_amd import _native as N
    bias = variant != "no_bias"
    want = {"no_bias": ("dx", "dw", "db"), "no_dx": ("dw", "db"), "no_dbias": ("dx", "dw"),
            "dx_only": ("dx",)}[variant]
    got = launch(N, rows, K, Nf, mode, bias=bias, want=want)
    assert set(got) == {"out", *want} | ({"g"} if mode != "linear" else set())
    check(got, reference(rows, K, Nf, mode, bias))
    full = launch(N, rows, K, Nf, mode, bias=bias)
    for name in got:                                   # what remains does not depend on what was left out
        assert torch.equal(got[name], full[name]), name


@pytest.mark.parametrize("K,Nf", [(5, 7), (1040, 3)])
def test_rows_zero(K, Nf):
    """No rows: the forwards write nothing, the backwards zero-fill dW and db and write nothing else."""
    from bcnf_amd import _native as N
    st = stream(N)
    x, w, b, dy = (t.float().to(DEV) for t in inputs(4, K, Nf))
    rng = rng_state("train")
    assert N.call_raw("bcnf_linear_work_bytes", 0, K, Nf) == 0
    (ob, ov), (gb, gv) = guarded(4, Nf), guarded(4, Nf)
    assert N.call_raw("bcnf_linear_forward", x, w, b, 0, K, Nf, ov, st) == N.OK
    assert N.call_raw("bcnf_linear_gelu_forward", x, w, b, 0, K, Nf, 0.5, rng, SALT, ov, gv, st) == N.OK
    for gelu in (False, True):
        (dxb, dxv), (dwb, dwv), (dbb, dbv), (wb, wv) = guarded(4, K), guarded(Nf, K), guarded(1, Nf), guarded(1, 8)
        if gelu:
            rc = N.call_raw("bcnf_linear_gelu_backward", x, w, dy, None, 0, K, Nf, dxv, dwv, dbv, wv, st)
        else:
            rc = N.call_raw("bcnf_linear_backward", x, w, dy, 0, K, Nf, dxv, dwv, dbv, wv, st)
        assert rc == N.OK
        torch.cuda.synchronize()
        assert canaries_alive(dwb, Nf, K) and canaries_alive(dbb, 1, Nf)
        assert bool((dwv == 0).all()) and bool((dbv == 0).all())
        assert bool(torch.isnan(dxb).all()) and bool(torch.isnan(wb).all())
    assert bool(torch.isnan(ob).all()) and bool(torch.isnan(gb).all())


def test_refusals_leave_the_outputs_untouched():
    from bcnf_amd import _native as N
    st = stream(N)
    rows, K, Nf = 9, 6, 5
    x, w, b, dy = (t.float().to(DEV) for t in inputs(rows, K, Nf))
    rng = rng_state("train")
    g = torch.ones(rows, Nf, device=DEV)
    wfl = N.call_raw("bcnf_linear_work_bytes", rows, K, Nf) // 4
    names = ("out", "g", "dx", "dw", "db", "work")
    shapes = ((rows, Nf), (rows, Nf), (rows, K), (Nf, K), (1, Nf), (1, wfl))

    def refused(fn):
        bufs = {n: guarded(*s) for n, s in zip(names, shapes)}
        rc = fn({n: v for n, (_, v) in bufs.items()})
        torch.cuda.synchronize()
        return rc == N.ERR_ARG and all(bool(torch.isnan(buf).all()) for buf, _ in bufs.values())

    for r, k, n in ((rows, 0, Nf), (rows, K, 0), (rows, -1, Nf), (rows, K, -1), (-1, K, Nf)):
        assert refused(lambda o: N.call_raw("bcnf_linear_forward", x, w, b, r, k, n, o["out"], st)), (r, k, n)
        assert refused(lambda o: N.call_raw("bcnf_linear_gelu_forward", x, w, b, r, k, n, 0.5, rng, SALT, o["out"],
                                            o["g"], st)), (r, k, n)
        assert refused(lambda o: N.call_raw("bcnf_linear_backward", x, w, dy, r, k, n, o["dx"], o["dw"], o["db"],
                                            o["work"], st)), (r, k, n)
        assert refused(lambda o: N.call_raw("bcnf_linear_gelu_backward", x, w, dy, g, r, k, n, o["dx"], o["dw"],
                                            o["db"], o["work"], st)), (r, k, n)
    for p in (1.0, -0.1, float("nan")):
        assert refused(lambda o: N.call_raw("bcnf_linear_gelu_forward", x, w, b, rows, K, Nf, p, rng, SALT, o["out"],
                                            o["g"], st)), p
    assert refused(lambda o: N.call_raw("bcnf_linear_gelu_backward", x, w, dy, None, rows, K, Nf, o["dx"], o["dw"],
                                        o["db"], o["work"], st))
    for name, extra in (("bcnf_linear_backward", ()), ("bcnf_linear_gelu_backward", (g,))):
        # dbias without dweight, dweight without work: refused before the dX launch
        assert refused(lambda o: N.call_raw(name, x, w, dy, *extra, rows, K, Nf, o["dx"], None, o["db"], o["work"],
                                            st)), name
        assert refused(lambda o: N.call_raw(name, x, w, dy, *extra, rows, K, Nf, o["dx"], o["dw"], o["db"], None,
                                            st)), name
        assert refused(lambda o: N.call_raw(name, x, w, dy, *extra, rows, K, Nf, o["dx"], o["dw"], None, None,
                                            st)), name


GELU_POINTS = [0.0, 1e-30, 1e-4, 0.5, 1.0, 2.0, 3.0, 4.0, 5.0, 6.5, 8.0, 9.9, 13.5, 20.0, 100.0]


def test_gelu_sweep():
    """K = 1, weight 1, no bias: pre is x exactly. a and g are finite and meet the gate against float64 over the whole
    sweep (scale 100) and over |x| <= 1 (scale 1); the measured errors are printed next to bcnf_device.h's claims
    (|GELU error| < 3.9e-7, |GELU' error| < 3.6e-7)."""
    from bcnf_amd import _native as N
    xs = torch.tensor([s * v for v in GELU_POINTS for s in (1.0, -1.0)], dtype=torch.float32)
    rows = xs.numel()
    assert rows == 30 and math.copysign(1.0, float(xs[1])) == -1.0
    one = torch.ones(1, 1, device=DEV)
    (ab, av), (gb, gv) = guarded(rows, 1), guarded(rows, 1)
    N.call("bcnf_linear_gelu_forward", xs.to(DEV).view(rows, 1), one, None, rows, 1, 1, 0.0, None, 0, av, gv,
           stream(N))
    torch.cuda.synchronize()
    assert canaries_alive(ab, rows, 1) and canaries_alive(gb, rows, 1)
    x64 = xs.double()
    small = x64.abs() <= 1.0
    for got, ref, what in ((av, gelu64(x64), "GELU"), (gv, dgelu64(x64), "GELU'")):
        got = got.cpu().view(-1)
        assert bool(torch.isfinite(got).all()), what
        err = (got.double() - ref).abs()
        i = int(err.argmax())
        print(f"{what}: max |err| {float(err.max()):.3e} at x = {float(xs[i])!r}; "
              f"over |x| <= 8: {float(err[x64.abs() <= 8.0].max()):.3e}; over |x| <= 1: {float(err[small].max()):.3e}")
        ok, e = close(got, ref)
        assert ok, (what, e)
        ok, e = close(got[small], ref[small])
        assert ok, (what, "|x| <= 1", e)


def test_fully_connected_network_training_end_to_end():
    """FullyConnectedFeatureNetwork([7, 20, 33, 5], dropout 0.3) in training mode against the float64 module chain fed
    feature_keep masks (salt = each Linear's module index, the run's one offset); the offset then advances by one."""
    from bcnf_amd.feature_network import FullyConnectedFeatureNetwork
    rows, p = 37, 0.3
    torch.manual_seed(1234)
    net = FullyConnectedFeatureNetwork([7, 20, 33, 5], dropout=p).to(DEV).train()
    dev = torch.device(DEV, torch.cuda.current_device())
    state = net.rng_state(dev)
    state[1] += 2**32 + 2                                   # both halves of the offset in use
    seed, offset = (int(v) for v in state.cpu())
    gen = torch.Generator().manual_seed(8)
    x = torch.randn(rows, 7, generator=gen)
    dout = torch.randn(rows, 5, generator=gen)
    xd = x.to(DEV).requires_grad_(True)
    out = net(xd)
    out.backward(dout.to(DEV))
    torch.cuda.synchronize()
    assert [int(v) for v in net.rng_state(dev).cpu()] == [seed, offset + 1]
    linears = [(i, m) for i, m in enumerate(net.nn) if isinstance(m, torch.nn.Linear)]
    assert [i for i, _ in linears] == [0, 3, 6]
    p32 = float(torch.tensor(p, dtype=torch.float32))
    params = [tuple(t.detach().cpu().double().requires_grad_(True) for t in (m.weight, m.bias)) for _, m in linears]
    xr = x.double().requires_grad_(True)
    h = xr
    for (i, m), (w, b) in zip(linears, params):
        h = h @ w.T + b
        if i != linears[-1][0]:
            assert bool((dgelu64(h.detach()).abs() > 1e-6).all())
            keep = torch.from_numpy(feature_keep(p, seed, offset, i, rows, m.out_features))
            assert 0 < int(keep.sum()) < keep.numel()
            h = gelu64(h) * (keep.double() / (1.0 - p32))
    h.backward(dout.double())
    ok, err = close(out.detach().cpu(), h.detach())
    assert ok, ("out", err)
    ok, err = close(xd.grad.cpu(), xr.grad, rtol=1e-4, floor=1e-4)
    assert ok, ("dx", err)
    for (i, m), (w, b) in zip(linears, params):
        for got, ref, what in ((m.weight.grad, w.grad, "weight"), (m.bias.grad, b.grad, "bias")):
            ok, err = close(got.cpu(), ref, rtol=1e-4, floor=1e-4)
            assert ok, (i, what, err)
