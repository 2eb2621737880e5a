"""GPU tests of the folded backward tail (bcnf_fold_backward_tail): one launch that runs the split-K D1^T [x | 1]
(the split's 128 rows staged as two 64-row halves) in front of the slab reduce, with the copy of [Wf | bf] and the
Adam scalars on a workgroup of their own, then the Gx sum, then the two finishing GEMMs.

* shape grid: fold == unfolded at tests/test_gpu_fold.py's gates (loss 2e-6 relative, gradients rtol 1e-4 / floor
  1e-5) over the batch sizes at which the split-K changes shape (one 16-row slab, its edge, exactly one split, a
  second split of one row, a ragged last split) and block counts with a lone block / a half-empty block pair;
* determinism: the tail called again on the same buffers, and on slabs that held different garbage, gives the same
  bits;
* fused Adam == the tail without it followed by the Adam launch, bit for bit (the scalars each reduce workgroup
  derives for itself), and the gradients do not depend on the in-place update of Wf / bf (the tail's copy)."""
import copy
import ctypes

import numpy as np
import pytest
import torch

from conftest import FC_SMALL_CFG, close, golden_sd

pytestmark = pytest.mark.gpu

DEV = "cuda"


def _cfg(in_shape, C, nb=32):
    cfg = copy.deepcopy(FC_SMALL_CFG)
    cfg["model"]["kwargs"]["n_conditions"] = C
    cfg["model"]["kwargs"]["n_blocks"] = nb
    X = int(np.prod(in_shape))
    cfg["feature_networks"][0]["kwargs"]["output_size"] = X
    cfg["feature_networks"][1]["kwargs"]["sizes"] = [X, C]
    return cfg


def _model(g1, in_shape=(30, 3), C=80, nb=32, train=True):
    """FC_small with the reference's g1 weights where the shape is FC_small's, else a seeded random init."""
    from bcnf_amd import CondRealNVP_v2
    fc_small = (tuple(in_shape), C, nb) == ((30, 3), 80, 32)
    torch.manual_seed(3)
    m = CondRealNVP_v2.from_config(FC_SMALL_CFG if fc_small else _cfg(in_shape, C, nb))
    if fc_small:
        m.load_state_dict(golden_sd(g1))
    m.to(DEV)
    m.train(train)
    m.flat_parameters()
    return m


def _inputs(B, in_shape, seed):
    gen = torch.Generator().manual_seed(seed)
    return torch.randn(B, 19, generator=gen).to(DEV), torch.randn((B,) + tuple(in_shape), generator=gen).to(DEV)


def _grads(m, y, traj, fold, seed):
    m.fold_features = fold
    m.zero_grad(set_to_none=True)
    m.fused.flat_param.grad = None
    m.fused.set_seed(seed)
    vals = m.nll_loss(y, traj)
    torch.autograd.backward(vals, torch.tensor([1.0, 0.0, 0.0], device=DEV))
    lin = m.feature_network_stack.feature_networks[1].nn[0]
    return vals.detach().clone(), m.fused.flat_param.grad.clone(), lin.weight.grad.clone(), lin.bias.grad.clone()


def _check_fold_equals_unfolded(m, y, traj):
    assert m._foldable_linear(y, (traj,)) is not None
    v1, p1, w1, b1 = _grads(m, y, traj, True, 99)
    v0, p0, w0, b0 = _grads(m, y, traj, False, 99)
    assert abs(v1[0].item() - v0[0].item()) <= 2e-6 * abs(v0[0].item()) + 1e-6
    for a, b, what in ((p1, p0, "stack"), (w1, w0, "feature W"), (b1, b0, "feature b")):
        ok, err = close(a.cpu(), b.cpu(), rtol=1e-4, floor=1e-5)
        assert ok, (what, err)


@pytest.mark.parametrize("train", [False, True])
@pytest.mark.parametrize("nb", [1, 3, 32])
@pytest.mark.parametrize("B", [1, 16, 17, 128, 129, 300])
def test_fold_tail_shape_grid(g1, B, nb, train):
    m = _model(g1, nb=nb, train=train)
    y, traj = _inputs(B, (30, 3), 1000 * nb + B)
    _check_fold_equals_unfolded(m, y, traj)


@pytest.mark.parametrize("train", [False, True])
@pytest.mark.parametrize("in_shape,C,nb", [((20, 4), 80, 5), ((7, 3), 13, 3), ((79, 3), 96, 4)])
def test_fold_tail_other_shapes(g1, in_shape, C, nb, train):
    m = _model(g1, in_shape, C, nb, train=train)
    y, traj = _inputs(129, in_shape, 7)
    _check_fold_equals_unfolded(m, y, traj)


class _Pass:
    """One folded training forward, kept so that the backward and its tail can be called directly (as
    FusedStack.time_kernels does). x rows are padded to a multiple of 4 floats, TrainStep's pool layout."""

    def __init__(self, g1, B, in_shape=(30, 3), C=80, nb=32):
        from bcnf_amd import _native as N
        self.N, self.L = N, N.lib()
        self.m = m = _model(g1, in_shape, C, nb, train=True)
        self.st = m.fused
        self.B, self.X = B, int(np.prod(in_shape))
        y, traj = _inputs(B, in_shape, 11 + B + nb)
        pad = torch.zeros(B, (self.X + 3) // 4 * 4, device=DEV)
        pad[:, :self.X] = traj.reshape(B, self.X)
        self.x = pad[:, :self.X]
        lin = m.feature_network_stack.feature_networks[1].nn[0]
        self.wf, self.bf = lin.weight.detach().clone(), lin.bias.detach().clone()
        self.st.set_seed(5)
        with torch.no_grad():
            self.z, _, _, (self.ws, self.pk) = self.st.launch_fold_nll_forward(y, self.x, self.wf, self.bf, True,
                                                                               finalize=False)
        self.stream = N.stream_handle(y.device)

    def slab(self, fill):
        N = self.N
        sb = N.query_i64(self.L.bcnf_fold_slab_bytes, self.st._pdesc, ctypes.c_int32(self.X), ctypes.c_int64(self.B))
        return torch.empty(sb // 4, dtype=torch.float32, device=DEV).fill_(fill)

    def backward(self, slab):
        N = self.N
        N.check(self.L.bcnf_nll_backward(self.st._pdesc, N.ptr(self.pk), N.ptr(self.x), N.ptr(self.z), None,
                                         ctypes.c_int64(self.B), ctypes.c_int32(1), N.ptr(self.ws), None, None, None,
                                         N.ptr(slab), None, None, None, self.stream), "bcnf_nll_backward")

    def tail(self, slab, wf=None, bf=None, adam=None):
        N = self.N
        wf = self.wf if wf is None else wf
        bf = self.bf if bf is None else bf
        out = (torch.full_like(self.st.flat, float("nan")), torch.full_like(wf, float("nan")),
               torch.full_like(bf, float("nan")))
        N.check(self.L.bcnf_fold_backward_tail(self.st._pdesc, N.ptr(self.pk), N.ptr(slab), N.ptr(self.x),
                                               ctypes.c_int32(self.x.stride(0)), ctypes.c_int32(self.X), N.ptr(wf),
                                               N.ptr(bf), N.ptr(self.ws), ctypes.c_int64(self.B), ctypes.c_int32(1),
                                               N.ptr(out[0]), N.ptr(out[1]), N.ptr(out[2]),
                                               None if adam is None else ctypes.byref(adam), self.stream),
                "bcnf_fold_backward_tail")
        torch.cuda.synchronize()
        return out


# (79, 3) x 96: Xp = 240, float4 row loads with eight column tiles per wave (the grids above reach that width with
# contiguous rows of 237 floats only)
@pytest.mark.parametrize("B,in_shape,C,nb", [(300, (30, 3), 80, 3), (4096, (30, 3), 80, 32), (129, (79, 3), 96, 4)])
def test_fold_tail_is_deterministic(g1, B, in_shape, C, nb):
    p = _Pass(g1, B, in_shape, C, nb)
    slab = p.slab(float("nan"))
    p.backward(slab)
    first = p.tail(slab)
    assert all(torch.isfinite(t).all() for t in first)
    for _ in range(2):                                  # the same packed buffer, slab and workspace again
        again = p.tail(slab)
        assert all(torch.equal(a, b) for a, b in zip(first, again))
    other = p.slab(1e30)                                # a slab that held different garbage
    p.backward(other)
    assert all(torch.equal(a, b) for a, b in zip(first, p.tail(other)))


def _adam_state(p, step0):
    """Parameters (the stack's flat buffer, Wf, bf), non-trivial moments and the step count: two equal copies."""
    gen = torch.Generator().manual_seed(17)
    params = [p.st.flat.detach().clone(), p.wf.clone(), p.bf.clone()]
    m1 = [(0.01 * torch.randn(t.shape, generator=gen)).to(DEV) for t in params]
    m2 = [(1e-4 * torch.rand(t.shape, generator=gen)).to(DEV) for t in params]
    step = torch.tensor(float(step0), device=DEV)
    a = (params, m1, m2, step)
    b = ([t.clone() for t in params], [t.clone() for t in m1], [t.clone() for t in m2], step.clone())
    return a, b


HYPER = dict(lr=2e-4, b1=0.9, b2=0.999, eps=1e-8, wd=0.0)


def _fold_adam(N, state, counter):
    params, m1, m2, step = state
    spec = N.BcnfFoldAdam()
    for t in range(3):
        spec.params[t], spec.exp_avg[t], spec.exp_avg_sq[t] = params[t].data_ptr(), m1[t].data_ptr(), m2[t].data_ptr()
    spec.step = step.data_ptr()
    spec.lr, spec.beta1, spec.beta2 = HYPER["lr"], HYPER["b1"], HYPER["b2"]
    spec.eps, spec.weight_decay = HYPER["eps"], HYPER["wd"]
    spec.done_counter = counter.data_ptr()
    return spec


def _adam_launch(N, state, grads):
    params, m1, m2, step = state
    L = N.lib()
    total = sum(t.numel() for t in params)
    part = torch.empty(int(L.bcnf_grad_partials(total)), dtype=torch.float32, device=DEV)
    N.check(L.bcnf_adam_step(3, N.ptr_array(params), N.ptr_array(list(grads)), N.ptr_array(m1), N.ptr_array(m2),
                             N.i64_array([t.numel() for t in params]), N.ptr(step), ctypes.c_double(HYPER["lr"]),
                             ctypes.c_double(HYPER["b1"]), ctypes.c_double(HYPER["b2"]), ctypes.c_double(HYPER["eps"]),
                             ctypes.c_double(HYPER["wd"]), N.ptr(part), ctypes.c_int32(1), None,
                             N.stream_handle(params[0].device)), "bcnf_adam_step")
    torch.cuda.synchronize()


@pytest.mark.parametrize("step0", [0, 7])
@pytest.mark.parametrize("nb", [3, 32])
def test_fold_tail_fused_adam_equals_adam_launch(g1, nb, step0):
    """The tail with a BcnfFoldAdam == the tail without one followed by the Adam launch, from the same parameters,
    moments and step count. The fused update runs in place on the very Wf / bf the tail is given, as in TrainStep:
    the gradients must not see it (the tail's copy of [Wf | bf])."""
    p = _Pass(g1, 300, nb=nb)
    slab = p.slab(0.0)
    p.backward(slab)
    plain = p.tail(slab)
    ref, fused = _adam_state(p, step0)
    _adam_launch(p.N, ref, plain)
    counter = torch.zeros(4, dtype=torch.int32, device=DEV)
    spec = _fold_adam(p.N, fused, counter)
    got = p.tail(slab, wf=fused[0][1], bf=fused[0][2], adam=spec)
    for a, b in zip(plain, got):                        # dparams (its W1 condition columns among them), dWf, dbf
        assert torch.equal(a, b)
    assert fused[3].item() == ref[3].item() == step0 + 1
    for what, a, b in (("params", ref[0], fused[0]), ("exp_avg", ref[1], fused[1]), ("exp_avg_sq", ref[2], fused[2])):
        for t in range(3):
            assert torch.equal(a[t], b[t]), (what, t, (a[t] - b[t]).abs().max().item())
    assert not torch.equal(fused[0][1], p.wf)           # Wf was updated under the tail


def test_fold_tail_gradients_ignore_the_in_place_update(g1):
    """After a tail with Adam, dparams' W1 condition columns equal those of a tail without Adam on the same inputs,
    bit for bit, with a learning rate large enough that reading an updated Wf would show."""
    p = _Pass(g1, 300, nb=32)
    slab = p.slab(0.0)
    p.backward(slab)
    plain = p.tail(slab)
    _, fused = _adam_state(p, 0)
    spec = _fold_adam(p.N, fused, torch.zeros(4, dtype=torch.int32, device=DEV))
    spec.lr = 0.5
    got = p.tail(slab, wf=fused[0][1], bf=fused[0][2], adam=spec)
    assert (fused[0][1] - p.wf).abs().max().item() > 0.1
    L = p.st
    flat = plain[0]
    assert torch.equal(flat, got[0]) and torch.equal(plain[1], got[1]) and torch.equal(plain[2], got[2])
    # the W1 condition columns are where role a's product with [Wf | bf] lands: they are not all zero
    named = dict(p.m.named_parameters())
    w1 = [(off, k, q) for (off, k), q in zip(L._offsets, L.trainable)
          if any(v is q and n.endswith("nn.0.weight") for n, v in named.items())]
    assert w1
    off, k, q = w1[0]
    cond = flat[off:off + k].view(q.shape)[:, -80:]
    assert cond.abs().max().item() > 0
