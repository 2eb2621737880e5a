"""GPU tests of the folded tail's slab-reduce shares: bcnf_fold_tail_plan cuts the reduce workgroups into ranges
that run behind the own workgroups of the tail's launches (k_fold_tail keeps three quarters, k_fold_finish runs the
last quarter, k_fold_gx's range is empty). At the smallest shapes where a share can go wrong (one block and one row;
two blocks and a ragged 16-row slab; three blocks with a second split of one row; FC_small's 32 blocks):

* every gradient is written (NaN-prefilled outputs come back finite) and does not depend on what the slab held;
* the fused Adam of every share == the tail without it followed by the Adam launch, bit for bit, at step counts 0 and
  7, and the step count advances exactly once (a share that updated twice, not at all, or took its scalars from an
  advanced step count shows here: k_fold_finish's share loads the scalars k_fold_tail published);
* outside the W1 condition columns dparams equals, bit for bit, what the unfolded reduce (bcnf_grad_reduce) writes
  from the same slabs. That comparison is the one used: the slab part of bcnf_fold_slab_bytes and of bcnf_slab_bytes
  is laid out alike (batch/16 slabs of the plan's stride), and both paths run the same fixed-order sum per element."""
import ctypes

import pytest
import torch

from test_gpu_fold_tail import DEV, _Pass, _adam_launch, _adam_state, _fold_adam

pytestmark = pytest.mark.gpu

SHAPES = [(1, 1), (2, 17), (3, 129), (32, 300)]          # (n_blocks, batch)


def _plan(p):
    out = (ctypes.c_int64 * 14)()
    p.N.check(p.L.bcnf_fold_tail_plan(p.st._pdesc, ctypes.c_int32(p.X), ctypes.c_int64(p.B), out),
              "bcnf_fold_tail_plan")
    return [int(v) for v in out]


@pytest.fixture(scope="module", params=SHAPES, ids=lambda s: f"nb{s[0]}-B{s[1]}")
def run(request, g1):
    """One forward + backward per shape, shared by the tests below (read-only): the pass, its slab (NaN before the
    backward wrote it) and the tail's outputs from it."""
    nb, B = request.param
    p = _Pass(g1, B, nb=nb)
    slab = p.slab(float("nan"))
    p.backward(slab)
    return p, slab, p.tail(slab)


def test_every_share_writes_its_gradients(run):
    p, slab, first = run
    plan = _plan(p)
    assert sum(plan[3:8:2]) == plan[0]                   # the three counts cover the reduce
    assert plan[3] >= 1 and plan[7] >= 1                 # both k_fold_tail and k_fold_finish run a share here
    assert all(torch.isfinite(t).all() for t in first)
    other = p.slab(1e30)                                # a slab that held different garbage
    p.backward(other)
    assert all(torch.equal(a, b) for a, b in zip(first, p.tail(other)))


@pytest.mark.parametrize("step0", [0, 7])
def test_fused_adam_of_every_share_equals_adam_launch(run, step0):
    p, slab, plain = run
    ref, fused = _adam_state(p, step0)
    _adam_launch(p.N, ref, plain)
    spec = _fold_adam(p.N, fused, torch.zeros(4, dtype=torch.int32, device=DEV))
    got = p.tail(slab, wf=fused[0][1], bf=fused[0][2], adam=spec)
    for a, b in zip(plain, got):
        assert torch.equal(a, b)
    assert fused[3].item() == ref[3].item() == step0 + 1
    for what, a, b in (("params", ref[0], fused[0]), ("exp_avg", ref[1], fused[1]), ("exp_avg_sq", ref[2], fused[2])):
        for t in range(3):
            assert torch.equal(a[t], b[t]), (what, t, (a[t] - b[t]).abs().max().item())


def test_shares_equal_the_unfolded_reduce(run):
    p, slab, first = run
    N, st = p.N, p.st
    plan = _plan(p)
    slab_floats = (p.B + 15) // 16 * plan[1]             # batch/16 slabs of the plan's stride
    sb = N.query_i64(p.L.bcnf_slab_bytes, st._pdesc, ctypes.c_int64(p.B))
    assert sb // 4 >= slab_floats
    unfolded = torch.zeros(sb // 4, dtype=torch.float32, device=DEV)
    unfolded[:slab_floats] = slab[:slab_floats]
    C = st.desc.n_conditions
    h = torch.zeros(p.B, C, device=DEV)                 # the W1 condition columns are not compared
    want = torch.full_like(st.flat, float("nan"))
    N.check(p.L.bcnf_grad_reduce(st._pdesc, N.ptr(unfolded), N.ptr(h), N.ptr(p.ws), ctypes.c_int64(p.B),
                                 ctypes.c_int32(1), N.ptr(want), p.stream), "bcnf_grad_reduce")
    torch.cuda.synchronize()
    keep = torch.ones_like(st.flat, dtype=torch.bool)
    named = dict(p.m.named_parameters())
    n_w1 = 0
    for (off, k), q in zip(st._offsets, st.trainable):
        if any(v is q and n.endswith("nn.0.weight") for n, v in named.items()):
            keep[off:off + k].view(q.shape)[:, -C:] = False
            n_w1 += 1
    assert n_w1 == st.desc.n_blocks
    assert torch.isfinite(want[keep]).all()
    assert torch.equal(first[0][keep], want[keep])
