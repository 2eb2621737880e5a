"""The oracle's `keep` hook (oracle/cnf_oracle.py): dropout masks handed in from outside, so the GPU training-parity
tests (tests/test_gpu_train_parity.py) can feed the fp64 oracle the HIP kernels' own masks. Pinned here on the CPU:
replaying exactly what a seeded `gen` draws reproduces the `gen` path bit for bit (same expression, same call order,
the (coupling, half, layer) indices in the documented order), and all-true masks at a dropout whose scale rounds to 1
reproduce eval mode."""
import pytest
import torch

from oracle import cnf_oracle as O

SPECS = [
    O.StackSpec(size=7, nested_sizes=[12, 9], n_blocks=3, n_conditions=5, dropout=0.3, act_norm=True, two_way=True),
    O.StackSpec(size=19, nested_sizes=[16] * 3, n_blocks=4, n_conditions=8, dropout=0.383, act_norm=False),
]


def _sd(spec, seed=0, dtype=torch.float32):
    g = torch.Generator().manual_seed(seed)
    sd = {}
    idx = O.mlp_linear_indices(spec)
    for li, kind in enumerate(O.layer_kinds(spec)):
        p = f"layers.{li}"
        if kind == "actnorm":
            sd[p + ".scale"] = (0.5 + torch.rand(spec.size, generator=g)).to(dtype)
            sd[p + ".bias"] = (0.1 * torch.randn(spec.size, generator=g)).to(dtype)
        elif kind == "ortho":
            q, _ = torch.linalg.qr(torch.randn(spec.size, spec.size, generator=g))
            sd[p + ".orthonormal_matrix"] = q.to(dtype)
        else:
            for half, nin, nout in (("nn_a", spec.Da, spec.Db), ("nn_b", spec.Db, spec.Da))[:2 if spec.two_way else 1]:
                widths = [nin + spec.n_conditions] + list(spec.nested_sizes) + [2 * nout]
                for j, i in enumerate(idx):
                    w = torch.randn(widths[j + 1], widths[j], generator=g) / widths[j] ** 0.5
                    sd[f"{p}.{half}.nn.{i}.weight"] = w.to(dtype)
                    sd[f"{p}.{half}.nn.{i}.bias"] = (0.1 * torch.randn(widths[j + 1], generator=g)).to(dtype)
    return sd


def _replay(spec, B, seed, calls):
    """`keep` that draws what nested_mlp's `gen` path draws, in call order, and logs the indices it was asked for."""
    gen = torch.Generator().manual_seed(seed)

    def keep(k, half, li):
        calls.append((k, half, li))
        return torch.rand((B, spec.nested_sizes[li]), generator=gen) >= spec.dropout
    return keep


@pytest.mark.parametrize("spec", SPECS, ids=["two_way", "one_way"])
@pytest.mark.parametrize("dtype", [torch.float32, torch.float64])
def test_keep_replaying_gen_is_bit_identical(spec, dtype):
    B = 11
    sd = _sd(spec, dtype=dtype)
    g = torch.Generator().manual_seed(1)
    y = torch.randn(B, spec.size, generator=g).to(dtype)
    h = torch.randn(B, spec.n_conditions, generator=g).to(dtype)
    halves = ["a", "b"] if spec.two_way else ["a"]
    order = [(k, s, li) for k in range(spec.n_blocks) for s in halves for li in range(len(spec.nested_sizes))]

    z0, l0 = O.model_forward(sd, spec, y, h, training=True, gen=torch.Generator().manual_seed(5))
    calls = []
    z1, l1 = O.model_forward(sd, spec, y, h, training=True, keep=_replay(spec, B, 5, calls))
    assert torch.equal(z0, z1) and torch.equal(l0, l1) and z1.dtype == dtype
    assert calls == order
    ze, _ = O.model_forward(sd, spec, y, h)
    assert not torch.equal(z0, ze)                       # the masks did something

    i0 = O.model_inverse(sd, spec, y, h, training=True, gen=torch.Generator().manual_seed(6))
    calls = []
    i1 = O.model_inverse(sd, spec, y, h, training=True, keep=_replay(spec, B, 6, calls))
    assert torch.equal(i0, i1)
    assert calls == [(k, s, li) for k in reversed(range(spec.n_blocks)) for s in halves
                     for li in range(len(spec.nested_sizes))]

    # a single coupling layer takes the same hook (index = what the caller says)
    p = f"layers.{O.layer_kinds(spec).index('coupling')}"
    c0 = O.coupling_forward(sd, p, spec, y, h, True, torch.Generator().manual_seed(7))
    calls = []
    c1 = O.coupling_forward(sd, p, spec, y, h, True, keep=_replay(spec, B, 7, calls), index=4)
    assert torch.equal(c0[0], c1[0]) and torch.equal(c0[1], c1[1]) and {c[0] for c in calls} == {4}
    v0 = O.coupling_inverse(sd, p, spec, y, h, True, torch.Generator().manual_seed(8))
    v1 = O.coupling_inverse(sd, p, spec, y, h, True, keep=_replay(spec, B, 8, []), index=4)
    assert torch.equal(v0, v1)


@pytest.mark.parametrize("spec", SPECS, ids=["two_way", "one_way"])
def test_all_true_keep_at_unit_scale_is_eval_mode(spec):
    """p = 1e-30: Dropout layers exist (stride-3 state dict), 1 - p rounds to 1, so all-true masks leave x * 1 / 1."""
    spec = O.StackSpec(**{**spec.__dict__, "dropout": 1e-30})
    assert 1.0 - spec.dropout == 1.0
    B = 9
    sd = _sd(spec, dtype=torch.float64)
    g = torch.Generator().manual_seed(2)
    y = torch.randn(B, spec.size, generator=g).double()
    h = torch.randn(B, spec.n_conditions, generator=g).double()
    ones = lambda k, half, li: torch.ones(B, spec.nested_sizes[li], dtype=torch.bool)  # noqa: E731
    ze, le = O.model_forward(sd, spec, y, h)
    zk, lk = O.model_forward(sd, spec, y, h, training=True, keep=ones)
    assert torch.equal(ze, zk) and torch.equal(le, lk)
    assert torch.equal(O.model_inverse(sd, spec, y, h), O.model_inverse(sd, spec, y, h, training=True, keep=ones))


def test_sample_hands_each_inverse_call_its_own_keep():
    spec = SPECS[1]
    sd = _sd(spec)
    cond = torch.randn(5, spec.n_conditions, generator=torch.Generator().manual_seed(3))
    seen = []

    def keeps(n, rows):
        seen.append((n, rows))
        return lambda k, half, li: torch.ones(rows, spec.nested_sizes[li], dtype=torch.bool)

    torch.manual_seed(4)
    s = O.sample(sd, spec, 5, cond, outer=True, batch_size=3, sample_batch_size=4, keeps=keeps)
    assert s.shape == (5, 5, spec.size)
    assert seen == [(0, 12), (1, 3), (2, 8), (3, 2)]      # (4 + 1 samples) x (3 + 2 conditions), one call each
    torch.manual_seed(4)
    e = O.sample(sd, spec, 5, cond, outer=True, batch_size=3, sample_batch_size=4)
    assert not torch.equal(s, e)                           # masks of all ones still scale by 1 / (1 - p)
