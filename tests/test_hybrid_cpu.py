"""CPU-side checks of the hybrid (NLL + prediction-head MSE) training step: what the reference fixture
tests/golden/g15_hybrid.npz means (recomputed in fp64 from its own tensors, no reference needed), that the hybrid
model's module tree carries the fixture's state_dict, the argument checks of the head C-ABI (they return before any
launch) and the error path of CondRealNVP_v2.hybrid_loss."""
import ctypes

import numpy as np
import pytest
import torch

from conftest import close, golden_sd, load_golden

NAMES = ['x0_x', 'x0_y', 'x0_z', 'v0_x', 'v0_y', 'v0_z', 'g_x', 'g_y', 'g_z', 'w_x', 'w_y', 'w_z', 'b', 'm',
         'a_x', 'a_y', 'a_z', 'r', 'A', 'Cd', 'rho']
# tests/golden/make_golden_hybrid.py CASES
CASES = {
    "a": dict(D=21, nested=[32] * 3, nb=4, C=32, fc=[60, 56, 56, 32], B=50, w=1.0),
    "b": dict(D=19, nested=[32] * 2, nb=3, C=37, fc=[90, 37], B=17, w=0.1),
    "c": dict(D=19, nested=[16] * 7, nb=4, C=80, fc=[90, 80], B=48, w=1.0),
}


def case_config(c, hybrid=True):
    return {
        "global": {"parameter_selection": NAMES[:c["D"]]},
        "model": {"kwargs": {"size": c["D"], "nested_sizes": list(c["nested"]), "n_conditions": c["C"],
                             "n_blocks": c["nb"], "dropout": 0.5, "act_norm": True, "hybrid": hybrid,
                             "random_state": 2024_03_25}},
        "feature_networks": [
            {"type": "ConcatenateCondition", "kwargs": {"input_size": None, "output_size": c["fc"][0]}},
            {"type": "FullyConnected", "kwargs": {"sizes": list(c["fc"])}},
        ],
    }


class Case:
    """One case of the fixture: keys without the "<case>/" prefix."""

    def __init__(self, g, name):
        self.name, self.cfg = name, CASES[name]
        pre = name + "/"
        self.d = {k[len(pre):]: g[k] for k in g.files if k.startswith(pre)}

    def __getitem__(self, k):
        return self.d[k]

    def keys(self):
        return self.d.keys()


@pytest.fixture(scope="module")
def g15():
    return load_golden("g15_hybrid.npz")


@pytest.mark.parametrize("name", ["a", "b", "c"])
def test_fixture_semantics(g15, name):
    """loss = (nll + w mse) / (1 + w), nll = mean(0.5 |z|^2 - ldj), mse = mean((h Wp^T + bp - y)^2), recomputed in
    fp64 from the fixture's h, z, ldj, y and prediction head: the project gate close(1e-5, 1e-5)."""
    c = Case(g15, name)
    f = lambda k: torch.from_numpy(np.asarray(c[k])).double()  # noqa: E731
    h, z, ldj, y = f("h"), f("z"), f("ldj"), f("y")
    w = c.cfg["w"]                                     # the fixture stores it rounded to fp32
    assert np.float32(w) == c["w"] and tuple(y.shape) == (c.cfg["B"], c.cfg["D"]) and h.shape[1] == c.cfg["C"]
    y_hat = h @ f("sd/prediction_head.weight").T + f("sd/prediction_head.bias")
    mse = ((y_hat - y) ** 2).mean()
    nll = (0.5 * (z ** 2).sum(dim=1) - ldj).mean()
    loss = (nll + w * mse) / (1 + w)
    for got, key in ((y_hat, "y_hat"), (mse, "mse"), (nll, "nll"), (loss, "loss")):
        ok, err = close(c[key], got)
        assert ok, (key, err)
    assert "grad/prediction_head.weight" in c.keys() and "after/prediction_head.bias" in c.keys()
    assert tuple(c["dh"].shape) == tuple(h.shape)


@pytest.mark.parametrize("name", ["a", "b", "c"])
def test_state_dict_and_flat_parameters(g15, name):
    from bcnf_amd import CondRealNVP_v2
    from bcnf_amd.fused import FusedStack
    from bcnf_amd.wide import WideStack
    c = Case(g15, name)
    m = CondRealNVP_v2.from_config(case_config(c.cfg))
    sd = golden_sd(c.d)
    assert set(m.state_dict().keys()) == set(sd.keys())
    m.load_state_dict(sd)
    assert type(m.fused) is (FusedStack if name == "c" else WideStack)
    flat = m.flat_parameters()
    for p in (m.prediction_head.weight, m.prediction_head.bias):
        assert any(q is p for q in flat)
    assert flat[0] is m.fused.flat_param
    assert tuple(m.prediction_head.weight.shape) == (c.cfg["D"], c.cfg["C"])


@pytest.mark.parametrize("name", ["a", "c"])
def test_families_are_siblings(g15, name):
    """The small and the wide family share StackBase and nothing else: the wide stack is no FusedStack and does not
    inherit the small family's pack-free forward switch, its table or the pending fused-Adam slot."""
    from bcnf_amd import CondRealNVP_v2
    from bcnf_amd.fused import FusedStack, StackBase
    from bcnf_amd.wide import WideStack
    assert not issubclass(WideStack, FusedStack) and not issubclass(FusedStack, WideStack)
    st = CondRealNVP_v2.from_config(case_config(Case(g15, name).cfg)).fused
    assert isinstance(st, StackBase)
    small = type(st) is FusedStack
    assert small == (name == "c")
    for member in ("raw_table", "use_raw_forward", "pending_adam"):
        assert hasattr(st, member) == small, member


def test_head_abi_argument_checks():
    """Bad arguments come back as BCNF_ERR_ARG before any launch (so this runs without a GPU); the workspace size is
    positive and does not decrease in B."""
    from bcnf_amd import _native as N
    L = N.lib()

    def wb(B, K, D):
        out = ctypes.c_int64(-1)
        return L.bcnf_head_work_bytes(B, K, D, ctypes.byref(out)), out.value

    prev = 0
    for B in [1, 2, 7, 8, 9, 15, 16, 17, 50, 255, 256, 257, 511, 512, 513, 1000, 4096, 4097, 100000]:
        for K, D in ((1, 2), (37, 19), (512, 21), (1360, 32)):
            rc, n = wb(B, K, D)
            assert rc == N.OK and n > 0 and n % 16 == 0
        rc, n = wb(B, 512, 21)
        assert n >= prev
        prev = n
    assert wb(256, 512, 21)[1] >= 4 * 256 * 21            # at least the residual
    for B, K, D in ((0, 8, 4), (-1, 8, 4), (8, 0, 4), (8, 8, 1), (8, 8, 33)):
        assert wb(B, K, D)[0] == N.ERR_ARG
    assert L.bcnf_head_work_bytes(8, 8, 4, None) == N.ERR_ARG

    buf = (ctypes.c_float * 4096)()                         # host memory: never dereferenced by a failing call
    addr = (ctypes.addressof(buf) + 63) // 64 * 64
    p = ctypes.c_void_p(addr)
    null = ctypes.c_void_p(0)

    def fwd(x=p, ldx=8, K=8, W=p, bias=p, y=p, B=4, D=4, work=p):
        return L.bcnf_head_mse_forward(x, ldx, K, W, bias, y, B, D, work, null)

    def bwd(x=p, ldx=8, K=8, W=p, work=p, B=4, D=4, ldd=8, weight=1.0):
        return L.bcnf_head_mse_backward(x, ldx, K, W, work, null, ctypes.c_float(weight), B, D, p, p, p, ldd, 1, null)

    for f in (fwd, bwd):
        assert f(D=1) == N.ERR_ARG
        assert f(D=33) == N.ERR_ARG
        assert f(ldx=7) == N.ERR_ARG
        assert f(B=0) == N.ERR_ARG
        assert f(x=null) == N.ERR_ARG
        assert f(W=null) == N.ERR_ARG
        assert f(work=null) == N.ERR_ARG
        assert f(K=0) == N.ERR_ARG
    assert fwd(y=null) == N.ERR_ARG
    assert bwd(ldd=7) == N.ERR_ARG
    assert bwd(weight=-1.0) == N.ERR_ARG
    assert bwd(weight=float("nan")) == N.ERR_ARG
    fin = L.bcnf_hybrid_finalize
    assert fin(null, p, 4, 4, ctypes.c_float(1.0), null, null) == N.ERR_ARG
    assert fin(p, null, 4, 4, ctypes.c_float(1.0), null, null) == N.ERR_ARG
    assert fin(p, p, 0, 4, ctypes.c_float(1.0), null, null) == N.ERR_ARG
    assert fin(p, p, 4, 33, ctypes.c_float(1.0), null, null) == N.ERR_ARG


def test_hybrid_loss_needs_a_hybrid_model():
    from bcnf_amd import CondRealNVP_v2
    c = CASES["c"]
    m = CondRealNVP_v2.from_config(case_config(c, hybrid=False))
    with pytest.raises(ValueError, match="hybrid=True"):
        m.hybrid_loss(torch.randn(4, 19), torch.randn(4, 30, 3), hybrid_weight=1.0)
    mh = CondRealNVP_v2.from_config(case_config(c))
    with pytest.raises(ValueError, match="hybrid_weight"):
        mh.hybrid_loss(torch.randn(4, 19), torch.randn(4, 30, 3), hybrid_weight=-1.0)
