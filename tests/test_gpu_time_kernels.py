"""GPU tests of time_kernels (the per-launch device times bench.py reports): the keys each family returns on each
path, finite positive times, and that the timed launches leave nothing behind that the next training step depends on
(the dropout offset, the packed buffer)."""
import copy
import math

import pytest
import torch

from conftest import FC_SMALL_CFG, close

pytestmark = pytest.mark.gpu

DEV = "cuda"
B = 64
SMALL = {"k_forward", "k_backward", "tail"}
WIDE = {"forward", "backward"}


def _model(nested, n_blocks):
    from bcnf_amd import CondRealNVP_v2
    cfg = copy.deepcopy(FC_SMALL_CFG)
    cfg["model"]["kwargs"].update(nested_sizes=nested, n_blocks=n_blocks, n_conditions=80, dropout=0.1)
    del cfg["feature_networks"][1]["kwargs"]["dropout"]          # feature network: one Linear 90 -> 80
    torch.manual_seed(11)
    m = CondRealNVP_v2.from_config(cfg).to(DEV).train()
    m.flat_parameters()
    return m


def _step(m, y, traj, fold):
    m.fold_features = fold
    m.zero_grad(set_to_none=True)
    m.fused.flat_param.grad = None
    m.fused.set_seed(99)
    vals = m.nll_loss(y, traj)
    torch.autograd.backward(vals, torch.tensor([1.0, 0.0, 0.0], device=DEV))
    lin = m.feature_network_stack.feature_networks[1].nn[0]
    return [t.detach().clone().cpu() for t in (vals, m.fused.flat_param.grad, lin.weight.grad, lin.bias.grad)]


@pytest.mark.parametrize("family,fold,raw,keys", [
    ("FusedStack", False, True, SMALL),
    ("FusedStack", True, True, SMALL),                         # the pack-free forward: no pack launch
    ("FusedStack", True, False, SMALL | {"k_pack_fold"}),
    ("WideStack", False, True, WIDE),
    ("WideStack", True, True, WIDE),
])
def test_time_kernels_keys_and_no_residue(family, fold, raw, keys):
    m = _model([16] * 3, 4) if family == "FusedStack" else _model([48] * 2, 3)
    st = m.fused
    assert type(st).__name__ == family
    if family == "FusedStack":
        st.use_raw_forward = raw
        assert (st.raw_table(90) is not None) == raw
    gen = torch.Generator().manual_seed(5)
    y = torch.randn(B, 19, generator=gen).to(DEV)
    traj = torch.randn(B, 30, 3, generator=gen).to(DEV)
    before = _step(m, y, traj, fold)
    offset = int(st.rng_state()[1].item())
    assert offset == 1
    with torch.no_grad():
        h = m.feature_network_stack(traj).contiguous()
    lin = m.feature_network_stack.feature_networks[1].nn[0]
    spec = (traj.reshape(B, 90), lin.weight.detach(), lin.bias.detach()) if fold else None
    times = st.time_kernels(y, h, training=True, iters=2, fold=spec)
    assert set(times) == keys
    for k, v in times.items():
        assert math.isfinite(v) and v > 0.0, (k, v)
    assert int(st.rng_state()[1].item()) == offset           # no timed launch advanced the dropout stream
    after = _step(m, y, traj, fold)
    for a, b, what in zip(after, before, ("vals", "stack", "feature W", "feature b")):
        ok, err = close(a, b, rtol=1e-4, floor=1e-5)
        assert ok, (what, err)
