"""CPU checks of the Transformer / DualDomainTransformer feature networks (reference feature_network.py:183-307,
401-471) against tests/golden/g16_transformer.npz (written by tests/golden/make_golden_transformer.py from the
reference itself): state_dict layout, forward and autograd gradients on torch ops, the positional table, the invalid
head split, and from_config on two of the reference's run configs. No kernel runs here."""
import copy

import numpy as np
import pytest
import torch

from conftest import close, golden_sd, load_golden

T1 = dict(input_size=3, trf_size=32, n_heads=4, ff_size=32, n_blocks=2, output_size=16,
          add_positional_embeddings=True)
T2 = dict(input_size=3, trf_size=100, n_heads=4, ff_size=32, n_blocks=1, output_size=16,
          add_positional_embeddings=False)
D1 = dict(input_size=3, trf_size=32, n_heads=4, ff_size=32, n_blocks=2, fc_sizes=[16],
          add_positional_embeddings=True)
NAMES = ['x0_x', 'x0_y', 'x0_z', 'v0_x', 'v0_y', 'v0_z', 'g_x', 'g_y', 'g_z', 'w_x', 'w_y', 'w_z', 'b', 'm',
         'a_x', 'a_y', 'a_z', 'r', 'A', 'Cd', 'rho']
MODEL_CFG = {
    "global": {"parameter_selection": NAMES},
    "model": {"kwargs": {"size": 21, "nested_sizes": [32] * 3, "n_conditions": 16, "n_blocks": 3, "act_norm": True,
                         "dropout": 0.5, "random_state": 2024_03_25}},
    "feature_networks": [{"type": "ConcatenateCondition", "kwargs": {"input_size": None, "output_size": 3}},
                         {"type": "Transformer", "kwargs": T1}],
}

# configs/runs/nll/t_PTRF_large.yaml and configs/runs/hybrid/t_DPTRF_small_hybrid.yaml as from_config sees them, the
# flow cut to 2 blocks; the last entry is the reference's parameter count of the feature network
PTRF_LARGE = ({
    "global": {"parameter_selection": NAMES},
    "model": {"kwargs": {"size": 21, "nested_sizes": [512] * 4, "n_conditions": 512, "n_blocks": 2, "dropout": 0.5,
                         "act_norm": True, "layer": "Linear", "activation": "GELU", "random_state": 2024_03_25}},
    "feature_networks": [
        {"type": "ConcatenateCondition", "kwargs": {"input_size": None, "output_size": 3}},
        {"type": "Transformer", "kwargs": {"input_size": 3, "trf_size": 256, "n_heads": 8, "ff_size": 256,
                                           "n_blocks": 7, "output_size": 512, "trf_dropout": 0.1, "dropout": 0.5,
                                           "add_positional_embeddings": True}}],
}, 2_903_040)
DPTRF_SMALL_HYBRID = ({
    "global": {"parameter_selection": NAMES},
    "model": {"kwargs": {"size": 21, "nested_sizes": [128] * 3, "n_conditions": 128, "n_blocks": 2, "dropout": 0.5,
                         "act_norm": True, "layer": "Linear", "activation": "GELU", "random_state": 2024_03_25,
                         "hybrid": True}},
    "feature_networks": [
        {"type": "ConcatenateCondition", "kwargs": {"input_size": None, "output_size": 3}},
        {"type": "DualDomainTransformer", "kwargs": {"input_size": 3, "trf_size": 32, "n_heads": 4, "ff_size": 32,
                                                     "n_blocks": 6, "fc_sizes": [128], "fc_dropout": 0.5,
                                                     "trf_dropout": 0.1, "dropout": 0.5,
                                                     "add_positional_embeddings": True}}],
}, 88_352)


@pytest.fixture(scope="module")
def g16():
    return load_golden("g16_transformer.npz")


def build(name):
    from bcnf_amd import CondRealNVP_v2
    from bcnf_amd.feature_network import DualDomainTransformer, Transformer
    if name == "t1":
        return Transformer(**T1)
    if name == "t2":
        return Transformer(**T2)
    if name == "d1":
        return DualDomainTransformer(**D1)
    return CondRealNVP_v2.from_config(MODEL_CFG)


def loaded(g16, name):
    net = build(name)
    net.load_state_dict(golden_sd(g16, f"{name}/sd/"))
    return net.eval()


@pytest.mark.parametrize("name", ["t1", "t2", "d1", "m"])
def test_state_dict_matches_the_reference_key_for_key(g16, name):
    sd = build(name).state_dict()
    ref = golden_sd(g16, f"{name}/sd/")
    assert sorted(sd) == sorted(ref)
    for k, v in sd.items():
        assert tuple(v.shape) == tuple(ref[k].shape), k
    if name == "d1":
        keys = list(sd)
        assert keys[0] == "time_transformer.features.weight" and keys[-2:] == ["fc.nn.0.weight", "fc.nn.0.bias"]
        assert "frequency_transformer.layers.1.ffn.2.bias" in keys and "time_transformer.layers.0.norm2.weight" in keys
    if name == "t1":
        assert list(sd)[2:12] == [f"layers.0.attention.{m}.{p}" for m in ("q_linear", "k_linear", "v_linear", "fc_out")
                                  for p in ("weight", "bias")] + ["layers.0.norm1.weight", "layers.0.norm1.bias"]
        assert list(sd)[-2:] == ["output.weight", "output.bias"]


@pytest.mark.parametrize("name", ["t1", "t2", "d1"])
def test_cpu_forward_matches_the_reference(g16, name):
    net = loaded(g16, name)
    with torch.no_grad():
        h = net(torch.from_numpy(g16[f"{name}/traj"]))
    ok, err = close(h, g16[f"{name}/h"])
    assert ok, err


def test_cpu_feature_stack_of_the_full_model_matches_the_reference(g16):
    m = loaded(g16, "m")
    with torch.no_grad():
        h = m.feature_network_stack(torch.from_numpy(g16["m/traj"]))
    ok, err = close(h, g16["m/h"])
    assert ok, err


@pytest.mark.parametrize("name", ["t1", "d1"])
def test_cpu_gradients_match_the_reference(g16, name):
    net = loaded(g16, name)
    h = net(torch.from_numpy(g16[f"{name}/traj"]))
    (h * torch.from_numpy(g16[f"{name}/w"])).sum().backward()
    n = 0
    for pname, p in net.named_parameters():
        ok, err = close(p.grad, g16[f"{name}/grad/{pname}"], rtol=1e-4, floor=1e-4)
        assert ok, (pname, err)
        n += 1
    assert n == sum(k.startswith(f"{name}/grad/") for k in g16.keys())


def test_positional_table_is_the_references_and_no_state():
    from bcnf_amd.feature_network import Transformer
    net = Transformer(**T1)
    table = net.positional_table(30, "cpu")
    want = torch.zeros(30, 32)
    for i in range(30):
        for j in range(3):
            if j % 2 == 0:
                want[i, j] = np.sin(i / 10000 ** (2 * j / 3))
            else:
                want[i, j] = np.cos(i / 10000 ** (2 * j / 3))
    assert table.dtype == torch.float32 and torch.equal(table, want)
    assert bool((table[:, 3:] == 0).all()) and float(table[1, 0]) == float(np.float32(np.sin(1.0)))
    assert net.positional_table(30, "cpu") is table                  # cached per (S, device)
    assert net.positional_table(16, "cpu").shape == (16, 32)
    assert not any("table" in k or "positional" in k for k in net.state_dict())
    assert len(net.state_dict()) == 2 + 2 * 16 + 2 and not list(net.buffers())
    net2 = copy.deepcopy(net)                                          # the cache never blocks a copy or a load
    net2.load_state_dict(net.state_dict())


def test_invalid_head_split_constructs_loads_and_raises_on_forward():
    from bcnf_amd.feature_network import DualDomainTransformer, Transformer
    a = Transformer(3, 46, 4, 32, 2, 16)                               # t_PTRF_small: 46 / 4
    b = Transformer(3, 46, 4, 32, 2, 16)
    b.load_state_dict(a.state_dict())
    with pytest.raises(RuntimeError, match=r"46.*4"):
        b(torch.randn(5, 30, 3))
    # the rare (S, d) where the reference's view happens to fit (S * 46 % 44 == 0) is refused as well
    with pytest.raises(RuntimeError, match=r"46.*4"):
        b(torch.randn(5, 22, 3))
    d = DualDomainTransformer(3, 70, 8, 32, 1, [16])                   # t_DPTRF_medium: 70 / 8
    with pytest.raises(RuntimeError, match=r"70.*8"):
        d(torch.randn(5, 30, 3))


@pytest.mark.parametrize("case", [PTRF_LARGE, DPTRF_SMALL_HYBRID], ids=["t_PTRF_large", "t_DPTRF_small_hybrid"])
def test_from_config_builds_the_reference_run_configs(case):
    from bcnf_amd import CondRealNVP_v2
    from bcnf_amd.feature_network import DualDomainTransformer, Transformer
    from bcnf_amd.wide import WideStack
    cfg, n_feature_params = case
    m = CondRealNVP_v2.from_config(cfg)
    fn = m.feature_network_stack.feature_networks[1]
    assert isinstance(fn, (Transformer, DualDomainTransformer))
    assert fn.n_params == n_feature_params
    assert fn.output_size == m.n_conditions
    assert isinstance(m.fused, WideStack) and m.fused.supported
    assert m.hybrid == ("hybrid" in cfg["model"]["kwargs"])
    with torch.no_grad():
        h = m.eval().feature_network_stack(torch.randn(2, 30, 3))
    assert h.shape == (2, m.n_conditions) and bool(torch.isfinite(h).all())


def test_packed_parameters_are_views_of_one_flat_parameter():
    """TrainStep's packing of a feature network with more tensors than one optimizer launch takes (host logic): the
    members keep their values and become views of the flat parameter in order, an update of the flat parameter is an
    update of the members, and gather() concatenates their gradients and leaves each .grad a view of the result."""
    from bcnf_amd import _native as N
    from bcnf_amd.feature_network import Transformer
    from bcnf_amd.train import _PackedParameters
    torch.manual_seed(4)
    net = Transformer(**dict(T1, n_blocks=3))
    members = list(net.parameters())
    assert len(members) == 2 + 3 * 16 + 2 > N.MAX_TENSORS
    before = [p.detach().clone() for p in members]
    packed = _PackedParameters(members)
    assert packed.intact() and packed.param.numel() == sum(p.numel() for p in members)
    assert all(torch.equal(p, b) for p, b in zip(members, before))
    assert torch.equal(packed.param.detach(), torch.cat([b.reshape(-1) for b in before]))
    with torch.no_grad():
        packed.param.mul_(2.0)
    assert all(torch.equal(p, 2.0 * b) for p, b in zip(members, before))
    net(torch.randn(2, 30, 3)).sum().backward()
    grads = [p.grad.clone() for p in members]
    packed.gather()
    assert packed.param.grad is packed.flat_grad
    assert torch.equal(packed.flat_grad, torch.cat([g.reshape(-1) for g in grads]))
    packed.flat_grad.mul_(0.5)                                           # the clip after the step scales in place
    assert all(torch.equal(p.grad, 0.5 * g) for p, g in zip(members, grads))
    packed.clear()
    assert all(p.grad is None for p in members)
    net.double()                                                         # replaces the members' storage
    assert not packed.intact()
