"""CPU checks of the VerboseLSTM / DualDomainLSTM feature networks (reference feature_network.py:310-398) against
tests/golden/g17_dlstm*.npz (written by tests/golden/make_golden_dlstm.py from the reference itself): state_dict
layout, forward and autograd gradients on torch's own LSTM, the (x, h) pair, the factory, from_config on two of the
reference's run configs, copies, and the C ABI's declarations. No kernel runs here."""
import copy
import io
import os
import pickle
import re

import pytest
import torch

from conftest import ROOT, close, golden_sd, load_golden

L1 = dict(input_size=3, hidden_size=16, fc_sizes=[32], num_layers=1, bidirectional=True)
L2 = dict(input_size=3, hidden_size=32, fc_sizes=[16], num_layers=2, dropout=0.5, bidirectional=True, fc_dropout=0.5)
L3 = dict(input_size=3, hidden_size=48, fc_sizes=[24, 16], num_layers=3, bidirectional=False, pooling="max")
KWARGS = {"l1": L1, "l2": L2, "l3": L3}
NAMES = ['x0_x', 'x0_y', 'x0_z', 'v0_x', 'v0_y', 'v0_z', 'g_x', 'g_y', 'g_z', 'w_x', 'w_y', 'w_z', 'b', 'm',
         'a_x', 'a_y', 'a_z', 'r', 'A', 'Cd', 'rho']
MODEL_CFG = {
    "global": {"parameter_selection": NAMES},
    "model": {"kwargs": {"size": 21, "nested_sizes": [32] * 3, "n_conditions": 16, "n_blocks": 3, "act_norm": True,
                         "dropout": 0.5, "random_state": 2024_03_25}},
    "feature_networks": [{"type": "ConcatenateCondition", "kwargs": {"input_size": None, "output_size": 3}},
                         {"type": "DualDomainLSTM", "kwargs": L2}],
}


def dlstm_cfg(nested, n_blocks, hidden, layers, hybrid=False):
    """configs/runs/nll/t_DLSTM_*.yaml (hybrid: configs/runs/hybrid/t_DLSTM_*_hybrid.yaml) as from_config sees them."""
    model = {"size": 21, "nested_sizes": list(nested), "n_conditions": nested[0], "n_blocks": n_blocks, "dropout": 0.5,
             "act_norm": True, "layer": "Linear", "activation": "GELU", "random_state": 2024_03_25}
    if hybrid:
        model["hybrid"] = True
    return {"global": {"parameter_selection": NAMES}, "model": {"kwargs": model},
            "feature_networks": [
                {"type": "ConcatenateCondition", "kwargs": {"input_size": None, "output_size": 3}},
                {"type": "DualDomainLSTM", "kwargs": {"input_size": 3, "hidden_size": hidden, "num_layers": layers,
                                                      "dropout": 0.5, "bidirectional": True, "fc_sizes": [nested[0]],
                                                      "fc_dropout": 0.5, "pooling": "mean"}}]}


# the flow cut to 2 blocks; the last entry is the reference's parameter count of the feature network:
# per direction and layer 4 H (in + H + 2), in = 3 | 6 for the first layer and 2 H after it, plus the fc Linear
DLSTM_XSMALL = (dlstm_cfg([32] * 5, 2, 16, 1), 2 * (64 * 21 + 64 * 24) + 64 * 32 + 32)
DLSTM_SMALL = (dlstm_cfg([128] * 3, 2, 32, 2, hybrid=True),
               2 * (128 * 37 + 128 * 40) + 2 * 2 * 128 * 98 + 128 * 128 + 128)


def golden(name):
    """The archive holding case `name` (make_golden_dlstm.py splits the cases over three files)."""
    return load_golden({"l3": "g17_dlstm_l3.npz", "m": "g17_dlstm_m.npz"}.get(name, "g17_dlstm.npz"))


def build(name):
    from bcnf_amd import CondRealNVP_v2, DualDomainLSTM
    if name == "m":
        return CondRealNVP_v2.from_config(MODEL_CFG)
    return DualDomainLSTM(**KWARGS[name])


def loaded(name):
    net = build(name)
    net.load_state_dict(golden_sd(golden(name), f"{name}/sd/"))
    return net.eval()


@pytest.mark.parametrize("name", ["l1", "l2", "l3", "m"])
def test_state_dict_matches_the_reference_key_for_key(name):
    sd = build(name).state_dict()
    ref = golden_sd(golden(name), f"{name}/sd/")
    assert sorted(sd) == sorted(ref)
    for k, v in sd.items():
        assert tuple(v.shape) == tuple(ref[k].shape), k
    keys = list(sd)
    if name == "l1":
        assert keys[:4] == [f"lstm.lstm.0.{p}_l0" for p in ("weight_ih", "weight_hh", "bias_ih", "bias_hh")]
        assert keys[4] == "lstm.lstm.0.weight_ih_l0_reverse" and keys[-2:] == ["fc.nn.0.weight", "fc.nn.0.bias"]
    if name == "l2":        # dropout > 0: the Dropout entry leaves an index gap in the ModuleList
        assert "lstm.lstm.2.weight_ih_l0_reverse" in keys and "frequency_lstm.lstm.2.bias_hh_l0" in keys
        assert not any(k.startswith("lstm.lstm.1.") for k in keys)
        assert tuple(sd["lstm.lstm.2.weight_ih_l0"].shape) == (128, 64)
        assert tuple(sd["frequency_lstm.lstm.0.weight_ih_l0"].shape) == (128, 6)
    if name == "l3":        # dropout == 0: no gap
        assert "lstm.lstm.1.weight_hh_l0" in keys and "lstm.lstm.2.bias_ih_l0" in keys
        assert not any("reverse" in k for k in keys) and tuple(sd["fc.nn.0.weight"].shape) == (24, 96)


@pytest.mark.parametrize("name", ["l1", "l2", "l2x5", "l3"])
def test_cpu_forward_and_gradients_match_the_reference(name):
    net = loaded(name[:2])
    g = golden(name)
    h = net(torch.from_numpy(g[f"{name}/traj"]))
    ok, err = close(h.detach(), g[f"{name}/h"])
    assert ok, err
    (h * torch.from_numpy(g[f"{name[:2]}/w"])).sum().backward()
    n = 0
    for pname, p in net.named_parameters():
        ok, err = close(p.grad, g[f"{name}/grad/{pname}"], rtol=1e-4, floor=1e-4)
        assert ok, (pname, err)
        n += 1
    assert n == sum(k.startswith(f"{name}/grad/") for k in g.keys())


def test_cpu_feature_stack_of_the_full_model_matches_the_reference():
    m, g = loaded("m"), golden("m")
    with torch.no_grad():
        h = m.feature_network_stack(torch.from_numpy(g["m/traj"]))
    ok, err = close(h, g["m/h"])
    assert ok, err


def test_verbose_lstm_returns_x_and_every_layers_output():
    from bcnf_amd import VerboseLSTM
    torch.manual_seed(0)
    net = VerboseLSTM(3, 16, 3, dropout=0.25, bidirectional=True).eval()
    assert [type(m).__name__ for m in net.lstm] == ["LSTM", "Dropout", "LSTM", "Dropout", "LSTM"]
    x, h = net(torch.randn(5, 30, 3))
    assert x.shape == (5, 30, 32) and h.shape == (5, 3, 30, 32)
    assert torch.equal(h[:, 2], x)
    want = net.lstm[0](torch.zeros(1, 4, 3))[0]
    assert torch.equal(net(torch.zeros(1, 4, 3))[1][:, 0], want)
    x2, none = net(torch.zeros(1, 4, 3), return_h=False)
    assert none is None and x2.shape == (1, 4, 32)
    uni = VerboseLSTM(6, 16, 1)
    x, h = uni(torch.randn(2, 16, 6))
    assert x.shape == (2, 16, 16) and h.shape == (2, 1, 16, 16) and list(uni.state_dict()) == [
        "lstm.0.weight_ih_l0", "lstm.0.weight_hh_l0", "lstm.0.bias_ih_l0", "lstm.0.bias_hh_l0"]


def test_factory_and_exports():
    import bcnf_amd
    from bcnf_amd.factories import FeatureNetworkFactory
    from bcnf_amd.feature_network import FEATURE_NETWORKS, DualDomainLSTM, VerboseLSTM
    fn = FeatureNetworkFactory.get_feature_network("DualDomainLSTM", dict(L1))
    assert type(fn) is DualDomainLSTM and FEATURE_NETWORKS["DualDomainLSTM"] is DualDomainLSTM
    assert bcnf_amd.DualDomainLSTM is DualDomainLSTM and bcnf_amd.VerboseLSTM is VerboseLSTM
    assert "DualDomainLSTM" in bcnf_amd.__all__ and "VerboseLSTM" in bcnf_amd.__all__
    assert fn.input_size == 3 and fn.output_size == 32 and fn.fc.input_size == 2 * 16 * 2
    assert isinstance(fn.lstm, VerboseLSTM) and fn.frequency_lstm.input_size == 6
    c = fn.eval().combined(torch.randn(4, 30, 3))
    assert c.shape == (4, 64)


def test_invalid_pooling_raises():
    from bcnf_amd import DualDomainLSTM
    with pytest.raises(ValueError, match="median"):
        DualDomainLSTM(3, 16, [8], pooling="median")
    net = DualDomainLSTM(3, 16, [8])
    net.pooling = "median"                      # the reference raises on forward
    with pytest.raises(ValueError, match="median"):
        net(torch.randn(2, 30, 3))


@pytest.mark.parametrize("case", [DLSTM_XSMALL, DLSTM_SMALL], ids=["t_DLSTM_xsmall", "t_DLSTM_small_hybrid"])
def test_from_config_builds_the_reference_run_configs(case):
    from bcnf_amd import CondRealNVP_v2, DualDomainLSTM
    cfg, n_feature_params = case
    m = CondRealNVP_v2.from_config(cfg)
    fn = m.feature_network_stack.feature_networks[1]
    assert isinstance(fn, DualDomainLSTM)
    assert fn.n_params == n_feature_params
    kw = cfg["feature_networks"][1]["kwargs"]
    assert m.n_conditions == kw["fc_sizes"][-1] == fn.output_size
    assert m.fused.supported
    assert m.hybrid == ("hybrid" in cfg["model"]["kwargs"])
    with torch.no_grad():
        h = m.eval().feature_network_stack(torch.randn(2, 30, 3))
    assert h.shape == (2, m.n_conditions) and bool(torch.isfinite(h).all())


def test_deepcopy_and_pickle_round_trip():
    from bcnf_amd import CondRealNVP_v2
    torch.manual_seed(3)
    m = CondRealNVP_v2.from_config(MODEL_CFG).eval()
    traj = torch.randn(3, 30, 3)
    with torch.no_grad():
        h = m.feature_network_stack(traj)
    buf = io.BytesIO()
    torch.save(m, buf)
    buf.seek(0)
    for c in (copy.deepcopy(m), pickle.loads(pickle.dumps(m)), torch.load(buf, weights_only=False)):
        assert c.fused is not m.fused
        for (k, a), (k2, b) in zip(m.state_dict().items(), c.state_dict().items()):
            assert k == k2 and torch.equal(a, b)
        fm = m.feature_network_stack.feature_networks[1]
        fc = c.feature_network_stack.feature_networks[1]
        assert fc is not fm and fc.lstm.lstm[0].weight_hh_l0.data_ptr() != fm.lstm.lstm[0].weight_hh_l0.data_ptr()
        with torch.no_grad():
            assert torch.equal(c.eval().feature_network_stack(traj), h)
    pickle.loads(pickle.dumps(m.feature_network_stack.feature_networks[1]))


def test_header_declares_and_native_binds_the_lstm_entry_points():
    from bcnf_amd import _native as N
    src = open(os.path.join(ROOT, "include", "bcnf_amd.h")).read()
    lib = N.lib()
    for name in ("bcnf_lstm_forward", "bcnf_lstm_backward"):
        assert re.search(rf"^int\s+{name}\s*\(", src, flags=re.M), name
        assert name in N.EXPORTS
        fn = getattr(lib, name)
        assert fn.argtypes is not None and fn.restype is N._i32
    assert "feature_network.py:310-398" in src
    assert len(lib.bcnf_lstm_forward.argtypes) == 16 and len(lib.bcnf_lstm_backward.argtypes) == 14
    # refused before anything is launched: no GPU needed
    args_f = [None, None, 64, None, None, None, None, 1, 1, 16, 1, None, 16, None, None, None]
    assert lib.bcnf_lstm_forward(*args_f) == N.ERR_ARG
    args_b = [None, 16, None, None, None, None, 1, 1, 16, 1, None, None, 64, None]
    assert lib.bcnf_lstm_backward(*args_b) == N.ERR_ARG
