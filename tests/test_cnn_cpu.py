"""CPU checks of the CNN feature network (reference models/cnn.py) against tests/golden/g18_cnn*.npz (written by
tests/golden/make_golden_cnn.py from the reference itself): state_dict layout and the bit-exact initial state, the
padding rule, forward and autograd gradients on torch's own ops, a stride-2 network, the factory, from_config with an
LSTM behind the CNN, the dropout draw's restatement, and the C ABI's declarations and refusals. No kernel runs here."""
import hashlib
import os
import re

import numpy as np
import pytest
import torch

from conftest import ROOT, close, load_golden

NAMES = ['x0_x', 'x0_y', 'x0_z', 'v0_x', 'v0_y', 'v0_z', 'g_x', 'g_y', 'g_z', 'w_x', 'w_y', 'w_z', 'b', 'm',
         'a_x', 'a_y', 'a_z', 'r', 'A', 'Cd', 'rho']
C1 = dict(hidden_channels=[8, 16, 32], kernel_sizes=[8, 5, 3], strides=[1, 1, 1], output_size_lin=24, output_size=24,
          image_input_size=[26, 40], dropout_prob=0.5)
C2 = dict(C1, hidden_channels=[5, 10, 15], kernel_sizes=[3, 3, 5], num_CNN=2)
KWARGS = {"c1": C1, "c2": C2}
PROXY_SEED = {"c1": 18, "c2": 18, "m": 19}
MODEL_CFG = {
    "global": {"parameter_selection": NAMES},
    "model": {"kwargs": {"size": 21, "nested_sizes": [32] * 3, "n_conditions": 16, "n_blocks": 3, "act_norm": True,
                         "dropout": 0.5, "random_state": 2024_03_25}},
    "feature_networks": [{"type": "ConcatenateCondition", "kwargs": {"input_size": None, "output_size": [26, 40]}},
                         {"type": "CNN", "kwargs": dict(C1, output_size=96)},
                         {"type": "FullyConnected", "kwargs": {"sizes": [4 * 24, 16]}}],
}
# [ConcatenateCondition, CNN c1, LSTM(pool_dim=1)]: the shape of configs/runs/dev/videos_CNN_LSTM_*.yaml. The LSTM's
# inter-layer dropout is off: with it on, only the first training forward + backward of a process was seen to get
# non-zero gradients below the second layer of torch's MIOpen LSTM (whatever runs in front of it), which
# would make the GPU tests' "every feature gradient is non-zero" depend on the test order.
CNN_LSTM_CFG = {
    "global": {"parameter_selection": NAMES},
    "model": {"kwargs": {"size": 21, "nested_sizes": [32] * 3, "n_conditions": 16, "n_blocks": 3, "act_norm": True,
                         "dropout": 0.25, "random_state": 2024_03_25}},
    "feature_networks": [{"type": "ConcatenateCondition", "kwargs": {"input_size": [26, 40], "output_size": [26, 40]}},
                         {"type": "CNN", "kwargs": dict(C1)},
                         {"type": "LSTM", "kwargs": {"input_size": 24, "hidden_size": 16, "output_size": 16,
                                                     "num_layers": 2, "dropout": 0.0, "bidirectional": True,
                                                     "pooling": "mean", "pool_dim": 1}}],
}


def golden(name):
    """The archive holding `name` (make_golden_cnn.py splits the cases over three files)."""
    return load_golden({"m": "g18_cnn_m.npz", "c1_grad": "g18_cnn_c1_grad.npz"}.get(name, "g18_cnn.npz"))


def proxy_sd(model, seed):
    """tests/golden/make_golden_cnn.py:proxy_state -- numpy PCG64 weights in state_dict order (the orthonormal matrices
    are kept): the archives hold no weights."""
    rng = np.random.Generator(np.random.PCG64(seed))
    sd = {}
    for k, v in model.state_dict().items():
        if k.endswith("orthonormal_matrix"):
            sd[k] = v.detach().cpu()
            continue
        shape = tuple(v.shape)
        if k.endswith(".scale"):
            a = rng.uniform(0.7, 1.3, size=shape)
        elif len(shape) >= 2:
            a = rng.uniform(-1.0, 1.0, size=shape) / np.sqrt(np.prod(shape[1:]))
        else:
            a = rng.uniform(-0.05, 0.05, size=shape)
        sd[k] = torch.from_numpy(a.astype(np.float32))
    return sd


def build(name):
    from bcnf_amd import CNN, CondRealNVP_v2
    if name == "m":
        torch.manual_seed(2024_03_25)
        return CondRealNVP_v2.from_config(MODEL_CFG)
    return CNN(**KWARGS[name])


def loaded(name):
    net = build(name)
    sd = proxy_sd(net, PROXY_SEED[name])
    if name == "m":
        g = golden("m")
        for k in sd:
            if k.endswith("orthonormal_matrix"):
                sd[k] = torch.from_numpy(g[f"m/sd/{k}"])
    net.load_state_dict(sd)
    return net.eval()


def grads_of(name):
    g = golden("c1_grad" if name == "c1" else name)
    return {k[len(f"{name}/grad/"):]: g[k] for k in g.keys() if k.startswith(f"{name}/grad/")}


def test_state_dict_keys_and_bit_exact_initial_state():
    from bcnf_amd import CNN
    g = golden("c1")
    torch.manual_seed(5)
    sd = CNN(**C1).state_dict()
    want = [f"cnn_layers.0.{i}.{p}" for i in (0, 4, 8) for p in ("weight", "bias")] + ["final_layer.weight",
                                                                                       "final_layer.bias"]
    assert list(sd) == want and len(sd) == 8
    assert sorted("init/" + k for k in sd) == sorted(k for k in g.keys() if k.startswith("init/"))
    for k, v in sd.items():
        digest = np.frombuffer(hashlib.sha256(v.numpy().tobytes()).digest(), dtype=np.uint8)
        assert np.array_equal(digest, g["init/" + k]), k
        if v.dim() == 1:
            assert np.array_equal(v.numpy(), g["init_b/" + k]), k
    assert tuple(sd["cnn_layers.0.4.weight"].shape) == (16, 8, 5, 5)
    assert tuple(sd["final_layer.weight"].shape) == (24, 2 * 32 * 4 * 6)


def test_module_layout_and_the_padding_quirk():
    from bcnf_amd import CNN
    net = CNN(**C1)
    seq = net.cnn_layers[0]
    assert [type(m).__name__ for m in seq] == ["Conv2d", "ReLU", "Dropout", "MaxPool2d"] * 3 + ["Flatten"]
    assert seq[3] is net.pool and seq[7] is net.pool and seq[11] is net.pool            # the one shared pool module
    # layer i + 1 is padded from kernel_sizes[i]: 8 -> 3, 8 -> 3 (not 5 -> 2), 5 -> 2 (not 3 -> 1)
    assert [seq[i].padding for i in (0, 4, 8)] == [(3, 3), (3, 3), (2, 2)]
    assert [seq[i].kernel_size for i in (0, 4, 8)] == [(8, 8), (5, 5), (3, 3)]
    assert net.final_output_size == 32 * 4 * 6 and net.example_camera_input.shape == (1, 1, 26, 40)
    # the pooled sizes 25 x 39 -> 12 x 19, 14 x 21 -> 7 x 10, 9 x 12 -> 4 x 6 ... as the convolutions see them
    x = torch.zeros(1, 1, 26, 40)
    shapes = []
    for i in (0, 4, 8):
        x = seq[i](x)
        shapes.append(tuple(x.shape[2:]))
        x = net.pool(x)
    assert shapes == [(25, 39), (14, 21), (9, 12)]
    two = CNN(**C2)
    assert len(two.cnn_layers) == 2 and len(two.state_dict()) == 14
    assert [two.cnn_layers[1][i].padding for i in (0, 4, 8)] == [(1, 1), (1, 1), (1, 1)]
    # strides enter the rule with the size: stride 2 on 26 x 40 pads (25 + 6) // 2 by (39 + 6) // 2 ... for K = 8
    s2 = CNN([4, 4], [8, 3], [2, 1], 8, 8, [26, 40])
    assert s2.cnn_layers[0][0].padding == ((26 - 2 + 8) // 2, (40 - 2 + 8) // 2)


@pytest.mark.parametrize("name", ["c1", "c2"])
def test_cpu_forward_and_gradients_match_the_reference(name):
    net = loaded(name)
    g = golden(name)
    h = net(torch.from_numpy(g["videos"]))
    assert h.shape == (3, 4, 24)
    ok, err = close(h.detach(), g[f"{name}/h"])
    assert ok, err
    (h * torch.from_numpy(g[f"{name}/w"])).sum().backward()
    ref = grads_of(name)
    n = 0
    for pname, p in net.named_parameters():
        ok, err = close(p.grad, ref[pname], rtol=1e-4, floor=1e-4)
        assert ok, (pname, err)
        n += 1
    assert n == len(ref)


def test_cpu_full_model_matches_the_reference():
    m, g = loaded("m"), golden("m")
    videos = torch.from_numpy(golden("c1")["videos"])
    with torch.no_grad():
        h = m.feature_network_stack(videos)
    ok, err = close(h, g["m/h"])
    assert ok, err
    assert sum(k.startswith("m/grad/") for k in g.keys()) == len(list(m.named_parameters())) - 2   # 2 frozen matrices


def test_stride_two_runs_on_the_torch_modules():
    from bcnf_amd import CNN
    torch.manual_seed(1)
    net = CNN([4, 6], [3, 3], [2, 1], 8, 8, [26, 40], dropout_prob=0.0).eval()
    x = torch.randn(2, 2, 3, 26, 40)
    h = net(x)
    ref = net.double()(x.double())
    assert h.shape == (2, 3, 8)
    ok, err = close(h.detach(), ref.detach())
    assert ok, err


def test_factory_exports_and_from_config_with_an_lstm_behind():
    import bcnf_amd
    from bcnf_amd import CNN, CondRealNVP_v2
    from bcnf_amd.factories import FeatureNetworkFactory
    from bcnf_amd.feature_network import FEATURE_NETWORKS, FeatureRngMixin, FullyConnectedFeatureNetwork
    assert FEATURE_NETWORKS["CNN"] is CNN and bcnf_amd.CNN is CNN and "CNN" in bcnf_amd.__all__
    assert type(FeatureNetworkFactory.get_feature_network("CNN", dict(C1))) is CNN
    assert issubclass(CNN, FeatureRngMixin) and issubclass(FullyConnectedFeatureNetwork, FeatureRngMixin)
    torch.manual_seed(2)
    m = CondRealNVP_v2.from_config(CNN_LSTM_CFG)          # from_config ends in verify()
    m.verify()
    fns = list(m.feature_network_stack.feature_networks)
    assert [type(f).__name__ for f in fns] == ["ConcatenateCondition", "CNN", "LSTMFeatureNetwork"]
    assert fns[1].input_size == [26, 40] and fns[1].output_size == 24 and fns[2].pool_dim == 1
    with torch.no_grad():
        h = m.eval().feature_network_stack(torch.randn(2, 2, 4, 26, 40))
    assert h.shape == (2, 16) and bool(torch.isfinite(h).all())
    bad = {**CNN_LSTM_CFG, "feature_networks": [CNN_LSTM_CFG["feature_networks"][0],
                                                {"type": "CNN", "kwargs": dict(C1, output_size=25)},
                                                CNN_LSTM_CFG["feature_networks"][2]]}
    with pytest.raises(AssertionError):
        CondRealNVP_v2.from_config(bad)


def test_model_binds_the_cnn_to_its_dropout_state():
    from bcnf_amd.feature_network import _RNG_OWNERS
    m = build("m")
    cnn, fc = m.feature_network_stack.feature_networks[1:]
    assert _RNG_OWNERS[cnn]() is m and _RNG_OWNERS[fc]() is m


def test_conv_keep_restatement():
    from cnn_ref import conv_keep
    from dropout_ref import feature_keep, philox4x32_10, thresh32
    seed, offset, salt = (7 << 40) + 12345, (5 << 32) + 9, 4
    shape = (2, 3, 5, 7)
    keep = conv_keep(0.5, seed, offset, salt, shape)
    assert keep.shape == shape and keep.dtype == bool
    # unit by unit: word e & 3 of the draw of quad e >> 2
    k0 = (seed & 0xFFFFFFFF) ^ ((salt * 0x9E3779B9) & 0xFFFFFFFF)
    k1 = ((seed >> 32) ^ 0x40000000) & 0xFFFFFFFF
    flat = keep.reshape(-1)
    for e in (0, 1, 2, 3, 4, 7, 101, 209):
        words = philox4x32_10(e >> 2, 0, offset & 0xFFFFFFFF, offset >> 32, k0, k1)
        assert bool(flat[e]) == (int(words[e & 3]) >= thresh32(0.5)), e
    assert conv_keep(0.0, seed, offset, salt, shape).all()
    big = conv_keep(0.3, seed, offset, salt, (1, 1, 512, 512))
    q = 1.0 - thresh32(0.3) / 2**32
    assert abs(big.mean() - q) < 5 * np.sqrt(q * (1 - q) / big.size)
    for other in (conv_keep(0.5, seed, offset, salt + 1, shape), conv_keep(0.5, seed, offset + 1, salt, shape),
                  conv_keep(0.5, seed, offset + 2**32, salt, shape), conv_keep(0.5, seed ^ 1, offset, salt, shape),
                  conv_keep(0.5, seed ^ 2**32, offset, salt, shape)):
        assert not np.array_equal(keep, other)
    # not the feature Linear layers' draw for the same (seed, offset, salt)
    assert not np.array_equal(keep.reshape(30, 7), feature_keep(0.5, seed, offset, salt, 30, 7))


def test_header_declares_and_native_binds_the_conv_entry_points():
    from bcnf_amd import _native as N
    src = open(os.path.join(ROOT, "include", "bcnf_amd.h")).read()
    lib = N.lib()
    for name in ("bcnf_conv_block_forward", "bcnf_conv_block_work_bytes", "bcnf_conv_block_backward"):
        assert re.search(rf"^int\s+{name}\s*\(", src, flags=re.M), name
        assert name in N.EXPORTS
        fn = getattr(lib, name)
        assert fn.argtypes is not None and fn.restype is N._i32
    assert "models/cnn.py" in src and "0x40000000" in src
    assert len(lib.bcnf_conv_block_forward.argtypes) == 17 and len(lib.bcnf_conv_block_backward.argtypes) == 18
    # the work size is host arithmetic: the real first layer at the configs' batch, and a refusal
    assert N.query_i64("bcnf_conv_block_work_bytes", 1920, 1, 90, 160, 8, 8, 3, 3, 0.5) > 0
    assert N.query_status("bcnf_conv_block_work_bytes", 1, 1, 90, 160, 8, 9, 3, 3, 0.5)[0] == N.ERR_ARG
