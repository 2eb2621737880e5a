"""Generate g18_cnn.npz (cases c1, c2 and the init digests), g18_cnn_c1_grad.npz and g18_cnn_m.npz by running the
REFERENCE (psaegert/bcnf) on CPU: the CNN feature network (models/cnn.py), standalone and under a coupling stack.

Test infrastructure only, run like make_golden_dlstm.py (same dynaconf stub; nothing of the reference is copied, only
inputs / outputs). The reference checkout's src directory is the first argument, or $BCNF_REFERENCE_SRC:

    python tests/golden/make_golden_cnn.py path/to/reference/src

Weights: numpy PCG64(seed) in state_dict order (proxy_state below, restated as tests/test_cnn_cpu.py:proxy_sd, so the
archives hold no weights): 4-D conv weights U(-1, 1) / sqrt(c_in k^2), 2-D U(-1, 1) / sqrt(fan_in), 1-D
U(-0.05, 0.05), ActNorm scales U(0.7, 1.3); the orthonormal matrices are stored as built at
torch.manual_seed(2024_03_25). Inputs: numpy PCG64(7), N(0, 1). Every network is in eval mode; videos (3, 2, 4, 26, 40).

  case  network                                                                             stored
  c1    CNN([8,16,32], [8,5,3], [1,1,1], 24, 24, [26,40], dropout_prob=0.5)                  h, w, grad/* (own file);
        and its initial state_dict at torch.manual_seed(5)                                   init/<key> = SHA-256 of the
                                                                                             tensor's bytes, init_b/<bias>
  c2    the same with num_CNN=2, hidden_channels=[5,10,15], kernel_sizes=[3,3,5]             h, w, grad/*
  m     CondRealNVP_v2(size=21, nested_sizes=[32]*3, n_conditions=16, n_blocks=3,            h, z, ldj, inv = inverse(z),
        act_norm=True, dropout=0.5) on ConcatenateCondition([26,40]) + c1 (declared          nll, grad/* of the eval NLL
        output_size 96, what verify() compares) + FullyConnected([4*24, 16])

grad/* are the gradients of sum(h w). Each case also runs in float64, and the generator stops unless the reference's
fp32 values lie within a quarter of the value gate close(rtol=1e-5, floor=1e-5) of tests/conftest.py and its fp32
gradients within a quarter of the gradient gate close(rtol=1e-4, floor=1e-4): the fixture then leaves three quarters of
each gate to the code under test (and holds no window whose fp32 and float64 winners differ). Fixed zip timestamps: a
rerun reproduces the archives byte for byte. Three archives because a committed file stays under 1 MB.
"""
import copy
import hashlib
import io
import os
import sys
import tempfile
import zipfile

import numpy as np
import torch

REF_SRC = sys.argv[1] if len(sys.argv) > 1 else os.environ.get("BCNF_REFERENCE_SRC")
OUT = os.path.dirname(os.path.abspath(__file__))
NAMES = ['x0_x', 'x0_y', 'x0_z', 'v0_x', 'v0_y', 'v0_z', 'g_x', 'g_y', 'g_z', 'w_x', 'w_y', 'w_z', 'b', 'm',
         'a_x', 'a_y', 'a_z', 'r', 'A', 'Cd', 'rho']
VIDEOS = (3, 2, 4, 26, 40)
C1 = dict(hidden_channels=[8, 16, 32], kernel_sizes=[8, 5, 3], strides=[1, 1, 1], output_size_lin=24, output_size=24,
          image_input_size=[26, 40], dropout_prob=0.5)
C2 = dict(C1, hidden_channels=[5, 10, 15], kernel_sizes=[3, 3, 5], num_CNN=2)
MODEL_CFG = {
    "global": {"parameter_selection": NAMES},
    "model": {"kwargs": {"size": 21, "nested_sizes": [32] * 3, "n_conditions": 16, "n_blocks": 3, "act_norm": True,
                         "dropout": 0.5, "random_state": 2024_03_25}},
    "feature_networks": [{"type": "ConcatenateCondition", "kwargs": {"input_size": None, "output_size": [26, 40]}},
                         {"type": "CNN", "kwargs": dict(C1, output_size=96)},
                         {"type": "FullyConnected", "kwargs": {"sizes": [4 * 24, 16]}}],
}


def _import_reference():
    if not REF_SRC or not os.path.isdir(REF_SRC):
        raise SystemExit("usage: make_golden_cnn.py path/to/reference/src (or set BCNF_REFERENCE_SRC)")
    stub = tempfile.mkdtemp(prefix="bcnf_stub_")
    os.makedirs(os.path.join(stub, "dynaconf"))
    with open(os.path.join(stub, "dynaconf", "__init__.py"), "w") as f:
        f.write("class Dynaconf:\n    def __init__(self, *a, **k):\n        raise RuntimeError('stub')\n")
    sys.dont_write_bytecode = True
    sys.path[:0] = [stub, REF_SRC]
    import bcnf.models.cnf as cnf  # noqa
    import bcnf.models.cnn as cnn  # noqa
    import bcnf.utils as utils  # noqa
    return cnf, cnn, utils


def proxy_state(model, seed):
    rng = np.random.Generator(np.random.PCG64(seed))
    sd = {}
    for k, v in model.state_dict().items():
        if k.endswith("orthonormal_matrix"):
            sd[k] = v.detach().cpu().numpy()
            continue
        shape = tuple(v.shape)
        if k.endswith(".scale"):
            a = rng.uniform(0.7, 1.3, size=shape)
        elif len(shape) >= 2:
            a = rng.uniform(-1.0, 1.0, size=shape) / np.sqrt(np.prod(shape[1:]))
        else:
            a = rng.uniform(-0.05, 0.05, size=shape)
        sd[k] = a.astype(np.float32)
    return sd


def quarter_gate(what, a32, a64, rtol, floor):
    """|a32 - a64| <= (rtol |a64| + floor max(1, max|a64|)) / 4, else stop; returns the largest used fraction."""
    a = torch.as_tensor(a32, dtype=torch.float64)
    b = torch.as_tensor(a64, dtype=torch.float64)
    bound = rtol * b.abs() + floor * max(1.0, float(b.abs().max()))
    frac = float(((a - b).abs() / bound).max())
    if not frac <= 0.25:
        raise SystemExit(f"{what}: the reference's own fp32 error uses {frac:.3f} of the gate (limit 0.25)")
    return frac


def run_network(net, videos, w):
    net.zero_grad()
    h = net(videos)
    out = {"h": h.detach().numpy().copy()}
    (h * w).sum().backward()
    out.update({"grad/" + n: p.grad.detach().numpy().copy() for n, p in net.named_parameters()})
    return out


def network_case(name, net, videos, w):
    net.eval()
    net.load_state_dict({k: torch.from_numpy(v) for k, v in proxy_state(net, 18).items()})
    net64 = copy.deepcopy(net).double()
    got = run_network(net, videos, w)
    ref = run_network(net64, videos.double(), w.double())
    fv = quarter_gate(f"{name}/h", got["h"], ref["h"], 1e-5, 1e-5)
    fg = max(quarter_gate(f"{name}/{k}", got[k], ref[k], 1e-4, 1e-4) for k in got if k.startswith("grad/"))
    print(f"case {name}: h {got['h'].shape}, value gate used {fv:.3f}, gradient gate used {fg:.3f}")
    arrays = {f"{name}/{k}": v for k, v in got.items()}
    arrays[f"{name}/w"] = w.numpy()
    return arrays


def run_model(model, utils, y, videos):
    model.zero_grad()
    z, h = model.forward(y, videos, log_det_J=True, return_features=True)
    ldj = model.log_det_J
    nll = utils.inn_nll_loss(z, ldj)
    nll.backward()
    out = {"h": h.detach().numpy().copy(), "z": z.detach().numpy().copy(), "ldj": ldj.detach().numpy().copy(),
           "nll": np.asarray(nll.item())}
    out.update({"grad/" + n: p.grad.detach().numpy().copy() for n, p in model.named_parameters()
                if p.grad is not None})
    with torch.no_grad():
        out["inv"] = model.inverse(z.detach(), videos).numpy().copy()
    return out


def model_case(cnf, utils, y, videos):
    torch.manual_seed(2024_03_25)
    model = cnf.CondRealNVP_v2.from_config(MODEL_CFG)
    model.eval()
    model.load_state_dict({k: torch.from_numpy(v) for k, v in proxy_state(model, 19).items()})
    m64 = copy.deepcopy(model).double()
    m64.log_det_J = m64.log_det_J.double()
    got = run_model(model, utils, y, videos)
    ref = run_model(m64, utils, y.double(), videos.double())
    fv = max(quarter_gate(f"m/{k}", got[k], ref[k], 1e-5, 1e-5) for k in ("h", "z", "ldj", "inv"))
    fg = max(quarter_gate(f"m/{k}", got[k], ref[k], 1e-4, 1e-4) for k in got if k.startswith("grad/"))
    print(f"case m: nll {float(got['nll']):.5f}, value gate used {fv:.3f}, gradient gate used {fg:.3f}")
    got["nll"] = np.float32(got["nll"])
    # the orthonormal matrices are not proxy weights: stored as built
    out = {"sd/" + k: v.numpy() for k, v in model.state_dict().items() if k.endswith("orthonormal_matrix")}
    out.update(got, y=y.numpy())
    return {f"m/{k}": v for k, v in out.items()}


def write_npz(path, arrays):
    """np.savez_compressed with fixed entry timestamps (a rerun gives the same bytes)."""
    with zipfile.ZipFile(path, "w", zipfile.ZIP_DEFLATED) as zf:
        for key in sorted(arrays):
            buf = io.BytesIO()
            np.lib.format.write_array(buf, np.asanyarray(arrays[key]), allow_pickle=False)
            info = zipfile.ZipInfo(key + ".npy", date_time=(1980, 1, 1, 0, 0, 0))
            info.compress_type = zipfile.ZIP_DEFLATED
            info.external_attr = 0o644 << 16
            zf.writestr(info, buf.getvalue())


def main():
    cnf, cnn, utils = _import_reference()
    rng = np.random.Generator(np.random.PCG64(7))
    videos = torch.from_numpy(rng.standard_normal(VIDEOS).astype(np.float32))
    y = torch.from_numpy(rng.standard_normal((VIDEOS[0], 21)).astype(np.float32))
    w = torch.from_numpy(rng.standard_normal((VIDEOS[0], VIDEOS[2], 24)).astype(np.float32))
    arrays = {"videos": videos.numpy()}
    torch.manual_seed(5)
    init = cnn.CNN(**C1).state_dict()
    for k, v in init.items():
        arrays["init/" + k] = np.frombuffer(hashlib.sha256(v.numpy().tobytes()).digest(), dtype=np.uint8)
        if v.dim() == 1:
            arrays["init_b/" + k] = v.numpy()
    torch.manual_seed(2024_03_25)
    arrays.update(network_case("c1", cnn.CNN(**C1), videos, w))
    arrays.update(network_case("c2", cnn.CNN(**C2), videos, w))
    arrays.update(model_case(cnf, utils, y, videos))

    def part(k):
        case = k.split("/")[0]
        if case == "m":
            return "g18_cnn_m.npz"
        return "g18_cnn_c1_grad.npz" if k.startswith("c1/grad/") else "g18_cnn.npz"
    for fname in ("g18_cnn.npz", "g18_cnn_c1_grad.npz", "g18_cnn_m.npz"):
        path = os.path.join(OUT, fname)
        write_npz(path, {k: v for k, v in arrays.items() if part(k) == fname})
        size = os.path.getsize(path)
        print(f"{path}: {size} bytes")
        if size > 1000_000:
            raise SystemExit(f"{fname} is over 1 MB")


if __name__ == "__main__":
    main()
