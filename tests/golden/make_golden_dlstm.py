"""Generate g17_dlstm.npz (cases l1, l2), g17_dlstm_l3.npz and g17_dlstm_m.npz by running the REFERENCE
(psaegert/bcnf) on CPU: the DualDomainLSTM feature network (feature_network.py:310-398, VerboseLSTM inside it),
standalone and under a coupling stack.

Test infrastructure only, run like make_golden_transformer.py (same dynaconf stub; nothing of the reference is copied,
only inputs / outputs). The reference checkout's src directory is the first argument, or $BCNF_REFERENCE_SRC:

    python tests/golden/make_golden_dlstm.py path/to/reference/src

Weights: numpy PCG64(seed) in state_dict order as make_golden.py's large_proxy_state (2-D: U(-1, 1) / sqrt(fan_in),
1-D: U(-0.05, 0.05), ActNorm scales: U(0.7, 1.3); the orthonormal matrices are kept). Inputs: numpy PCG64(7). Every
network is in eval mode, B = 12, trajectories (12, 30, 3).

  case  network                                                                        trajectories  stored
  l1    DualDomainLSTM(3, 16, [32], num_layers=1, bidirectional=True)  (t_DLSTM_xsmall) 5 N(0, 1)     sd, h, w, grad/*
  l2    DualDomainLSTM(3, 32, [16], num_layers=2, dropout=0.5, bidirectional=True,     N(0, 1)       sd, h, w, grad/*
        fc_dropout=0.5)                                                                 5 N(0, 1)     as l2x5/*
  l3    DualDomainLSTM(3, 48, [24, 16], num_layers=3, bidirectional=False,             5 N(0, 1)     sd, h, w, grad/*
        pooling='max')
  m     CondRealNVP_v2(size=21, nested_sizes=[32]*3, n_conditions=16, n_blocks=3, act_norm=True, dropout=0.5) on
        ConcatenateCondition(None, 3) + the l2 network                                  5 N(0, 1)     h, z, ldj, inv =
        inverse(z), nll, grad/* of the eval NLL

grad/* are the gradients of sum(h w). Each case also runs in float64, and the generator stops unless the reference's
fp32 values lie within a quarter of the value gate close(rtol=1e-5, floor=1e-5) of tests/conftest.py and its fp32
gradients within a quarter of the gradient gate close(rtol=1e-4, floor=1e-4): the fixture then leaves three quarters of
each gate to the code under test. Fixed zip timestamps: a rerun reproduces the archives byte for byte. Three archives
because the weights and gradients of all four cases together are 2.3 MB and a committed file stays under 1 MB.
"""
import copy
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
B = 12
L1 = dict(input_size=3, hidden_size=16, fc_sizes=[32], num_layers=1, bidirectional=True)
L2 = dict(input_size=3, hidden_size=32, fc_sizes=[16], num_layers=2, dropout=0.5, bidirectional=True, fc_dropout=0.5)
L3 = dict(input_size=3, hidden_size=48, fc_sizes=[24, 16], num_layers=3, bidirectional=False, pooling="max")
MODEL_CFG = {
    "global": {"parameter_selection": NAMES},
    "model": {"kwargs": {"size": 21, "nested_sizes": [32] * 3, "n_conditions": 16, "n_blocks": 3, "act_norm": True,
                         "dropout": 0.5, "random_state": 2024_03_25}},
    "feature_networks": [{"type": "ConcatenateCondition", "kwargs": {"input_size": None, "output_size": 3}},
                         {"type": "DualDomainLSTM", "kwargs": L2}],
}


def _import_reference():
    if not REF_SRC or not os.path.isdir(REF_SRC):
        raise SystemExit("usage: make_golden_dlstm.py path/to/reference/src (or set BCNF_REFERENCE_SRC)")
    stub = tempfile.mkdtemp(prefix="bcnf_stub_")
    os.makedirs(os.path.join(stub, "dynaconf"))
    with open(os.path.join(stub, "dynaconf", "__init__.py"), "w") as f:
        f.write("class Dynaconf:\n    def __init__(self, *a, **k):\n        raise RuntimeError('stub')\n")
    sys.dont_write_bytecode = True
    sys.path[:0] = [stub, REF_SRC]
    import bcnf.models.cnf as cnf  # noqa
    import bcnf.models.feature_network as fnet  # noqa
    import bcnf.utils as utils  # noqa
    return cnf, fnet, utils


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
        elif len(shape) == 2:
            a = rng.uniform(-1.0, 1.0, size=shape) / np.sqrt(shape[1])
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


def run_network(net, traj, w):
    net.zero_grad()
    h = net(traj)
    out = {"h": h.detach().numpy().copy()}
    (h * w).sum().backward()
    out.update({"grad/" + n: p.grad.detach().numpy().copy() for n, p in net.named_parameters()})
    return out


def network_case(name, net, trajs, w):
    """trajs: {suffix: trajectories}; the first entry's results are stored as name/*, the others as name<suffix>/*."""
    net.eval()
    sd = proxy_state(net, 16)
    net.load_state_dict({k: torch.from_numpy(v) for k, v in sd.items()})
    net64 = copy.deepcopy(net).double()
    arrays = {f"{name}/sd/{k}": v for k, v in sd.items()}
    arrays[f"{name}/w"] = w.numpy()
    for suffix, traj in trajs.items():
        got = run_network(net, traj, w)
        ref = run_network(net64, traj.double(), w.double())
        fv = quarter_gate(f"{name}{suffix}/h", got["h"], ref["h"], 1e-5, 1e-5)
        fg = max(quarter_gate(f"{name}{suffix}/{k}", got[k], ref[k], 1e-4, 1e-4) for k in got if k.startswith("grad/"))
        print(f"case {name}{suffix}: value gate used {fv:.3f}, gradient gate used {fg:.3f}")
        arrays.update({f"{name}{suffix}/{k}": v for k, v in got.items()})
        arrays[f"{name}{suffix}/traj"] = traj.numpy()
    return arrays


def run_model(model, utils, y, traj):
    model.zero_grad()
    z, h = model.forward(y, traj, log_det_J=True, return_features=True)
    ldj = model.log_det_J
    nll = utils.inn_nll_loss(z, ldj)
    nll.backward()
    out = {"h": h.detach().numpy().copy(), "z": z.detach().numpy().copy(), "ldj": ldj.detach().numpy().copy(),
           "nll": np.asarray(nll.item())}
    out.update({"grad/" + n: p.grad.detach().numpy().copy() for n, p in model.named_parameters()
                if p.grad is not None})
    with torch.no_grad():
        out["inv"] = model.inverse(z.detach(), traj).numpy().copy()
    return out


def model_case(cnf, utils, y, traj):
    torch.manual_seed(2024_03_25)
    model = cnf.CondRealNVP_v2.from_config(MODEL_CFG)
    model.eval()
    sd = proxy_state(model, 17)
    model.load_state_dict({k: torch.from_numpy(v) for k, v in sd.items()})
    m64 = copy.deepcopy(model).double()
    m64.log_det_J = m64.log_det_J.double()
    got = run_model(model, utils, y, traj)
    ref = run_model(m64, utils, y.double(), traj.double())
    fv = max(quarter_gate(f"m/{k}", got[k], ref[k], 1e-5, 1e-5) for k in ("h", "z", "ldj", "inv"))
    fg = max(quarter_gate(f"m/{k}", got[k], ref[k], 1e-4, 1e-4) for k in got if k.startswith("grad/"))
    print(f"case m: nll {float(got['nll']):.5f}, value gate used {fv:.3f}, gradient gate used {fg:.3f}")
    out = {"sd/" + k: v for k, v in sd.items()}
    got["nll"] = np.float32(got["nll"])
    out.update(got, y=y.numpy(), traj=traj.numpy())
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
    cnf, fnet, utils = _import_reference()
    rng = np.random.Generator(np.random.PCG64(7))
    unit = torch.from_numpy(rng.standard_normal((B, 30, 3)).astype(np.float32))
    y = torch.from_numpy(rng.standard_normal((B, 21)).astype(np.float32))
    w32 = torch.from_numpy(rng.standard_normal((B, 32)).astype(np.float32))
    w16 = torch.from_numpy(rng.standard_normal((B, 16)).astype(np.float32))
    arrays = {}
    torch.manual_seed(2024_03_25)
    arrays.update(network_case("l1", fnet.DualDomainLSTM(**L1), {"": 5.0 * unit}, w32))
    arrays.update(network_case("l2", fnet.DualDomainLSTM(**L2), {"": unit, "x5": 5.0 * unit}, w16))
    arrays.update(network_case("l3", fnet.DualDomainLSTM(**L3), {"": 5.0 * unit}, w16))
    arrays.update(model_case(cnf, utils, y, 5.0 * unit))
    # every committed file stays under 1 MiB: the weights and gradients of l3 and of m go to files of their own
    parts = {"g17_dlstm.npz": ("l1", "l2", "l2x5"), "g17_dlstm_l3.npz": ("l3",), "g17_dlstm_m.npz": ("m",)}
    for fname, cases in parts.items():
        path = os.path.join(OUT, fname)
        write_npz(path, {k: v for k, v in arrays.items() if k.split("/")[0] in cases})
        size = os.path.getsize(path)
        print(f"{path}: {size} bytes")
        if size > 1000_000:
            raise SystemExit(f"{fname} is over 1 MB")


if __name__ == "__main__":
    main()
