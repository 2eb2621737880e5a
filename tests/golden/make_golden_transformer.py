"""Generate g16_transformer.npz by running the REFERENCE (psaegert/bcnf) on CPU: the Transformer and
DualDomainTransformer feature networks (feature_network.py:183-307, 401-471), standalone and under a coupling stack.

Test infrastructure only, run like make_golden_hybrid.py (same dynaconf stub; nothing of the reference is copied, only
inputs / outputs). The reference checkout's src directory is the first argument, or $BCNF_REFERENCE_SRC:

    python tests/golden/make_golden_transformer.py path/to/reference/src

Weights: numpy PCG64(seed) in state_dict order as make_golden.py's large_proxy_state (2-D: U(-1, 1) / sqrt(fan_in),
1-D: U(-0.05, 0.05), ActNorm scales and LayerNorm weights: U(0.7, 1.3); the orthonormal matrices are kept). Inputs:
numpy PCG64(7). Every network is in eval mode, B = 12, trajectories (12, 30, 3).

  case  network                                                                    trajectories  stored
  t1    Transformer(3, 32, 4, 32, 2, 16, add_positional_embeddings=True)           5 N(0, 1)     h, w, grad/* of sum(h w)
  t2    Transformer(3, 100, 4, 32, 1, 16)  (head_dim 25, no positional table)      5 N(0, 1)     h
  d1    DualDomainTransformer(3, 32, 4, 32, 2, [16], add_positional_embeddings=True)  N(0, 1)    h, w, grad/* of sum(h w)
  m     CondRealNVP_v2(size=21, nested_sizes=[32]*3, n_conditions=16, n_blocks=3, act_norm=True, dropout=0.5) on
        ConcatenateCondition(None, 3) + the t1 Transformer                          5 N(0, 1)     h, z, ldj, inv =
        inverse(z), nll, grad/* of the eval NLL

(d1 at unit scale: at 5 N(0, 1) the reference's own fp32 gradients of the frequency branch miss the 1e-4 gradient gate
against its float64 run.) Each case also runs in float64, and the generator stops unless the reference's fp32 values
lie within a quarter of the value gate close(rtol=1e-5, floor=1e-5) of tests/conftest.py and its fp32 gradients within a
quarter of the gradient gate close(rtol=1e-4, floor=1e-4): the fixture then leaves three quarters of each gate to the
code under test. Fixed zip timestamps: a rerun reproduces the archive byte for byte.
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
T1 = dict(input_size=3, trf_size=32, n_heads=4, ff_size=32, n_blocks=2, output_size=16,
          add_positional_embeddings=True)
T2 = dict(input_size=3, trf_size=100, n_heads=4, ff_size=32, n_blocks=1, output_size=16,
          add_positional_embeddings=False)
D1 = dict(input_size=3, trf_size=32, n_heads=4, ff_size=32, n_blocks=2, fc_sizes=[16],
          add_positional_embeddings=True)
MODEL_CFG = {
    "global": {"parameter_selection": NAMES},
    "model": {"kwargs": {"size": 21, "nested_sizes": [32] * 3, "n_conditions": 16, "n_blocks": 3, "act_norm": True,
                         "dropout": 0.5, "random_state": 2024_03_25}},
    "feature_networks": [{"type": "ConcatenateCondition", "kwargs": {"input_size": None, "output_size": 3}},
                         {"type": "Transformer", "kwargs": T1}],
}


def _import_reference():
    if not REF_SRC or not os.path.isdir(REF_SRC):
        raise SystemExit("usage: make_golden_transformer.py path/to/reference/src (or set BCNF_REFERENCE_SRC)")
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
        if k.endswith(".scale") or k.endswith(("norm1.weight", "norm2.weight")):
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
    if w is not None:
        (h * w).sum().backward()
        out.update({"grad/" + n: p.grad.detach().numpy().copy() for n, p in net.named_parameters()})
    return out


def network_case(name, net, traj, w):
    net.eval()
    sd = proxy_state(net, 16)
    net.load_state_dict({k: torch.from_numpy(v) for k, v in sd.items()})
    net64 = copy.deepcopy(net).double()
    got = run_network(net, traj, w)
    ref = run_network(net64, traj.double(), None if w is None else w.double())
    fv = quarter_gate(f"{name}/h", got["h"], ref["h"], 1e-5, 1e-5)
    fg = max([quarter_gate(f"{name}/{k}", got[k], ref[k], 1e-4, 1e-4) for k in got if k.startswith("grad/")] or [0.0])
    print(f"case {name}: value gate used {fv:.3f}, gradient gate used {fg:.3f}")
    out = {"sd/" + k: v for k, v in sd.items()}
    out.update(got, traj=traj.numpy())
    if w is not None:
        out["w"] = w.numpy()
    return {f"{name}/{k}": v for k, v in out.items()}


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
    w = torch.from_numpy(rng.standard_normal((B, 16)).astype(np.float32))
    arrays = {}
    torch.manual_seed(2024_03_25)
    arrays.update(network_case("t1", fnet.Transformer(**T1), 5.0 * unit, w))
    arrays.update(network_case("t2", fnet.Transformer(**T2), 5.0 * unit, None))
    arrays.update(network_case("d1", fnet.DualDomainTransformer(**D1), unit, w))
    arrays.update(model_case(cnf, utils, y, 5.0 * unit))
    path = os.path.join(OUT, "g16_transformer.npz")
    write_npz(path, arrays)
    print(f"{path}: {os.path.getsize(path)} bytes")


if __name__ == "__main__":
    main()
