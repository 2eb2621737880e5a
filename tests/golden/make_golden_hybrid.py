"""Generate g15_hybrid.npz by running the REFERENCE (psaegert/bcnf @ /root/reference) on CPU: the hybrid training
loss of Trainer._train_batch (trainer.py:261-269), loss = (nll + w * MSE(prediction_head(h), y)) / (1 + w).

Test infrastructure only, run in the build container like make_golden.py (same dynaconf stub, nothing of the
reference is copied, only inputs / outputs):

    python tests/golden/make_golden_hybrid.py

Three cases (keys "<case>/..."), each: torch.manual_seed(20240325), CondRealNVP_v2.from_config with dropout 0.5,
act_norm, hybrid=True, random_state 20240325 and the first D names of the hybrid run configs' parameter_selection,
eval mode, inputs from torch.Generator().manual_seed(7): y = randn(B, D), then traj = 2 * randn(B, X / 3, 3).

  case  D   nested   nb  C   FullyConnected    B   w     covers
  a     21  [32]x3   4   32  [60, 56, 56, 32]  50  1.0   wide family, two N tiles (11-column tail), row tail 50 = 3*16 + 2
  b     19  [32]x2   3   37  [90, 37]          17  0.1   K = 37 (not a multiple of 4), wide fold bypassed, w != 1
  c     19  [16]x7   4   80  [90, 80]          48  1.0   small family, single-Linear fold bypassed

Stored per case: y, traj, w, sd/*, h, z, ldj, y_hat, loss, nll, mse, dh, grad/* of every parameter
(prediction_head.* included), and after/* + clip_total_norm from one Adam(lr=2e-4).step() followed by
clip_grad_norm_(1.0). The archive is written with fixed zip timestamps, so a rerun reproduces it byte for byte.
"""
import io
import os
import sys
import tempfile
import zipfile

import numpy as np
import torch

REF_SRC = "/root/reference/src"
OUT = os.path.dirname(os.path.abspath(__file__))
SEED = 2024_03_25
NAMES = ['x0_x', 'x0_y', 'x0_z', 'v0_x', 'v0_y', 'v0_z', 'g_x', 'g_y', 'g_z', 'w_x', 'w_y', 'w_z', 'b', 'm',
         'a_x', 'a_y', 'a_z', 'r', 'A', 'Cd', 'rho']

CASES = {
    "a": dict(D=21, nested=[32] * 3, nb=4, C=32, fc=[60, 56, 56, 32], B=50, w=1.0),
    "b": dict(D=19, nested=[32] * 2, nb=3, C=37, fc=[90, 37], B=17, w=0.1),
    "c": dict(D=19, nested=[16] * 7, nb=4, C=80, fc=[90, 80], B=48, w=1.0),
}


def case_config(c):
    return {
        "global": {"parameter_selection": NAMES[:c["D"]]},
        "model": {"kwargs": {"size": c["D"], "nested_sizes": list(c["nested"]), "n_conditions": c["C"],
                             "n_blocks": c["nb"], "dropout": 0.5, "act_norm": True, "hybrid": True,
                             "random_state": SEED}},
        "feature_networks": [
            {"type": "ConcatenateCondition", "kwargs": {"input_size": None, "output_size": c["fc"][0]}},
            {"type": "FullyConnected", "kwargs": {"sizes": list(c["fc"])}},
        ],
    }


def _import_reference():
    stub = tempfile.mkdtemp(prefix="bcnf_stub_")
    os.makedirs(os.path.join(stub, "dynaconf"))
    with open(os.path.join(stub, "dynaconf", "__init__.py"), "w") as f:
        f.write("class Dynaconf:\n    def __init__(self, *a, **k):\n        raise RuntimeError('stub')\n")
    sys.dont_write_bytecode = True
    sys.path[:0] = [stub, REF_SRC]
    import bcnf.models.cnf as cnf  # noqa
    import bcnf.utils as utils  # noqa
    return cnf, utils


def make_case(cnf, utils, name, c):
    torch.manual_seed(SEED)
    model = cnf.CondRealNVP_v2.from_config(case_config(c))
    model.eval()
    out = {"sd/" + k: v.detach().numpy().copy() for k, v in model.state_dict().items()}
    gen = torch.Generator().manual_seed(7)
    y = torch.randn(c["B"], c["D"], generator=gen)
    traj = 2.0 * torch.randn(c["B"], c["fc"][0] // 3, 3, generator=gen)
    w = c["w"]
    model.zero_grad()
    z, h = model.forward(y, traj, log_det_J=True, return_features=True)
    h.retain_grad()
    y_hat = model.prediction_head(h)
    mse = torch.nn.MSELoss()(y_hat, y)
    nll = utils.inn_nll_loss(z, model.log_det_J)
    loss = (nll + mse * w) / (1 + w)
    loss.backward()
    out.update(y=y.numpy(), traj=traj.numpy(), w=np.float32(w), h=h.detach().numpy(), z=z.detach().numpy(),
               ldj=model.log_det_J.detach().numpy().copy(), y_hat=y_hat.detach().numpy(),
               loss=np.float32(loss.item()), nll=np.float32(nll.item()), mse=np.float32(mse.item()),
               dh=h.grad.detach().numpy().copy())
    out.update({"grad/" + n: p.grad.detach().numpy().copy() for n, p in model.named_parameters()
                if p.grad is not None})
    opt = torch.optim.Adam(model.parameters(), lr=2e-4)
    opt.step()
    total_norm = torch.nn.utils.clip_grad_norm_(model.parameters(), max_norm=1.0)
    out.update({"after/" + n: p.detach().numpy().copy() for n, p in model.named_parameters()})
    out["clip_total_norm"] = np.float32(total_norm.item())
    print(f"case {name}: loss {loss.item():.5f} nll {nll.item():.5f} mse {mse.item():.6f}")
    return {f"{name}/{k}": v for k, v in out.items()}


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
    cnf, utils = _import_reference()
    arrays = {}
    for name, c in CASES.items():
        arrays.update(make_case(cnf, utils, name, c))
    write_npz(os.path.join(OUT, "g15_hybrid.npz"), arrays)


if __name__ == "__main__":
    main()
