"""Generate g21_trainer.npz by running the REFERENCE's training loop (psaegert/bcnf @ /root/reference,
src/bcnf/train/trainer.py Trainer._train with trainer_loss_handler.py) on CPU.

Test infrastructure only, run in the build container like make_golden_hybrid.py (stub `wandb`, `torchsummary` and
`dynaconf` modules; nothing of the reference is copied, only inputs / outputs):

    python tests/golden/make_golden_trainer.py

The Trainer is built with object.__new__ (its __init__ loads data sets) and `_train` is called with DataLoaders over
explicit `batch_sampler`s, so the batch order of every epoch is RECORDED (orders[e] = a numpy PCG64 permutation of the
121 training samples, cut into batches of 48, 48, 25), not drawn from torch's global RNG. The validation loader walks
the 79 validation samples in order (48 + 31).

Model (dropout 0): D = 19, nested [16] x 7, 4 blocks, C = 80, ConcatenateCondition -> FullyConnected [90, 80],
act_norm, random_state 20240325; n = 200 samples from torch.Generator().manual_seed(7): y = randn(200, 19),
cond = 2 * randn(200, 30, 3); validation_split 0.4 -> int(1 - 0.4 * 200) = -79: 121 training, 79 validation samples.

  run i   hybrid_weight 0, Adam(lr = LR_I), ReduceLROnPlateau(patience=1, factor=0.5, threshold_mode="abs"),
          val_loss_window_size 2, val_loss_patience 4, tolerance abs 0.1, n_epochs 40. The maker asserts at least one
          lr reduction and stop_reason == "val_loss_plateau".
  run ii  hybrid model, hybrid_weight 1, Adam(lr = 2e-4), same scheduler, n_epochs 3 -> "max_epochs".

Stored per run ("<run>/..."): sd/* (initial state_dict), hist/<key> = the full parameter_history entry as an (entries,
2) float64 array of (epoch + 1, value) -- the per-epoch train and validation triples, lr, distance, time, the
z_mean / z_std / log_det_J statistics, first entry duplicated as the reference stores it --, stop_reason,
best_val_epoch, best_val_loss, n_epochs_run, lr0, w, and val0/* = one validation pass of the reference's
_validate_batch over the validation loader at the INITIAL weights (loss, nll, mse means; z_mean, z_std and
mean(log_det_J) of the last batch). Shared: y, cond, orders. Fixed zip timestamps: a rerun reproduces the bytes
(`time` excepted).
"""
import io
import os
import sys
import tempfile
import types
import zipfile

import numpy as np
import torch

REF_SRC = "/root/reference/src"
OUT = os.path.dirname(os.path.abspath(__file__))
SEED = 2024_03_25
NAMES = ['x0_x', 'x0_y', 'x0_z', 'v0_x', 'v0_y', 'v0_z', 'g', 'w_x', 'w_y', 'w_z', 'b', 'm', 'a_x', 'a_y', 'a_z', 'r',
         'A', 'Cd', 'rho']
N, SPLIT, BATCH = 200, 0.4, 48
LR_I = 2e-2
MAX_EPOCHS_I = 40


def model_config(hybrid):
    return {
        "global": {"parameter_selection": NAMES},
        "model": {"kwargs": {"size": 19, "nested_sizes": [16] * 7, "n_conditions": 80, "n_blocks": 4, "dropout": 0.0,
                             "act_norm": True, "hybrid": hybrid, "random_state": SEED}},
        "feature_networks": [
            {"type": "ConcatenateCondition", "kwargs": {"input_size": None, "output_size": 90}},
            {"type": "FullyConnected", "kwargs": {"sizes": [90, 80]}},
        ],
    }


def training_config(n_epochs):
    return {"training": {"val_loss_window_size": 2, "val_loss_patience": 4, "val_loss_tolerance_mode": "abs",
                         "val_loss_tolerance": 0.1, "n_epochs": n_epochs, "verbose": False, "timeout": None,
                         "validation_split": SPLIT, "batch_size": BATCH}}


def _import_reference():
    stub = tempfile.mkdtemp(prefix="bcnf_stub_")
    os.makedirs(os.path.join(stub, "dynaconf"))
    with open(os.path.join(stub, "dynaconf", "__init__.py"), "w") as f:
        f.write("class Dynaconf:\n    def __init__(self, *a, **k):\n        raise RuntimeError('stub')\n")
    wandb = types.ModuleType("wandb")
    wandb.log = lambda *a, **k: None
    wandb.init = lambda *a, **k: None
    wandb.config = {}
    sys.modules["wandb"] = wandb
    ts = types.ModuleType("torchsummary")
    ts.summary = lambda *a, **k: None
    sys.modules["torchsummary"] = ts
    sys.dont_write_bytecode = True
    sys.path[:0] = [stub, REF_SRC]
    import bcnf.models.cnf as cnf  # noqa
    import bcnf.train.trainer as trainer  # noqa
    return cnf, trainer


class RecordedBatches:
    """A batch_sampler whose e-th iteration yields orders[e] cut into batches (the last one ragged)."""

    def __init__(self, orders, batch):
        self.orders, self.batch, self.epoch = orders, batch, 0

    def __len__(self):
        return -(-self.orders.shape[1] // self.batch)

    def __iter__(self):
        o = self.orders[self.epoch].tolist()
        self.epoch += 1
        for i in range(0, len(o), self.batch):
            yield o[i:i + self.batch]


def validate_initial(tr, model, val_loader):
    model.eval()
    sums = np.zeros(3)
    with torch.no_grad():
        for y, *conditions in val_loader:
            loss, nll, mse, z_mean, z_std = tr._validate_batch(y, *conditions, model=model,
                                                               loss_function=tr.loss_function)
            sums += (loss, nll, mse)
    sums /= len(val_loader)
    return {"val0/loss": sums[0], "val0/nll": sums[1], "val0/mse": sums[2], "val0/z_mean": z_mean.numpy().copy(),
            "val0/z_std": z_std.numpy().copy(), "val0/ldj_mean": np.float64(model.log_det_J.mean().item())}


def make_run(cnf, trainer, name, y, cond, orders, hybrid, w, lr, n_epochs):
    from torch.utils.data import DataLoader, Subset, TensorDataset
    from bcnf.utils import inn_nll_loss
    torch.manual_seed(SEED)
    model = cnf.CondRealNVP_v2.from_config(model_config(hybrid))
    out = {"sd/" + k: v.detach().numpy().copy() for k, v in model.state_dict().items()}
    tr = object.__new__(trainer.Trainer)
    tr.config = training_config(n_epochs)
    tr.hybrid_weight = w
    tr.mse_loss = torch.nn.MSELoss()
    tr.loss_function = inn_nll_loss
    dataset = TensorDataset(y, cond)
    train_size = int(1 - SPLIT * len(dataset))
    idx = list(range(len(dataset)))
    train_set, val_set = Subset(dataset, idx[:train_size]), Subset(dataset, idx[train_size:])
    assert (len(train_set), len(val_set)) == (121, 79) and orders.shape[1] == 121
    train_loader = DataLoader(train_set, batch_sampler=RecordedBatches(orders, BATCH))
    n_val = len(val_set)
    val_batches = [list(range(i, min(i + BATCH, n_val))) for i in range(0, n_val, BATCH)]
    val_loader = DataLoader(val_set, batch_sampler=val_batches)
    out.update(validate_initial(tr, model, val_loader))
    optimizer = torch.optim.Adam(model.parameters(), lr=lr)
    scheduler = torch.optim.lr_scheduler.ReduceLROnPlateau(optimizer, patience=1, factor=0.5, threshold_mode="abs")
    tr._train(model, train_loader, val_loader, tr.loss_function, optimizer, scheduler)
    h = tr.meta_scheduler
    hist = h.parameter_history
    for k, v in hist.items():
        if k != "stop_reason":
            out["hist/" + k] = np.array(v, dtype=np.float64)
    out.update(stop_reason=np.array(hist["stop_reason"]), best_val_epoch=np.int64(h.best_val_epoch),
               best_val_loss=np.float64(h.best_val_loss), n_epochs_run=np.int64(len(hist["lr"]) - 1),
               lr0=np.float64(lr), w=np.float64(w), n_epochs=np.int64(n_epochs))
    lrs = [v for _, v in hist["lr"]]
    print(f"run {name}: {len(lrs) - 1} epochs, stop {hist['stop_reason']}, lr {lrs[0]} -> {lrs[-1]}, "
          f"best {h.best_val_loss:.5f} @ {h.best_val_epoch}, val {[round(v, 4) for _, v in hist['val_loss'][1:]]}")
    return {f"{name}/{k}": v for k, v in out.items()}, hist


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
    cnf, trainer = _import_reference()
    gen = torch.Generator().manual_seed(7)
    y = torch.randn(N, 19, generator=gen)
    cond = 2.0 * torch.randn(N, 30, 3, generator=gen)
    rng = np.random.Generator(np.random.PCG64(SEED))
    orders = np.stack([rng.permutation(121) for _ in range(MAX_EPOCHS_I)]).astype(np.int64)
    arrays = {"y": y.numpy(), "cond": cond.numpy(), "orders": orders}
    run_i, hist_i = make_run(cnf, trainer, "i", y, cond, orders, False, 0.0, LR_I, MAX_EPOCHS_I)
    lrs = [v for _, v in hist_i["lr"]]
    assert min(lrs) < lrs[0], "run i shows no lr reduction"
    assert hist_i["stop_reason"] == "val_loss_plateau", hist_i["stop_reason"]
    run_ii, hist_ii = make_run(cnf, trainer, "ii", y, cond, orders, True, 1.0, 2e-4, 3)
    assert hist_ii["stop_reason"] == "max_epochs"
    arrays.update(run_i)
    arrays.update(run_ii)
    write_npz(os.path.join(OUT, "g21_trainer.npz"), arrays)


if __name__ == "__main__":
    main()
