"""The literal training loop the Trainer tests compare against: Trainer._train (reference trainer.py:156-240) written
out batch by batch -- one eager `TrainStep(capture=False)` step per training batch with the lr edited through
`param_groups`, `_validate_batch` (trainer.py:279-303) in torch ops with its three `.item()` per batch -- plus the
models and configs of tests/golden/make_golden_trainer.py. GPU only where a model is run."""
import math
import time

import numpy as np
import torch

from conftest import golden_sd

NAMES = ['x0_x', 'x0_y', 'x0_z', 'v0_x', 'v0_y', 'v0_z', 'g', 'w_x', 'w_y', 'w_z', 'b', 'm', 'a_x', 'a_y', 'a_z', 'r',
         'A', 'Cd', 'rho', 'p19', 'p20']
BATCH, SPLIT = 48, 0.4


def model_config(hybrid=False, dropout=0.0, D=19, nested=(16,) * 7, C=80, n_blocks=4):
    return {
        "global": {"parameter_selection": NAMES[:D]},
        "model": {"kwargs": {"size": D, "nested_sizes": list(nested), "n_conditions": C, "n_blocks": n_blocks,
                             "dropout": dropout, "act_norm": True, "hybrid": hybrid, "random_state": 2024_03_25}},
        "feature_networks": [
            {"type": "ConcatenateCondition", "kwargs": {"input_size": None, "output_size": 90}},
            {"type": "FullyConnected", "kwargs": {"sizes": [90, C]}},
        ],
    }


def golden_model(g, run, dropout=0.0, seed=77, device="cuda"):
    """The golden run's model at its initial weights. The golden model has dropout 0, hence no nn.Dropout modules in
    its nested Sequentials; with dropout > 0 the same tensors sit under other indices, so they are carried over in
    state_dict order."""
    from bcnf_amd import CondRealNVP_v2
    m = CondRealNVP_v2.from_config(model_config(hybrid=(run == "ii"), dropout=0.0))
    m.load_state_dict(golden_sd(g, prefix=f"{run}/sd/"))
    if dropout > 0.0:
        md = CondRealNVP_v2.from_config(model_config(hybrid=(run == "ii"), dropout=dropout))
        src, dst = m.state_dict(), md.state_dict()
        assert [tuple(v.shape) for v in src.values()] == [tuple(v.shape) for v in dst.values()]
        md.load_state_dict(dict(zip(dst.keys(), src.values())))
        m = md
    m.to(device)
    if device != "cpu":
        m.fused.set_seed(seed)
    return m


def golden_data(g):
    y = torch.from_numpy(np.ascontiguousarray(g["y"])).cuda()
    cond = torch.from_numpy(np.ascontiguousarray(g["cond"])).cuda()
    return y, cond


def train_config(n_epochs, lr, sched_kwargs=None, timeout=None, patience=4):
    return {"global": {"conditions": [["trajectories"]]},
            "training": {"val_loss_window_size": 2, "val_loss_patience": patience, "val_loss_tolerance_mode": "abs",
                         "val_loss_tolerance": 0.1, "n_epochs": n_epochs, "validation_split": SPLIT,
                         "batch_size": BATCH, "timeout": timeout, "verbose": False},
            "optimizer": {"type": "Adam", "kwargs": {"lr": lr}},
            "lr_scheduler": {"type": "ReduceLROnPlateau",
                             "kwargs": dict(sched_kwargs or dict(patience=1, factor=0.5, threshold_mode="abs"))}}


def validate_torch(model, y, cond, batch, w):
    """The validation loop of _train in torch ops: ((loss, nll, mse) epoch means, z_mean, z_std, mean(log_det_J)) with
    the last three from the last batch."""
    from bcnf_amd.utils import inn_nll_loss
    was = model.training
    model.eval()
    sums, nb = [0.0, 0.0, 0.0], 0
    with torch.no_grad():
        for lo in range(0, y.shape[0], batch):
            yb, cb = y[lo:lo + batch], cond[lo:lo + batch]
            z, h = model.forward(yb, cb, log_det_J=True, return_features=True)
            mse = torch.nn.functional.mse_loss(model.prediction_head(h), yb) if w > 0 else torch.tensor(0.0)
            nll = inn_nll_loss(z, model.log_det_J)
            loss = (nll + mse.to(nll.device) * w) / (1 + w)
            for i, v in enumerate((loss.item(), nll.item(), mse.item())):
                sums[i] += v
            nb += 1
            z_mean, z_std = z.mean(dim=0), z.std(dim=0)
        ldj = model.log_det_J.mean().item()
    model.train(was)
    return tuple(s / nb for s in sums), z_mean, z_std, ldj


def literal_loop(model, config, y, cond, order_fn, w, start_epoch=0):
    """-> (handler, per-epoch training triples, per-epoch validation values, the eager TrainStep)."""
    from bcnf_amd.errors import TrainingDivergedError
    from bcnf_amd.train import TrainStep
    from bcnf_amd.trainer import (TrainerParameterHistoryHandler, epoch_end, make_scheduler, split_sizes,
                                  z_statistics)
    tr = config["training"]
    n_train, _ = split_sizes(y.shape[0], tr["validation_split"])
    batch = tr["batch_size"]
    ts = TrainStep(model, lr=config["optimizer"]["kwargs"]["lr"], hybrid_weight=w, capture=False)
    ts.set_pool(y[:n_train].contiguous(), cond[:n_train].contiguous())
    scheduler = make_scheduler(config, ts.opt)
    yv, cv = y[n_train:].contiguous(), cond[n_train:].contiguous()
    h = TrainerParameterHistoryHandler(tr["val_loss_window_size"], tr["val_loss_patience"],
                                       tr["val_loss_tolerance_mode"], tr["val_loss_tolerance"], fold=-1)
    trains, vals = [], []
    start = time.time()
    for epoch in range(start_epoch, tr["n_epochs"]):
        h.update_epoch(epoch)
        model.train()
        order = torch.as_tensor(order_fn(epoch, n_train)).cuda()
        sums, nb = [0.0, 0.0, 0.0], 0
        for lo in range(0, n_train, batch):
            v = ts.step_indexed(order[lo:lo + batch])
            if (v[0] > 1e5 or math.isnan(v[0])) and epoch > 10:
                raise TrainingDivergedError(f"Loss exploded to {v[0]}")
            for i in range(3):
                sums[i] += v[i]
            nb += 1
        train = tuple(s / nb for s in sums)
        val, z_mean, z_std, ldj = validate_torch(model, yv, cv, batch, w)
        trains.append(train)
        vals.append(val + z_statistics(z_mean, z_std, ldj))
        if epoch_end(h, epoch, train, val, z_statistics(z_mean, z_std, ldj), ts.opt, scheduler, tr["timeout"],
                     start) is not None:
            return h, trains, vals, ts
    h.parameter_history["stop_reason"] = "max_epochs"
    return h, trains, vals, ts


def bits_equal(a, b):
    """Bit-for-bit equality of two fp32 tensors (NaNs included)."""
    return a.shape == b.shape and torch.equal(a.detach().contiguous().view(torch.int32),
                                              b.detach().contiguous().view(torch.int32))
