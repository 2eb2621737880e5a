"""`bcnf.train.Trainer` (src/bcnf/train/trainer.py) on the device: the loop that ties `TrainStep.run_epoch`, the
validation epoch (`bcnf_amd.validate.ValidationPass`), the parameter history, the lr scheduler and the three stops
into a training run.

An epoch of `Trainer.train` is an epoch of the reference's `_train` (trainer.py:156-240):

    training batches          TrainStep.run_epoch (whole batches, one host sync) + step_indexed (ragged remainder)
    validation batches        ValidationPass.run (captured multi-batch graphs, one host sync)
    rolling validation loss   TrainerParameterHistoryHandler.update_rolling_validation_loss
    the 14 logged keys        TrainerParameterHistoryHandler.log
    scheduler                 ReduceLROnPlateau.step(rolling average) / step(); a changed lr -> TrainStep.set_lr
    best loss, stops          update_best_loss; val_loss_plateau (>=), timeout, max_epochs

Everything after the two device passes is `epoch_end`, a host function that needs no GPU.

Differences a user meets:
* the data live on the device as one training pool and one validation pool (the reference's split rule,
  `split_sizes`); batches are pool indices, not DataLoader tuples;
* the reference's DataLoader shuffles with the process-global torch RNG, which no other loop can follow. The epoch
  order here is `order_fn(epoch, n_train)` -> a permutation of range(n_train) (or any index tensor of that length);
  the default is `torch.randperm(n_train, generator=g)` with ONE generator `g` seeded from
  `config["training"]["random_state"]` (default 2024_03_25) when `train` starts, so a run is reproducible from its
  config. The validation pool is walked in order: no validation value but the last batch's statistics depends on
  the loader's shuffle;
* `wandb` is replaced by an optional `log_fn(values: dict, step: int)` callback.
"""
from __future__ import annotations

import datetime
import math
import time
from collections import deque
from typing import Any, Callable

import torch

from bcnf_amd.errors import TrainingDivergedError
from bcnf_amd.validate import ONE_CONDITION, require_one_condition

DEFAULT_RANDOM_STATE = 2024_03_25


class TrainerParameterHistoryHandler:
    """The reference's epoch bookkeeping (src/bcnf/train/trainer_loss_handler.py), names and quirks kept: `log` stores
    a parameter's first value twice, `update_best_loss` moves the best only when a patience is set, the tolerance
    modes are 'rel' and 'abs', and the rolling average is the mean of a deque of `val_loss_window_size` losses."""

    def __init__(self, val_loss_window_size: int, val_loss_patience: int | None = None,
                 val_loss_tolerance_mode: str = "abs", val_loss_tolerance: float = 1e-1, fold: int = 1,
                 log_fn: Callable[[dict, int], None] | None = None) -> None:
        if val_loss_tolerance_mode not in ("rel", "abs"):
            raise ValueError("val_loss_tolerance_mode must be either 'rel' or 'abs'")
        self.val_loss_tolerance_mode = val_loss_tolerance_mode
        self.best_val_loss = float("inf")
        self.best_val_epoch = 0
        self.val_losses: deque = deque(maxlen=val_loss_window_size)
        self.val_loss_rolling_avg: float
        self.val_loss_window_size = val_loss_window_size
        self.val_loss_patience = val_loss_patience
        self.val_loss_tolerance = val_loss_tolerance
        self.parameter_history: dict[str, Any] = {}
        self.epoch = 0
        self.fold = fold
        self.log_fn = log_fn

    def update_epoch(self, epoch: int) -> None:
        self.epoch = epoch

    def log(self, parameter: str, value: Any) -> None:
        entry = (self.epoch + 1, value)
        if parameter not in self.parameter_history:
            self.parameter_history[parameter] = [entry]         # ... and appended again below: the first value twice
        self.parameter_history[parameter].append(entry)
        if self.log_fn is not None:
            self.log_fn({"epoch": self.epoch + 1, f"{parameter}_fold_{self.fold}": value}, self.epoch)

    def update_rolling_validation_loss(self, val_loss: float) -> None:
        if len(self.val_losses) >= self.val_loss_window_size:
            self.val_losses.popleft()
        self.val_losses.append(val_loss)
        self.val_loss_rolling_avg = sum(self.val_losses) / len(self.val_losses)

    def update_best_loss(self) -> None:
        if self.val_loss_patience is None or self.val_loss_rolling_avg is None:
            return
        if self.val_loss_tolerance_mode == "rel":
            bar = self.best_val_loss * (1 - self.val_loss_tolerance)
        else:
            bar = self.best_val_loss - self.val_loss_tolerance
        if self.val_loss_rolling_avg < bar:
            self.best_val_loss = self.val_loss_rolling_avg
            self.best_val_epoch = self.epoch


def split_sizes(n: int, split_ratio: float) -> tuple[int, int]:
    """(training samples, validation samples) of TrainerDataHandler.split_dataset (trainer_data_handler.py:195-203),
    arithmetic included: train_size = int(1 - split_ratio * n) is NEGATIVE for any real split, and the two sets are
    indices[:train_size] and indices[train_size:] -- the last int(split_ratio * n - 1) samples validate."""
    train_size = int(1 - split_ratio * n)
    idx = range(n)
    return len(idx[:train_size]), len(idx[train_size:])


def default_order_fn(random_state: int | None = None):
    """order_fn(epoch, n_train) = torch.randperm(n_train, generator=g), g seeded once from random_state."""
    g = torch.Generator()
    g.manual_seed(DEFAULT_RANDOM_STATE if random_state is None else int(random_state))

    def order_fn(epoch: int, n_train: int):
        return torch.randperm(n_train, generator=g)
    return order_fn


def z_statistics(z_mean, z_std, log_det_J_mean: float):
    """The five scalars _train logs from the last validation batch (trainer.py:213-217), as fp32 torch reductions."""
    zm = torch.as_tensor(z_mean, dtype=torch.float32).cpu()
    zs = torch.as_tensor(z_std, dtype=torch.float32).cpu()
    return (zm.mean().item(), zm.std().item(), zs.mean().item(), zs.std().item(), float(log_det_J_mean))


def epoch_end(handler: TrainerParameterHistoryHandler, epoch: int, train, val, stats, optimizer, scheduler,
              timeout: float | None, start_time: float, now: Callable[[], float] = time.time):
    """Everything _train does after an epoch's two passes (trainer.py:200-238), in its order; needs no GPU.
    train / val: the epoch's (loss, nll, mse) means; stats: z_statistics(...). Returns the stop reason
    ('val_loss_plateau' or 'timeout', also stored in parameter_history) or None to go on. handler.update_epoch(epoch)
    has been called by the caller, as at the top of the reference's loop."""
    handler.update_rolling_validation_loss(val[0])
    handler.log("train_loss", train[0])
    handler.log("train_loss_mse", train[2])
    handler.log("train_loss_nll", train[1])
    handler.log("val_loss", val[0])
    handler.log("val_loss_mse", val[2])
    handler.log("val_loss_nll", val[1])
    handler.log("lr", optimizer.param_groups[0]["lr"])
    handler.log("distance_to_last_best_val_loss", epoch - handler.best_val_epoch)
    handler.log("time", datetime.datetime.now().timestamp())
    for key, value in zip(("z_mean_mean", "z_mean_std", "z_std_mean", "z_std_std", "log_det_J"), stats):
        handler.log(key, value)
    if scheduler is not None:
        if isinstance(scheduler, torch.optim.lr_scheduler.ReduceLROnPlateau):
            scheduler.step(handler.val_loss_rolling_avg)
        elif isinstance(scheduler, torch.optim.lr_scheduler.LRScheduler):
            scheduler.step()
    handler.update_best_loss()
    # the distance logged BEFORE update_best_loss decides, compared with >= (None patience: the reference's TypeError)
    if handler.parameter_history["distance_to_last_best_val_loss"][-1][1] >= handler.val_loss_patience:
        handler.parameter_history["stop_reason"] = "val_loss_plateau"
        return "val_loss_plateau"
    if timeout is not None and now() - start_time > timeout:
        handler.parameter_history["stop_reason"] = "timeout"
        return "timeout"
    return None


def make_scheduler(config: dict, optimizer):
    sc = config.get("lr_scheduler")
    if not sc or sc.get("type") is None:
        return None
    kwargs = dict(sc.get("kwargs") or {})
    if sc["type"] == "ReduceLROnPlateau":
        return torch.optim.lr_scheduler.ReduceLROnPlateau(optimizer, **kwargs)
    cls = getattr(torch.optim.lr_scheduler, sc["type"], None)
    if cls is None:
        raise NotImplementedError(f"Scheduler {sc['type']} not implemented")
    return cls(optimizer, **kwargs)


class Trainer:
    def __init__(self, config: dict, parameter_index_mapping, hybrid_weight: float = 0, data=None,
                 verbose: bool = False, log_fn: Callable[[dict, int], None] | None = None,
                 order_fn: Callable[[int, int], torch.Tensor] | None = None) -> None:
        self.config = config
        self.verbose = verbose
        self.parameter_index_mapping = parameter_index_mapping
        self.hybrid_weight = float(hybrid_weight)
        self.log_fn = log_fn
        self.order_fn = order_fn
        self.meta_scheduler = self._handler()
        if torch.distributed.is_available() and torch.distributed.is_initialized() and \
                torch.distributed.get_world_size() > 1:
            raise NotImplementedError("bcnf_amd Trainer: world size > 1 is not supported (drive TrainStep's "
                                      "data-parallel step directly)")
        require_one_condition(config)
        self.data = self._generate() if data is None else tuple(data)
        if len(self.data) != 2:
            raise NotImplementedError(ONE_CONDITION)
        self.train_step = None
        self.validation = None

    def _handler(self, fold: int = -1):
        t = self.config["training"]
        return TrainerParameterHistoryHandler(
            val_loss_window_size=t["val_loss_window_size"], val_loss_patience=t["val_loss_patience"],
            val_loss_tolerance_mode=t["val_loss_tolerance_mode"], val_loss_tolerance=t["val_loss_tolerance"],
            fold=fold, log_fn=self.log_fn)

    def _generate(self):
        """TrainerDataHandler.get_data_for_training's generate branch (trainer_data_handler.py:53-86) on the device."""
        from bcnf_amd.generate import generate_data_device
        d = self.config["data"]
        data = generate_data_device(d["config_file"], n=d["n_samples"], output_type=d["output_type"], dt=d["dt"],
                                    T=d["T"], verbose=d.get("verbose", False),
                                    break_on_impact=d.get("break_on_impact", True), do_filter=d.get("do_filter", True))
        names = list(self.parameter_index_mapping.parameters)
        missing = [p for p in names if p not in data]
        if missing:
            raise KeyError(f'Parameter "{missing[0]}" not found in the generated data. Have: {list(data.keys())}')
        y = torch.stack([data[p].reshape(-1) for p in names], dim=1).to(torch.float32).contiguous()
        parts = []
        for key in self.config["global"]["conditions"][0]:
            v = data[key]
            parts.append(v[:, None] if v.dim() == 1 else v)
        cond = (parts[0] if len(parts) == 1 else torch.cat(parts, dim=1)).to(torch.float32).contiguous()
        return y, cond

    # ------------------------------------------------------------------ the run
    def train(self, model, start_epoch: int = 0, fold: int = -1):
        """trainer.py:50-242. `start_epoch`: the first epoch's number (the reference always starts at 0; its
        divergence check, trainer.py:168, is live after epoch 10). Returns the model; the history, best epoch and
        `stop_reason` are in `self.meta_scheduler`."""
        from bcnf_amd.train import TrainStep
        from bcnf_amd.validate import ValidationPass
        require_one_condition(model)
        cfg = self.config
        tr = cfg["training"]
        opt_cfg = cfg["optimizer"]
        if opt_cfg["type"] != "Adam":
            raise NotImplementedError(f"Optimizer {opt_cfg['type']} not implemented")
        okw = dict(opt_cfg.get("kwargs") or {})
        y, cond = self.data
        n = int(y.shape[0])
        n_train, n_val = split_sizes(n, tr["validation_split"])
        batch = int(tr["batch_size"])
        if n_train < 1 or n_val < 1:
            raise ValueError(f"bcnf_amd Trainer: the split leaves {n_train} training and {n_val} validation samples")

        ts = TrainStep(model, lr=okw.pop("lr", 1e-3), hybrid_weight=self.hybrid_weight)
        for k, v in okw.items():
            if k not in ts.opt.param_groups[0]:
                raise NotImplementedError(f"bcnf_amd Trainer: Adam option {k} is not supported by FusedAdam")
            ts.opt.param_groups[0][k] = tuple(v) if k == "betas" else v
        scheduler = make_scheduler(cfg, ts.opt)
        ts.set_pool(y[:n_train].contiguous(), cond[:n_train].contiguous())
        vp = ValidationPass(model, hybrid_weight=self.hybrid_weight)
        vp.set_pool(y[n_train:].contiguous(), cond[n_train:].contiguous(), batch)
        self.train_step, self.validation = ts, vp
        order_fn = self.order_fn or default_order_fn(tr.get("random_state"))
        n_whole = n_train // batch
        n_loader = n_whole + (1 if n_train % batch else 0)

        self.meta_scheduler = h = self._handler(fold)
        lr = ts.opt.param_groups[0]["lr"]
        start_time = time.time()
        for epoch in range(start_epoch, tr["n_epochs"]):
            h.update_epoch(epoch)
            model.train()
            order = torch.as_tensor(order_fn(epoch, n_train)).to(device=y.device, dtype=torch.int64)
            if order.numel() != n_train:
                raise ValueError(f"order_fn returned {order.numel()} indices for {n_train} training samples")
            check = epoch > 10
            triples = []
            if n_whole:
                ts.set_epoch(order[:n_whole * batch], batch)
                triples += ts.run_epoch(check_divergence=check)
            if n_loader > n_whole:
                v = ts.step_indexed(order[n_whole * batch:])
                if check and (v[0] > 1e5 or math.isnan(v[0])):
                    raise TrainingDivergedError(f"Loss exploded to {v[0]} at epoch {epoch + n_whole / n_loader}")
                triples.append(v)
            sums = [0.0, 0.0, 0.0]
            for v in triples:
                for i in range(3):
                    sums[i] += v[i]
            train = tuple(s / n_loader for s in sums)

            val_loss, val_nll, val_mse, z_mean, z_std, ldj_mean = vp.run()
            row = vp.last_row_host()
            D = (row.numel() - 4) // 2
            stats = z_statistics(row[4:4 + D], row[4 + D:], ldj_mean)

            stop = epoch_end(h, epoch, train, (val_loss, val_nll, val_mse), stats, ts.opt, scheduler,
                             tr.get("timeout"), start_time)
            if self.verbose or tr.get("verbose"):
                print(f"epoch {epoch + 1}: train {train[0]:.4f} val {val_loss:.4f} "
                      f"(avg {h.val_loss_rolling_avg:.4f}, best {h.best_val_loss:.4f}) lr {lr:.2e}")
            new_lr = ts.opt.param_groups[0]["lr"]
            if new_lr != lr:
                ts.set_lr(new_lr)       # the captured steps hold lr by value
                lr = new_lr
            if stop is not None:
                return model
        h.parameter_history["stop_reason"] = "max_epochs"
        return model


__all__ = ["Trainer", "TrainerParameterHistoryHandler", "epoch_end", "split_sizes", "default_order_fn",
           "z_statistics"]
