"""The validation epoch of `bcnf.train.Trainer._train` (src/bcnf/train/trainer.py:181-198, 213-217) on the device.

The reference runs, per validation batch, an eval-mode forward, three losses, `z.mean(0)`, `z.std(0)` and three
`.item()` host syncs, and after the loop logs the LAST batch's `z_mean`, `z_std` and `model.log_det_J.mean()`:

    model.eval()
    with torch.no_grad():
        for y, *conditions in val_loader:                 # shuffle is irrelevant to every value but the last batch's
            z, h = model(y, *conditions, log_det_J=True, return_features=True)
            mse = MSE(prediction_head(h), y) if hybrid_weight > 0 else 0
            nll = inn_nll_loss(z, model.log_det_J)
            loss = (nll + mse * w) / (1 + w)
            val_loss += loss.item(); ...

`ValidationPass.run()` gathers each batch from a device pool on a device cursor (bcnf_amd/epoch.py), runs the same
forward on the fused kernels and ONE bcnf_validation_stats launch per batch, which writes the batch's row
`[loss, nll, mse, mean(ldj), z_mean[D], z_std[D]]`, adds the triple into a 3-double epoch sum on the device and
advances the cursor. The whole batches are replayed as captured multi-batch graphs (8, 4, 2, 1 batches per graph, as
`TrainStep.run_epoch`'s multi-step graphs); the ragged last batch (DataLoader drop_last=False) runs eagerly on the same
kernels. One stream sync per `run()`.

The pool is walked in its own order (the identity): the epoch means do not depend on the validation loader's shuffle,
only the three last-batch statistics do, and those are reported for the pool's last batch.

`validation_stats_host` restates the kernel in numpy float64; the tests use it as the kernel's oracle.
"""
from __future__ import annotations

import numpy as np
import torch

from bcnf_amd.epoch import DevicePool, EpochWalk, graph_schedule

ONE_CONDITION = ("bcnf_amd: the device training loop serves models with ONE condition tensor (TrainStep's "
                 "one-condition limit: its pool, gather and captured step take a single condition)")


def require_one_condition(model_or_config):
    """NotImplementedError for a model whose feature stack takes, or a run config (dict) that lists, more than one
    condition."""
    if isinstance(model_or_config, dict):
        conditions = model_or_config.get("global", {}).get("conditions")
        many = conditions is not None and len(conditions) > 1
    else:
        fns = getattr(model_or_config, "feature_network_stack", None)
        many = fns is not None and getattr(fns, "n_distinct_conditions", 1) > 1
    if many:
        raise NotImplementedError(ONE_CONDITION)


def validation_stats_host(z, ldj, pred=None, y=None, w: float = 0.0):
    """bcnf_validation_stats in numpy float64 -> (loss, nll, mse, ldj_mean, z_mean[D], z_std[D]).

    nll, mse, mean(ldj), z_mean and z_std are float64 (the kernel rounds each once to fp32); loss is the fp32
    expression (nll + mse * w) / (1 + w) on the ROUNDED nll and mse, as the kernel and the reference's fp32 tensor
    expression evaluate it. z_std is torch.std's unbiased estimate from the two-pass sum of squared deviations
    (NaN at B = 1)."""
    z = np.asarray(z, dtype=np.float64)
    ldj = np.asarray(ldj, dtype=np.float64).reshape(-1)
    B, D = z.shape
    nll = float((0.5 * (z * z).sum() - ldj.sum()) / B)
    mse = 0.0
    if pred is not None:
        d = np.asarray(pred, dtype=np.float64) - np.asarray(y, dtype=np.float64)
        mse = float((d * d).sum() / (B * D))
    z_mean = z.sum(0) / B
    dev = z - z_mean
    with np.errstate(invalid="ignore", divide="ignore"):
        z_std = np.sqrt((dev * dev).sum(0) / np.float64(B - 1))
    wf = np.float32(w)
    loss = float((np.float32(nll) + np.float32(mse) * wf) / (np.float32(1.0) + wf))
    return loss, nll, mse, float(ldj.sum() / B), z_mean, z_std


def validation_stats(z, ldj, pred=None, y=None, w: float = 0.0, row=None, epoch_sum=None, cursor=None,
                     n_batches: int = 1):
    """One bcnf_validation_stats launch on the current stream; returns the row tensor (4 + 2 D floats, or the
    (n_batches, 4 + 2 D) rows when a cursor selects the row)."""
    from bcnf_amd import _native as N
    B, D = z.shape
    if row is None:
        row = torch.empty((n_batches if cursor is not None else 1, 4 + 2 * D), dtype=torch.float32, device=z.device)
    N.call("bcnf_validation_stats", z, ldj, pred, y, B, D, float(w), row, epoch_sum, cursor, n_batches,
           N.stream_handle(z.device))
    return row


class ValidationPass:
    """`ValidationPass(model, hybrid_weight).set_pool(y, cond, batch)`, then `.run()` after every training epoch:
    (val_loss, val_loss_nll, val_loss_mse, z_mean, z_std, log_det_J_mean) as the reference's epoch computes them --
    the three losses averaged over ceil(n / batch) batches, the other three from the last batch (z_mean / z_std are
    device tensors of D floats, log_det_J_mean a Python float).

    The model is put in eval mode for the pass and its mode restored; eval-mode launches draw no dropout masks, so the
    dropout RNG does not advance. Parameters are read by the captured launches where they live (the pack is a graph
    node), so a run() after further training sees the new weights."""

    unroll = 8         # batches per captured graph, then 4, 2, 1 (TrainStep.epoch_unroll)

    def __init__(self, model, hybrid_weight: float = 0.0, capture: bool = True):
        require_one_condition(model)
        self.model = model
        self.hybrid_weight = float(hybrid_weight)
        if self.hybrid_weight > 0.0 and not getattr(model, "hybrid", False):
            raise ValueError("bcnf_amd ValidationPass: hybrid_weight > 0 needs a model built with hybrid=True")
        self.layerwise = getattr(model, "_path", "fused") == "layerwise"
        self.capture = bool(capture) and not self.layerwise
        self.pool = None
        self._graphs = {}
        self.rows = None

    # ------------------------------------------------------------------ pool
    def set_pool(self, y_pool, cond_pool, batch: int):
        pool = DevicePool(y_pool, cond_pool, who="ValidationPass.set_pool")
        n, batch = pool.n, int(batch)
        if n < 1 or cond_pool.shape[0] != n or batch < 1:
            raise ValueError("ValidationPass.set_pool: y_pool and cond_pool need the same, non-zero, number of rows "
                             "and batch >= 1")
        dev = pool.device
        self.pool = pool
        self.batch = batch
        self.n_whole = n // batch
        self.tail = n - self.n_whole * batch
        self.n_batches = self.n_whole + (1 if self.tail else 0)
        D = y_pool.shape[1]
        # the whole batches, in the pool's own order; None when the pool is smaller than one batch
        self.walk = EpochWalk(pool, torch.arange(self.n_whole * batch), batch) if self.n_whole else None
        self.rows = torch.zeros((self.n_batches, 4 + 2 * D), dtype=torch.float32, device=dev)
        self._sum = torch.zeros(3, dtype=torch.float64, device=dev)
        self._host_sum = torch.zeros(3, dtype=torch.float64).pin_memory()
        self._host_row = torch.zeros(4 + 2 * D, dtype=torch.float32).pin_memory()
        self._graphs = {}
        self._warm = False

    # ------------------------------------------------------------------ one batch
    def _stats(self, y, cond, row, cursor):
        m = self.model
        z, h = m.forward(y, cond, log_det_J=True, return_features=True)
        pred = None
        if self.hybrid_weight > 0.0:
            from bcnf_amd import _native as N
            head = m.prediction_head       # nn.Linear(C, D) on the library's Linear kernel, as the feature networks'
            h = h.contiguous()
            pred = torch.empty((h.shape[0], head.out_features), dtype=torch.float32, device=h.device)
            N.call("bcnf_linear_forward", h, head.weight, head.bias, h.shape[0], h.shape[1], head.out_features, pred,
                   N.stream_handle(h.device))
        validation_stats(z.contiguous(), m.log_det_J.contiguous(), pred, y if pred is not None else None,
                         self.hybrid_weight, row=row, epoch_sum=self._sum, cursor=cursor,
                         n_batches=max(self.n_whole, 1))

    def _whole_batch(self):
        """The cursor's batch: gather, forward, statistics into rows[cursor]; the stats launch advances the cursor."""
        y, c = self.walk.gather()
        self._stats(y, c, self.rows, self.walk.cursor)

    def _graph(self, k: int):
        if k not in self._graphs:
            g = torch.cuda.CUDAGraph()
            with torch.cuda.graph(g):
                for _ in range(k):
                    self._whole_batch()
            self._graphs[k] = g
        return self._graphs[k]

    # ------------------------------------------------------------------ the epoch
    def run(self):
        if self.pool is None:
            raise RuntimeError("ValidationPass.run() needs set_pool()")
        m = self.model
        was_training = m.training
        m.eval()
        try:
            with torch.no_grad():
                self._sum.zero_()
                n = self.n_whole
                if n:
                    self.walk.rewind()
                if n and self.capture and not self._warm:
                    # allocations and kernel attributes settle outside any capture; the warm-up batches are whole
                    # batches of this epoch (the cursor walks on), so nothing is run twice
                    s = torch.cuda.Stream()
                    s.wait_stream(torch.cuda.current_stream())
                    with torch.cuda.stream(s):
                        self._whole_batch()
                        self._sum.zero_()
                        self.walk.rewind()
                    torch.cuda.current_stream().wait_stream(s)
                    self._warm = True
                sched = graph_schedule(n, self.unroll, 1) if self.capture else []
                for k in sched:
                    self._graph(k).replay()
                for _ in range(n - sum(sched)):
                    self._whole_batch()
                if self.tail:
                    lo = n * self.batch
                    self._stats(self.pool.y[lo:], self.pool.cond[lo:], self.rows[n], None)
                self._host_sum.copy_(self._sum, non_blocking=True)
                self._host_row.copy_(self.rows[self.n_batches - 1], non_blocking=True)
                torch.cuda.current_stream().synchronize()
        finally:
            m.train(was_training)
        nb = self.n_batches
        loss, nll, mse = (float(v) / nb for v in self._host_sum.tolist())
        D = (self._host_row.numel() - 4) // 2
        last = self.rows[nb - 1]
        return loss, nll, mse, last[4:4 + D].clone(), last[4 + D:].clone(), float(self._host_row[3])

    def last_row_host(self):
        """The last batch's row as run() copied it to the host (no further sync): [loss, nll, mse, mean(ldj),
        z_mean[D], z_std[D]]."""
        return self._host_row.clone()


__all__ = ["ValidationPass", "require_one_condition", "validation_stats", "validation_stats_host"]
