"""The device-resident data pool and the epoch walk over it, shared by `TrainStep` and `ValidationPass`.

`DevicePool` holds the two pool tensors (targets and ONE condition) and serves rows of both in one native launch;
`EpochWalk` is an order of pool indices walked batch by batch on a device cursor, so a captured step needs no
host-to-device traffic. The walk never advances the cursor: the launch that ends a step does (the clip, Adam's
bookkeeping, the validation statistics). `graph_schedule` is the one place that decides how many batches each
captured multi-batch graph of an epoch runs.
"""
from __future__ import annotations

import torch


def check_indices(idx, n: int):
    """Pool indices in range (the reference's DataLoader raises IndexError; the device gather would read out of
    bounds), before anything is launched. Host indices (a DataLoader's) are checked on the host, no device sync;
    device-resident indices cost one host round trip."""
    if idx.numel() == 0:
        return
    lo, hi = torch.aminmax(idx if idx.device.type == "cpu" else idx.to(torch.int64))
    if int(lo) < 0 or int(hi) >= n:
        raise IndexError(f"bcnf_amd TrainStep: batch index out of range [0, {n}) (got {int(lo)}..{int(hi)})")


def graph_schedule(n: int, unroll: int, smallest: int):
    """The multi-batch graphs replayed for `n` whole batches: sizes unroll, unroll / 2, ... down to `smallest`, each
    as often as it fits, largest first (20 batches, unroll 8: 8 + 8 + 4). A graph boundary costs ~9 us of idle GPU
    between two replays, so fewer, longer graphs; what the sizes leave over runs batch by batch."""
    out, k = [], unroll
    while k >= max(smallest, 1):
        out += [k] * (n // k)
        n %= k
        k //= 2
    return out


def whole_batches(numel: int, batch: int, keep=None) -> int:
    """Batches in an order of `numel` indices; whole batches only (a ragged last batch, drop_last=False, goes
    through step_indexed, which runs a batch of another size eagerly). keep = (n_batches, batch) of a walk whose
    captured graphs hold buffers of that size."""
    nb = numel // batch
    if nb < 1 or numel != nb * batch:
        raise ValueError(f"set_epoch: order must hold a whole number of batches ({numel} indices, "
                         f"batch {batch}); pass the remainder to step_indexed()")
    if keep is not None and (nb, batch) != keep:
        raise ValueError("set_epoch: a captured TrainStep keeps its order size")
    return nb


class DevicePool:
    """`y` (n, D) and `cond` (n, *cond_shape): contiguous fp32 device tensors. With `row_width` the condition rows
    are zero-padded to that many floats (the folded feature Linear reads 16-byte-aligned rows with float4 loads:
    90 -> 92 floats for FC_small) and `cond_shape` = (per-sample shape, its size X); else `cond_shape` is None."""

    def __init__(self, y, cond, row_width=None, who: str = "set_pool"):
        for t in (y, cond):
            if not (t.is_cuda and t.dtype == torch.float32 and t.is_contiguous()):
                raise ValueError(f"{who}: contiguous fp32 device tensors required")
        self.cond_shape = None
        if row_width is not None:
            X = cond[0].numel()
            padded = torch.zeros((cond.shape[0], row_width), dtype=cond.dtype, device=cond.device)
            padded[:, :X] = cond.reshape(cond.shape[0], X)
            self.cond_shape = (tuple(cond.shape[1:]), X)
            cond = padded
        self.y, self.cond = y, cond
        self.n, self.device = y.shape[0], y.device

    def unpad(self, t):
        """A batch of the padded condition pool as the (n, *cond_shape) view the model expects (row stride = the
        padded width; the folded path reads it in place with float4 loads)."""
        if self.cond_shape is None:
            return t
        shape, X = self.cond_shape
        return t[:, :X].view((t.shape[0],) + shape)

    def rows(self, idx):
        return self.y.index_select(0, idx), self.unpad(self.cond.index_select(0, idx))

    def empty_batch(self, n: int):
        """The two uninitialised destination tensors of an n-row gather (the condition rows at the pool's width)."""
        return tuple(torch.empty((n,) + tuple(p.shape[1:]), dtype=p.dtype, device=p.device)
                     for p in (self.y, self.cond))

    def gather_rows(self, idx, out=None):
        """(y[idx], cond[idx]) by a device index buffer, both tensors in one native launch on the current stream."""
        from bcnf_amd import _native as N
        y, c = out if out is not None else self.empty_batch(idx.shape[0])
        N.call("bcnf_gather_rows2", idx, idx.shape[0], self.y, self.y[0].numel(), y, self.cond,
               self.cond[0].numel(), c, N.stream_handle(self.device))
        return y, self.unpad(c)

    def gather_spec(self, idx, n: int, cursor=None, out=None):
        """(y, cond, spec): the same gather, not launched -- the BcnfGather2 for the folded path's pack launch to
        run (bcnf_pack_params_fold). With `cursor`, rows idx[cursor[0] * n + r]."""
        from bcnf_amd import _native as N
        y, c = out if out is not None else self.empty_batch(n)
        spec = N.BcnfGather2(idx=idx.data_ptr(), cursor=None if cursor is None else cursor.data_ptr(), n=n,
                             src0=self.y.data_ptr(), cols0=self.y[0].numel(), dst0=y.data_ptr(),
                             src1=self.cond.data_ptr(), cols1=self.cond[0].numel(), dst1=c.data_ptr())
        return y, self.unpad(c), spec


class EpochWalk:
    """`order` (n_batches * batch pool indices, e.g. a shuffled epoch) walked batch by batch: `cursor` (device int64,
    one element) is the batch the next gather reads, `host_cursor` its host mirror (the history row of the next
    step), kept by the caller that knows which launches advanced the device's."""

    def __init__(self, pool: DevicePool, order, batch: int):
        self.n_batches = whole_batches(order.numel(), batch)
        check_indices(order, pool.n)
        self.pool, self.batch = pool, batch
        self.order = order.to(device=pool.device, dtype=torch.int64).contiguous().clone()
        self.cursor = torch.zeros(1, dtype=torch.int64, device=pool.device)
        self.host_cursor = 0

    def reset(self, order, batch=None):
        """Another order of the same size (captured graphs hold this walk's buffers), from its first batch."""
        whole_batches(order.numel(), self.batch if batch is None else batch, keep=(self.n_batches, self.batch))
        check_indices(order, self.pool.n)
        self.order.copy_(order)
        self.rewind()

    def rewind(self):
        self.cursor.zero_()
        self.host_cursor = 0

    def gather(self, out=None):
        """The cursor's batch of both pool tensors, one native launch on the current stream."""
        from bcnf_amd import _native as N
        p = self.pool
        y, c = out if out is not None else p.empty_batch(self.batch)
        N.call("bcnf_gather_batch", self.order, self.cursor, self.batch, p.y, p.y[0].numel(), y, p.cond,
               p.cond[0].numel(), c, N.stream_handle(p.device))
        return y, p.unpad(c)

    def gather_spec(self, out=None):
        return self.pool.gather_spec(self.order, self.batch, self.cursor, out)


__all__ = ["DevicePool", "EpochWalk", "check_indices", "graph_schedule", "whole_batches"]
