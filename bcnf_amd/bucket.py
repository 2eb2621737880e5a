"""The data-parallel gradient bucket of `TrainStep` (world > 1): every gradient in one buffer, ONE all-reduce per step.

The bucket holds all gradients back to back plus a 4-float tail with the step's logged (loss, nll, mse): the one
all-reduce of the step also averages them, so every rank logs -- and judges divergence on -- the global loss. The
folded backwards write their gradients straight into it (stack hooks), and with `overlap_ranges` the wide family's
backward hands finished block ranges over to be all-reduced while the rest of it runs. Works on CPU tensors under
gloo as on device tensors under RCCL.
"""
from __future__ import annotations

import contextlib

import torch
import torch.distributed as dist


def range_blocks(n_blocks: int, r: int):
    """The backward's `r` block ranges [lo, hi), in the order it finishes them (last blocks first); empty ranges
    are dropped."""
    cuts = [round(n_blocks * i / r) for i in range(r + 1)]
    return [(cuts[i - 1], cuts[i]) for i in range(r, 0, -1) if cuts[i] > cuts[i - 1]]


class GradBucket:
    def __init__(self, params, process_group, world: int):
        self.params, self.pg, self.world = params, process_group, world
        self.buf = None         # every gradient in one buffer + the logged values' tail
        self.n_grad = 0         # gradient floats in the bucket; the 3 logged values follow (reduced with them)
        self.gvals = None       # the all-reduced (loss, nll, mse) -- a view of the bucket tail
        self.packed_inplace = False    # the last pack found the gradients already in place
        self.works = []         # in-flight all-reduces of bucket slices, and the slices [lo, hi) they cover
        self.reduced = []
        self.hooks = None       # the stack attributes stack_hooks installs around each backward

    def pack_grads(self):
        """All gradients -> one contiguous bucket, so the data-parallel exchange is ONE collective per step whatever
        the number of feature-network tensors (FC_large: 17, LSTM_large: 19). Gradients the backward already wrote
        into their bucket slots (the folded backwards, FusedStack / WideStack.grad_bucket) are not copied."""
        grads = [p.grad for p in self.params]
        if any(g is None for g in grads):
            raise RuntimeError("bcnf_amd TrainStep: a parameter received no gradient")
        if self.buf is None:
            self._alloc(grads[0].device)
        base, off, slots = self.buf.data_ptr(), 0, []
        for g in grads:
            slots.append((g, off, g.is_contiguous() and g.data_ptr() == base + 4 * off))
            off += g.numel()
        self.packed_inplace = all(ok for _, _, ok in slots)
        if self.packed_inplace:
            return
        if not any(ok for _, _, ok in slots):
            torch.cat([g.reshape(-1) for g in grads], out=self.buf[:self.n_grad])
            return
        for g, o, ok in slots:
            if ok:
                continue
            if any(lo < o + g.numel() and o < hi for lo, hi in self.reduced):
                raise RuntimeError("bcnf_amd TrainStep: a gradient of an already all-reduced bucket slice is not in "
                                   "its slot")
            self.buf[o:o + g.numel()].copy_(g.reshape(-1))

    def _alloc(self, dev):
        self.n_grad = sum(p.numel() for p in self.params)
        self.buf = torch.zeros(self.n_grad + 4, dtype=torch.float32, device=dev)
        self.gvals = self.buf[self.n_grad:self.n_grad + 3]

    def setup(self, model, fold: bool, overlap_ranges: int):
        """Allocate the bucket up front and let the folded backwards (`fold`: the step runs the fused loss on a
        fused stack) write their gradients into it, no copy before the all-reduce: the small family's (coupling +
        feature Linear, FusedStack.grad_bucket), the wide family's coupling gradients (WideStack.grad_bucket), the
        latter range by range when overlap_ranges is set. The hooks are installed only around the step's own
        backward (stack_hooks), so a backward outside the TrainStep never writes into the bucket or issues
        collectives."""
        if self.buf is not None:
            return
        self._alloc(self.params[0].device)
        lin = model._fold_linear() if hasattr(model, "_fold_linear") else None
        if lin is None or not fold:
            return
        offs, off = {}, 0
        for p in self.params:
            offs[id(p)] = off
            off += p.numel()
        st = model.fused
        fp = st.flat_param
        from bcnf_amd.wide import WideStack
        if isinstance(st, WideStack):
            if id(fp) not in offs:
                return
            self.hooks = {"grad_bucket": (self.buf, offs[id(fp)])}
            if overlap_ranges > 0:
                self.hooks["range_blocks"] = range_blocks(st.cfg.n_blocks, overlap_ranges)
                self.hooks["on_range"] = self.reduce_range
            return
        if len(self.params) != (3 if lin.bias is not None else 2) or id(fp) not in offs or id(lin.weight) not in offs:
            return
        self.hooks = {"grad_bucket": (self.buf, (offs[id(fp)], offs[id(lin.weight)],
                                                 offs[id(lin.bias)] if lin.bias is not None else 0))}

    @contextlib.contextmanager
    def stack_hooks(self, stack):
        """The bucket / range hooks on the fused stack for the duration of a step's forward + backward (eager or
        being captured), removed afterwards even when the step raises."""
        if not self.hooks:
            yield
            return
        for k, v in self.hooks.items():
            setattr(stack, k, v)
        try:
            yield
        finally:
            for k in self.hooks:
                setattr(stack, k, None)

    def drain_slices(self):
        """Join and forget slice all-reduces a previous step left in flight (it raised between issuing them and the
        update's join), so this step neither skips those slices nor waits on stale handles."""
        works, self.works = self.works, []
        self.reduced.clear()
        for w in works:
            try:
                w.wait()
            except Exception:       # the failed step's own error was already raised to the caller
                pass

    def bind_grads(self):
        """Every .grad becomes a view of the (reduced) bucket: Adam and the clip read it in place."""
        off = 0
        for p in self.params:
            n = p.numel()
            p.grad = self.buf[off:off + n].view_as(p)
            off += n

    def reduce(self):
        """Sum over ranks of the gradient bucket: ONE RCCL all-reduce per step (the 1/world scaling runs inside
        the captured update segment, scale). With slices already in flight (overlap_ranges), the rest of the
        bucket -- the feature-network gradients and the logged values -- then a join on every slice."""
        if not self.works:
            dist.all_reduce(self.buf, op=dist.ReduceOp.SUM, group=self.pg)
            return
        lo = 0
        for a, b in sorted(self.reduced) + [(self.buf.numel(), self.buf.numel())]:
            if a > lo:
                dist.all_reduce(self.buf[lo:a], op=dist.ReduceOp.SUM, group=self.pg)
            lo = max(lo, b)
        for w in self.works:
            w.wait()
        self.works.clear()
        self.reduced.clear()

    def reduce_range(self, lo: int, hi: int):
        """A finished block range's bucket slice [lo, hi): its all-reduce runs while the backward continues
        (WideStack.on_range); the update joins it (reduce)."""
        self.works.append(dist.all_reduce(self.buf[lo:hi], op=dist.ReduceOp.SUM, group=self.pg, async_op=True))
        self.reduced.append((lo, hi))

    def scale(self):
        self.buf.mul_(1.0 / self.world)

    def allreduce(self, vals=None):
        """Eager data-parallel exchange; returns the all-reduced logged values (None without `vals`)."""
        self.pack_grads()
        if vals is not None:
            self.gvals.copy_(vals)
        self.reduce()
        self.scale()
        self.bind_grads()
        return self.gvals if vals is not None else None

    def check_global(self, guard):
        """The divergence guard judged on the all-reduced loss (bcnf_guard_check_global)."""
        if guard is None:
            return
        from bcnf_amd import _native as N
        N.call("bcnf_guard_check_global", self.gvals, guard, N.stream_handle(self.gvals.device))


__all__ = ["GradBucket", "range_blocks"]
