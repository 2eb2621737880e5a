"""Host runtime of the wide-MLP coupling stack (trajectory_FC_large / trajectory_LSTM_large class).

Same contract as `FusedStack` (both are a `StackBase`, bcnf_amd/fused.py, which holds what the families share): one
flat fp32 buffer of the trainable coupling parameters in state_dict order with every nn.Parameter a view into it, the
frozen orthonormal matrices in a second buffer, the same autograd Functions (`_StackForward`, `_StackNLL`,
`_StackInverse`) and the same launch_* methods, so CondRealNVP_v2, TrainStep and the optimizer do not know which family
runs. The arithmetic is in libbcnf_amd.so (bcnf_amd/csrc/bcnf_wide.hip): fp32-MFMA GEMMs with fused
bias/GELU/dropout/gradient epilogues and per-sample link kernels; the condition projection h W0h^T of all blocks is
one GEMM per pass.
"""
from __future__ import annotations

import math

import torch

from bcnf_amd import _native as N
from bcnf_amd.fused import FusedStack, StackBase

_LOG2PI = math.log(2.0 * math.pi)


class WideStack(StackBase):
    """The wide-MLP family: drives the wide HIP kernels. As in FusedStack, a `_*_call` method validates, allocates and
    returns ((entry point, *arguments), results) for `launch_*` to run and `time_kernels` to time."""

    @property
    def supported(self) -> bool:
        return bool(N.call_raw("bcnf_wide_supported", self._pdesc))

    def counts(self):
        rc, (a, b) = N.query_status("bcnf_wide_param_count", self._pdesc, outs=2)
        N.check(rc, "bcnf_wide_param_count")
        return a, b

    def _packed_bytes(self):
        return N.query_i64("bcnf_wide_packed_bytes", self._pdesc)

    def _pack_into(self, out):
        """Padded weight copies (bcnf_wide_pack)."""
        N.call("bcnf_wide_pack", self._pdesc, self.flat, self.qflat, out, N.stream_handle(self.flat.device))

    def workspace_bytes(self, batch: int, save: bool):
        return N.query_i64("bcnf_wide_workspace_bytes", self._pdesc, batch, save), 0

    def _workspace(self, batch, save, dev):
        wb, _ = self.workspace_bytes(batch, save)
        return torch.empty(max(wb // 4, 1), dtype=torch.float32, device=dev)

    # ------------------------------------------------------------------ launches
    def _forward_call(self, y, h, training, save, nll_part=None):
        self._check_forward(y, h)
        B = y.shape[0]
        dev = y.device
        z = torch.empty_like(y)
        ldj = torch.empty(B, dtype=torch.float32, device=dev)
        rng = self.rng_state() if self._dropping(training) else None
        ws = self._workspace(B, save, dev)
        pk = self.packed(fresh=save)
        launch = ("bcnf_wide_forward", self._pdesc, self.flat, pk, y, h, B, z, ldj, nll_part, training, rng, ws, save,
                  N.stream_handle(dev))
        return launch, (z, ldj, rng, (ws, pk))

    def _forward(self, y, h, training, save, nll_part=None):
        launch, out = self._forward_call(y, h, training, save, nll_part)
        N.call(*launch)
        return out

    def launch_forward(self, y, h, training: bool, save: bool, want_logp: bool = False):
        B = y.shape[0]
        part = torch.empty(B, dtype=torch.float32, device=y.device) if want_logp else None
        z, ldj, rng, saved = self._forward(y, h, training, save, part)
        self._advance_rng(rng)
        logp = None
        if want_logp:
            logp = -part - 0.5 * self.cfg.size * _LOG2PI
        return z, ldj, logp, saved

    def launch_backward(self, h, dz, dldj, training: bool, saved, want_dy: bool, want_dh: bool):
        return self._backward(h, None, dz, dldj, None, False, saved, want_dy, want_dh)

    def _backward_call(self, h, z, dz, dldj, dvals, nll, saved, want_dy, want_dh):
        ws, pk = saved
        B = h.shape[0]
        dev = h.device
        dparams = torch.empty_like(self.flat)
        dh = torch.empty_like(h) if want_dh else None
        dy = torch.empty((B, self.cfg.size), dtype=torch.float32, device=dev) if want_dy else None
        launch = ("bcnf_wide_backward", self._pdesc, self.flat, pk, h, z, dz, dldj, dvals, nll, B, ws, dy, dh, dparams,
                  N.stream_handle(dev))
        return launch, (dy, dh, dparams)

    def _backward(self, *args):
        launch, out = self._backward_call(*args)
        N.call(*launch)
        return out

    def _finalize(self, ws, B, vals, training, save=True):
        rng = self.rng_state() if self._dropping(training) else None
        N.call("bcnf_wide_nll_finalize", self._pdesc, ws, B, save, vals, rng, self.guard,
               N.stream_handle(vals.device))

    def launch_nll_forward(self, y, h, training: bool, finalize: bool = True):
        B = y.shape[0]
        if B == 0:
            raise ValueError("bcnf_amd: the NLL of an empty batch is undefined")
        z, ldj, _, saved = self._forward(y, h, training, True)
        vals = torch.empty(3, dtype=torch.float32, device=y.device)
        if finalize:
            self._finalize(saved[0], B, vals, training)
        return z, ldj, vals, saved

    def launch_nll_backward(self, h, z, dvals, training: bool, saved, want_dy: bool, want_dh: bool,
                            finalize_into=None):
        if finalize_into is not None:
            self._finalize(saved[0], h.shape[0], finalize_into, training)
        return self._backward(h, z, None, None, dvals, True, saved, want_dy, want_dh)

    # ------------------------------------------------------------------ folded last feature Linear
    # h = x Wf^T + bf enters the stack only through the condition projection: P = [x | 1] (W0h_all [Wf | bf])^T, and
    # the backward forms Gx = dZ0^T [x | 1] instead of dL/dh (include/bcnf_amd.h, bcnf_wide_fold_*).
    def fold_supported(self, in_features: int) -> bool:
        """Whether the last feature nn.Linear [in_features -> n_conditions] can be folded into the condition
        projection (bcnf_wide_fold_*): any width."""
        return in_features >= 1

    def _fold_operands(self, x, wf, bf, pk):
        B, X = x.shape
        xp = (X + 1 + 3) // 4 * 4
        dev = x.device
        x1 = torch.zeros((B, xp), dtype=torch.float32, device=dev)
        x1[:, :X] = x
        x1[:, X] = 1.0
        wfb = torch.zeros((wf.shape[0], xp), dtype=torch.float32, device=dev)
        wfb[:, :X] = wf
        if bf is not None:
            wfb[:, X] = bf
        rows = N.query_i64("bcnf_wide_proj_rows", self._pdesc)
        wcb = torch.empty((rows, xp), dtype=torch.float32, device=dev)
        N.call("bcnf_wide_fold_prepare", self._pdesc, pk, wfb, xp, wcb, N.stream_handle(dev))
        return x1, wfb, wcb, xp

    def _fold_forward_call(self, y, x, wf, bf, training):
        cfg = self.cfg
        if y.dim() != 2 or y.shape[1] != cfg.size:
            raise ValueError(f"bcnf_amd forward: expected (N, {cfg.size}) input, got {tuple(y.shape)}")
        if x.dim() != 2 or x.shape[0] != y.shape[0] or tuple(wf.shape) != (cfg.n_conditions, x.shape[1]):
            raise ValueError(f"bcnf_amd forward: folded features need x (N, X) and Wf ({cfg.n_conditions}, X), got "
                             f"{tuple(x.shape)} and {tuple(wf.shape)}")
        self._check_device(y, x, wf, bf)
        B = y.shape[0]
        if B == 0:
            raise ValueError("bcnf_amd: the NLL of an empty batch is undefined")
        dev = y.device
        z = torch.empty_like(y)
        ldj = torch.empty(B, dtype=torch.float32, device=dev)
        rng = self.rng_state() if self._dropping(training) else None
        ws = self._workspace(B, True, dev)
        pk = self.packed(fresh=True)
        x1, wfb, wcb, xp = self._fold_operands(x, wf, bf, pk)
        launch = ("bcnf_wide_fold_forward", self._pdesc, self.flat, pk, y, x1, xp, wcb, B, z, ldj, training, rng, ws,
                  N.stream_handle(dev))
        return launch, (z, ldj, (ws, pk, x1, wfb, wcb, xp, x.shape[1]))

    def launch_fold_nll_forward(self, y, x, wf, bf, training: bool, finalize: bool = True):
        launch, (z, ldj, saved) = self._fold_forward_call(y, x, wf, bf, training)
        N.call(*launch)
        vals = torch.empty(3, dtype=torch.float32, device=y.device)
        if finalize:
            self._finalize(saved[0], y.shape[0], vals, training)
        return z, ldj, vals, saved

    # Data parallel (TrainStep): (bucket, offset) -- the coupling gradients land in bucket[offset:offset + n], a view
    # that autograd adopts as .grad; and, with range_blocks (descending real-block ranges covering [0, nb)), the
    # backward runs range by range and calls on_range(lo, hi) with each finished range's bucket slice [lo, hi), so
    # the slice's all-reduce overlaps the rest of the backward (one bcnf_wide_fold_backward call per range).
    grad_bucket = None
    range_blocks = None
    on_range = None

    def block_offset(self, block: int) -> int:
        """Canonical flat offset of real block `block` (block = nb: the parameter count)."""
        return N.query_i64("bcnf_wide_block_offset", self._pdesc, block)

    def _fold_backward_args(self, z, dvals, saved, want_x):
        """bcnf_wide_fold_backward's arguments up to the block range and the stream, the gradient buffers among them:
        dparams is the bucket's slice in a data-parallel TrainStep."""
        ws, pk, x1, wfb, wcb, xp, _ = saved
        B = z.shape[0]
        gx = torch.empty_like(wcb)
        if self.grad_bucket is not None:
            bucket, off = self.grad_bucket
            dparams = bucket.narrow(0, off, self.flat.numel()).view_as(self.flat)
        else:
            dparams = torch.empty_like(self.flat)
        dwfb = torch.empty_like(wfb)
        dx = torch.empty((B, xp), dtype=torch.float32, device=z.device) if want_x else None
        args = (self._pdesc, self.flat, pk, x1, xp, wfb, wcb, z, dvals, B, ws, gx, dparams, dwfb, dx)
        return args, (gx, dparams, dwfb, dx)

    def launch_fold_nll_backward(self, z, dvals, training: bool, saved, want_x: bool, finalize_into=None):
        ws, pk, x1, wfb, wcb, _, X = saved
        dev = z.device
        if finalize_into is not None:
            self._finalize(ws, z.shape[0], finalize_into, training)
        args, (gx, dparams, dwfb, dx) = self._fold_backward_args(z, dvals, saved, want_x)
        stream = N.stream_handle(dev)
        if self.range_blocks and self.on_range is not None and self.grad_bucket is not None:
            off = self.grad_bucket[1]
            for lo, hi in self.range_blocks:
                N.call("bcnf_wide_fold_backward", *args, lo, hi, stream)
                self.on_range(off + self.block_offset(lo), off + self.block_offset(hi))
        else:
            N.call("bcnf_wide_fold_backward", *args, 0, self.cfg.n_blocks, stream)
        return dparams, dwfb[:, :X], dwfb[:, X], (dx[:, :X] if want_x else None)

    @torch.no_grad()
    def time_kernels(self, y, h, training: bool = True, iters: int = 20, fold=None):
        """Average device time (us) of the wide forward (save on) and backward launches of one NLL training pass
        (_time_calls), the loss reduction never run, so no call advances the dropout offset. fold = (x, Wf, bf): the
        folded training launches instead."""
        if fold is None:
            forward, (z, _, _, saved) = self._forward_call(y, h, training, True)
            backward, _ = self._backward_call(h, z, None, None, None, True, saved, False, True)
        else:
            forward, (z, _, saved) = self._fold_forward_call(y, *fold, training)
            args, _ = self._fold_backward_args(z, None, saved, want_x=True)
            backward = ("bcnf_wide_fold_backward", *args, 0, self.cfg.n_blocks, N.stream_handle(y.device))
        return self._time_calls({"forward": forward, "backward": backward}, iters)

    # ------------------------------------------------------------------ inverse (StackBase.launch_inverse)
    def _inverse_scratch_bytes(self, feature_rows, n):
        return N.query_i64("bcnf_wide_inverse_scratch_bytes", self._pdesc, feature_rows, n)

    def _native_inverse(self, z, h, cond_index, y, training, rng, scratch):
        N.call("bcnf_wide_inverse", self._pdesc, self.flat, self.packed(), z, h, h.shape[0], cond_index, z.shape[0], y,
               training, rng, scratch, N.stream_handle(z.device))

    def _native_inverse_logdet(self, z, h, cond_index, y, training, ldj, logp, scratch):
        N.call("bcnf_wide_inverse_logdet", self._pdesc, self.flat, self.packed(), z, h, h.shape[0], cond_index,
               z.shape[0], y, ldj, logp, scratch, N.stream_handle(z.device))
        return y, ldj, logp


class _WideFoldNLL(torch.autograd.Function):
    """vals = [loss, nll, mse] of the wide stack with the feature network's last Linear folded into the condition
    projection: inputs (y, x, Wf, bf, flat_param); gradients for x (the earlier feature layers), Wf, bf and flat_param."""

    @staticmethod
    def forward(ctx, y, x, wf, bf, flat_param, stack: WideStack, training: bool, defer: bool):
        z, _, vals, saved = stack.launch_fold_nll_forward(y, x, wf, bf, training, finalize=not defer)
        ctx.stack, ctx.training, ctx.saved, ctx.defer = stack, training, saved, defer
        ctx.has_bias = bf is not None
        ctx.save_for_backward(z, vals)
        return vals

    @staticmethod
    def backward(ctx, dvals):
        z, vals = ctx.saved_tensors
        need_x = ctx.needs_input_grad[1]
        dparams, dwf, dbf, dx = ctx.stack.launch_fold_nll_backward(
            z, dvals.contiguous(), ctx.training, ctx.saved, want_x=need_x, finalize_into=vals if ctx.defer else None)
        return (None, dx, dwf, (dbf if ctx.has_bias else None), (dparams if ctx.needs_input_grad[4] else None), None,
                None, None)


def stack_nll_wide_fold(stack: WideStack, y, x, wf, bf, training: bool, defer: bool = False):
    y = y.contiguous()
    x = x.contiguous()
    stack.sync_grad_state()
    fp = stack.flat_param if stack.trainable[0].requires_grad else stack.flat_param.detach()
    return _WideFoldNLL.apply(y, x, wf, bf, fp, stack, training, defer)


def make_stack(cfg, trainable, frozen, bind: bool = True) -> StackBase:
    """The register-resident small family when the shape fits it (FC_small), else the wide-MLP family."""
    st = FusedStack(cfg, trainable, frozen, bind=False)
    if not st.supported:
        wd = WideStack(cfg, trainable, frozen, bind=False)
        if wd.supported:
            st = wd
    if bind:
        st.bind = True
        st.flatten()
    return st


__all__ = ["WideStack", "make_stack", "stack_nll_wide_fold"]
