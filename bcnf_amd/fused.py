"""Host runtime of the fused HIP coupling stack: flat parameter storage, packing, workspaces and the
autograd boundary. PyTorch provides device memory, streams and autograd plumbing; all arithmetic of
the coupling stack runs in libbcnf_amd.so (bcnf_amd/csrc/bcnf_stack*.hip; the file map: bcnf_stack_internal.h).

Parameter storage
-----------------
The trainable coupling-stack parameters (ActNorm scale/bias + every nested-MLP Linear, in state_dict
order, orthonormal matrices excluded) live in ONE contiguous fp32 buffer; every nn.Parameter of the
reference module tree (`layers.0.scale`, `layers.1.nn_a.nn.0.weight`, ...) is a view into it, so
state_dict / load_state_dict / optimizers keep working unchanged. The frozen orthonormal matrices
live in a second buffer. `flat_param` is a leaf Parameter over the same storage: the autograd
Function returns the whole flat gradient for it in a single AccumulateGrad. In "per_param" grad mode
(the default, what the unchanged bcnf Trainer expects) a post-accumulate hook additionally exposes
per-layer `.grad` tensors as views of that flat gradient.
"""
from __future__ import annotations

import ctypes
from dataclasses import dataclass

import torch

from bcnf_amd import _native as N


@dataclass
class StackConfig:
    size: int
    nested_sizes: tuple
    n_blocks: int
    n_conditions: int
    dropout: float
    act_norm: bool
    two_way: bool

    def desc(self):
        return N.make_desc(self.size, list(self.nested_sizes), self.n_blocks, self.n_conditions, self.dropout,
                           self.act_norm, self.two_way)


class StackBase:
    """What the kernel families share: the flat parameter buffers of one coupling stack, the pack policy, the dropout
    RNG state, TrainStep's hooks, the inverse and the timing loop. A family (FusedStack here, WideStack in wide.py)
    adds `supported`, `counts`, its packed-bytes query, `_pack_into`, the inverse's native calls and its launches."""

    def __init__(self, cfg: StackConfig, trainable: list, frozen: list, bind: bool = True):
        self.cfg = cfg
        self.bind = bind
        self.desc = cfg.desc()
        self._pdesc = ctypes.byref(self.desc)
        self.trainable = list(trainable)   # canonical order (state_dict order, orthonormal excluded)
        self.frozen = list(frozen)         # orthonormal matrices, block order
        self.grad_mode = "per_param"
        self._packed = None
        self._pack_frozen = False
        self._rng_state = None
        self.seed = None
        self.guard = None        # device int32[BCNF_GUARD_WORDS] divergence guard of a TrainStep, or None
        if bind:
            self.flatten()
        else:   # standalone layer: flat params are provided per call (see stack_forward(flat=...))
            self.flat = None
            self.qflat = None
            self.flat_param = None

    # ------------------------------------------------------------------ layout
    @staticmethod
    def _gather_views(tensors, dev, min_numel: int = 0):
        """Copy the tensors into one fp32 buffer on `dev` and rebind every `.data` to its view of that buffer."""
        flat = torch.empty(max(sum(t.numel() for t in tensors), min_numel), dtype=torch.float32, device=dev)
        off = 0
        with torch.no_grad():
            for t in tensors:
                k = t.numel()
                flat[off:off + k].copy_(t.detach().reshape(-1))
                t.data = flat[off:off + k].view(t.shape)
                off += k
        return flat

    def flatten(self):
        """(Re)build the flat buffers on the parameters' current device and rebind every Parameter
        to a view of them. Called at construction and after every Module._apply (to(), cuda(), ...)."""
        dev = self.trainable[0].device
        self.flat = self._gather_views(self.trainable, dev)
        self.qflat = self._gather_views(self.frozen, dev, 1)
        self.flat_param = torch.nn.Parameter(self.flat, requires_grad=True)
        self.flat_param.register_post_accumulate_grad_hook(self._on_flat_grad)
        self._offsets = []
        off = 0
        for p in self.trainable:
            self._offsets.append((off, p.numel()))
            off += p.numel()
        self._packed = None
        self._rng_state = None

    def _on_flat_grad(self, fp):
        if self.grad_mode != "per_param" or fp.grad is None:
            return
        g = fp.grad
        for p, (off, k) in zip(self.trainable, self._offsets):
            p.grad = g[off:off + k].view(p.shape)

    def sync_grad_state(self):
        """The Trainer zeroes per-layer grads (set_to_none); drop the stale flat grad with them."""
        if self.bind and self.grad_mode == "per_param" and self.trainable[0].grad is None:
            self.flat_param.grad = None

    # ------------------------------------------------------------------ device helpers
    def _check_inputs(self, x, h, what):
        cfg = self.cfg
        if x.dim() != 2 or x.shape[1] != cfg.size:
            raise ValueError(f"bcnf_amd {what}: expected (N, {cfg.size}) input, got {tuple(x.shape)}")
        if h.dim() != 2 or h.shape[1] != cfg.n_conditions:
            raise ValueError(f"bcnf_amd {what}: expected features (N, {cfg.n_conditions}), got {tuple(h.shape)}")
        self._check_device(x, h)

    def _check_forward(self, y, h):
        self._check_inputs(y, h, "forward")
        if h.shape[0] != y.shape[0]:
            raise ValueError(f"bcnf_amd forward: {y.shape[0]} samples but {h.shape[0]} feature rows")

    def _check_device(self, *tensors):
        for t in tensors:
            if t is None:
                continue
            if not t.is_cuda:
                raise RuntimeError("bcnf_amd runs the coupling stack on the MI355X HIP kernels only; "
                                   "move the model and inputs to a ROCm device (model.to('cuda')).")
            if t.dtype != torch.float32:
                raise TypeError(f"bcnf_amd coupling stack is fp32-only, got {t.dtype}")
        if self.flat is None or self.flat.device.type != "cuda":
            raise RuntimeError("bcnf_amd: model parameters are not on the GPU; call model.to('cuda') first.")

    # ------------------------------------------------------------------ pack policy
    def packed(self, fresh: bool = False):
        """The family's packed parameter buffer (`_pack_into`). Re-packed on every call unless inside `reuse_pack()`
        (parameters change in place after each optimizer step; `.data`-rebound views do not share one reliable
        version counter, so no staleness heuristics). Under HIP-graph capture the pack is a graph node."""
        if fresh and not self._pack_frozen:
            # private copy that a later forward cannot overwrite before this one's backward runs
            out = self._empty_pack()
            self._pack_into(out)
            return out
        if self._packed is None:
            self._packed = self._empty_pack()
        if not self._pack_frozen:
            self._pack_into(self._packed)
        return self._packed

    def _empty_pack(self):
        return torch.empty(self._packed_bytes() // 4, dtype=torch.float32, device=self.flat.device)

    class _Reuse:
        def __init__(self, stack):
            self.stack = stack

        def __enter__(self):
            self.stack.packed()
            self.prev = self.stack._pack_frozen
            self.stack._pack_frozen = True
            return self.stack

        def __exit__(self, *exc):
            self.stack._pack_frozen = self.prev

    def reuse_pack(self):
        """Pack once and reuse it for every launch inside the block (e.g. all chunks of sample())."""
        return StackBase._Reuse(self)

    # ------------------------------------------------------------------ dropout RNG state
    # A feature network bound to this stack draws its dropout from the same (seed, offset) and leaves the advance to
    # the coupling launch that follows in the step (feature_network.py). True between such a feature draw and the
    # next coupling launch: a second feature draw before any coupling launch (the feature network run on its own)
    # advances the offset itself first (feature_rng_state), so repeated standalone calls draw fresh masks.
    _feature_pending = False

    def _dropping(self, training: bool) -> bool:
        """Whether a launch in this mode draws dropout masks (and so takes an rng_state())."""
        return bool(training) and self.cfg.dropout > 0.0

    def rng_state(self):
        """Device-resident (seed, offset) for the in-kernel Philox dropout; the offset is bumped by a
        device-side add after every training forward, so HIP-graph replays draw fresh masks."""
        self._feature_pending = False          # a coupling launch takes this step's offset
        return self._rng_tensor()

    @staticmethod
    def _advance_rng(rng):
        """The post-launch offset bump of a launch that drew masks from `rng` (None: it drew none)."""
        if rng is not None:
            rng[1:2].add_(1)

    def feature_rng_state(self):
        """The state a bound feature network's fused dropout draws from, when the coupling launch of the step will
        advance it (a feature draw not followed by a coupling launch advances it at the next one)."""
        t = self._rng_tensor()
        if self._feature_pending:
            t[1:2].add_(1)
        self._feature_pending = True
        return t

    def _rng_tensor(self):
        if self._rng_state is None:
            seed = self.seed
            if seed is None:
                seed = (torch.cuda.initial_seed() * 0x9E3779B97F4A7C15 + id(self)) & ((1 << 62) - 1)
            self._rng_state = torch.tensor([seed, 0], dtype=torch.int64, device=self.flat.device)
        return self._rng_state

    def set_seed(self, seed: int):
        self.seed = int(seed)
        self._rng_state = None

    # ------------------------------------------------------------------ TrainStep's hooks
    # Hybrid loss (_HybridNLL). hybrid_cot = (cotangent of vals, [c0 / (1 + w), c1, 0], w): TrainStep's constant
    # cotangent and its stack form, so the backward launches no kernel to derive one from the other. hybrid_judge:
    # False in a data-parallel TrainStep, where the all-reduced loss is judged (bcnf_guard_check_global), not the shard's.
    hybrid_cot = None
    hybrid_judge = True

    def hybrid_guard(self):
        return self.guard if self.hybrid_judge else None

    # ------------------------------------------------------------------ inverse
    def _check_ldj(self, training: bool):
        """The density of a draw exists only where the inverse is the forward's inverse and deterministic."""
        if self.cfg.two_way:
            raise ValueError("bcnf_amd: no log-density for two_way stacks: the reference's two_way inverse "
                             "(cnf.py:198-213) is not the inverse of its forward")
        if self._dropping(training):
            raise ValueError("bcnf_amd: no log-density for a training-mode inverse with dropout > 0 (the draw is not "
                             "deterministic); call model.eval() first")

    def launch_inverse(self, z, h, cond_index=None, training: bool = False, want_ldj: bool = False):
        """y = inverse(z | h). want_ldj=True (eval, one-way): (y, ldj, log_prob) with ldj = log|det dz/dy| at the
        returned y (what launch_forward(y, h) gives) and log_prob = -0.5 |z|^2 + ldj - D/2 log 2pi, from the same
        launch; y is bit-identical to the plain call. The family supplies `_inverse_scratch_bytes`,
        `_native_inverse` and `_native_inverse_logdet`."""
        if want_ldj:
            self._check_ldj(training)
        self._check_inputs(z, h, "inverse")
        n = z.shape[0]
        if cond_index is None and h.shape[0] != n:
            raise ValueError(f"bcnf_amd inverse: {n} latents but {h.shape[0]} feature rows and no cond_index")
        y = torch.empty_like(z)
        rng = self.rng_state() if self._dropping(training) else None
        if cond_index is not None:
            cond_index = cond_index.to(device=z.device, dtype=torch.int64).contiguous()
        sb = self._inverse_scratch_bytes(h.shape[0], n)
        scratch = torch.empty(max(sb // 4, 1), dtype=torch.float32, device=z.device)
        if want_ldj:
            ldj = torch.empty(n, dtype=torch.float32, device=z.device)
            logp = torch.empty(n, dtype=torch.float32, device=z.device)
            return self._native_inverse_logdet(z, h, cond_index, y, training, ldj, logp, scratch)
        self._native_inverse(z, h, cond_index, y, training, rng, scratch)
        self._advance_rng(rng)
        return y

    # ------------------------------------------------------------------ kernel timing
    @staticmethod
    def _time_calls(calls, iters):
        """{key: (entry point, *arguments)} -> {key: average device time (us)}, measured with HIP events on the launch
        stream around `iters` back-to-back launches of the same (idempotent) call, so host launch latency is
        amortised."""
        out = {}
        for key, launch in calls.items():
            N.call(*launch)                           # warm (code object, LDS attributes)
            e0 = torch.cuda.Event(enable_timing=True)
            e1 = torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(iters):
                N.call_raw(*launch)
            e1.record()
            torch.cuda.synchronize()
            out[key] = e0.elapsed_time(e1) * 1e3 / iters
        return out


class FusedStack(StackBase):
    """The register-resident small family: drives the HIP kernels of bcnf_stack*.hip. A training launch is built by a
    `_*_call(s)` method, which validates, allocates and returns ((entry point, *arguments), results); `launch_*` runs
    it and `time_kernels` times the same tuples."""

    @property
    def supported(self) -> bool:
        return bool(N.call_raw("bcnf_stack_supported", self._pdesc))

    def counts(self):
        rc, (a, b) = N.query_status("bcnf_param_count", self._pdesc, outs=2)
        N.check(rc, "bcnf_param_count")
        return a, b

    def flatten(self):
        super().flatten()
        self._raw_tables = {}

    def _packed_bytes(self):
        return N.query_i64("bcnf_packed_bytes", self._pdesc)

    def _pack_into(self, out):
        N.call("bcnf_pack_params", self._pdesc, self.flat, self.qflat, out, N.stream_handle(self.flat.device))

    def workspace_bytes(self, batch: int, training: bool):
        wb = N.query_i64("bcnf_workspace_bytes", self._pdesc, batch, training)
        sb = N.query_i64("bcnf_slab_bytes", self._pdesc, batch)
        return wb, sb

    # ------------------------------------------------------------------ launches
    def _forward_buffers(self, y, training):
        """z, ldj, the dropout state (the pass's one rng_state() draw; None without dropout) and the workspace."""
        B = y.shape[0]
        z = torch.empty_like(y)
        ldj = torch.empty(B, dtype=torch.float32, device=y.device)
        rng = self.rng_state() if self._dropping(training) else None
        wb, _ = self.workspace_bytes(B, training)      # also holds the condition projection
        ws = torch.empty(max(wb // 4, 1), dtype=torch.float32, device=y.device)
        return z, ldj, rng, ws

    def _backward_buffers(self, h, slab_bytes, want_dy, want_dh):
        slab = torch.empty(max(slab_bytes // 4, 1), dtype=torch.float32, device=h.device)
        dparams = torch.empty_like(self.flat)
        dh = torch.empty_like(h) if want_dh else None
        dy = torch.empty((h.shape[0], self.cfg.size), dtype=torch.float32, device=h.device) if want_dy else None
        return slab, dparams, dh, dy

    def launch_forward(self, y, h, training: bool, save: bool, want_logp: bool = False):
        self._check_forward(y, h)
        B = y.shape[0]
        z, ldj, rng, ws = self._forward_buffers(y, training)
        logp = torch.empty(B, dtype=torch.float32, device=y.device) if want_logp else None
        pk = self.packed(fresh=save)
        N.call("bcnf_stack_forward", self._pdesc, pk, y, h, B, z, ldj, logp, training, rng, ws, save,
               N.stream_handle(y.device))
        self._advance_rng(rng)
        return z, ldj, logp, (ws, pk)

    def launch_backward(self, h, dz, dldj, training: bool, saved, want_dy: bool, want_dh: bool):
        ws, pk = saved
        B = h.shape[0]
        slab, dparams, dh, dy = self._backward_buffers(h, self.workspace_bytes(B, training)[1], want_dy, want_dh)
        N.call("bcnf_stack_backward", self._pdesc, pk, h, dz, dldj, B, training, ws, dy, None, None, slab,
               N.stream_handle(h.device))
        N.call(*self._tail_call(h, saved, slab, training, dh, dparams))
        return dy, dh, dparams

    def _tail_call(self, h, saved, slab, training, dh, dparams):
        """dL/dh and the deterministic parameter-gradient reduction after a backward launch (one fused tail
        launch + the split-K finish)."""
        ws, pk = saved
        return ("bcnf_backward_tail", self._pdesc, pk, slab, h, ws, h.shape[0], training, dh, dparams,
                N.stream_handle(h.device))

    def _nll_forward_call(self, y, h, training, finalize):
        self._check_forward(y, h)
        B = y.shape[0]
        if B == 0:
            raise ValueError("bcnf_amd: the NLL of an empty batch is undefined")
        z, ldj, rng, ws = self._forward_buffers(y, training)
        vals = torch.empty(3, dtype=torch.float32, device=y.device)
        pk = self.packed(fresh=True)
        launch = ("bcnf_nll_forward", self._pdesc, pk, y, h, B, z, ldj, training, rng, ws, finalize, vals,
                  self.guard if finalize else None, N.stream_handle(y.device))
        return launch, (z, ldj, vals, (ws, pk))

    def launch_nll_forward(self, y, h, training: bool, finalize: bool = True):
        """Stack forward fused with inn_nll_loss (trainer.py:260-266): returns z, ldj, vals=[loss, nll, mse]
        and the saved state for launch_nll_backward. With finalize=False the loss reduction and the
        dropout-RNG advance are deferred to the backward (vals is valid only after it)."""
        launch, out = self._nll_forward_call(y, h, training, finalize)
        N.call(*launch)
        return out

    def _nll_backward_call(self, rows, z, dvals, training, saved, slab, dy, finalize_into):
        """The fused NLL backward over `rows` (the features h, or the folded pass's x). finalize_into: the deferred
        loss reduction and dropout-RNG advance of the forward run in this launch."""
        ws, pk = saved
        rng = self.rng_state() if (finalize_into is not None and self._dropping(training)) else None
        return ("bcnf_nll_backward", self._pdesc, pk, rows, z, dvals, rows.shape[0], training, ws, dy, None, None, slab,
                finalize_into, rng, self.guard if finalize_into is not None else None, N.stream_handle(rows.device))

    def _nll_backward_calls(self, h, z, dvals, training, saved, want_dy, want_dh, finalize_into=None):
        slab, dparams, dh, dy = self._backward_buffers(h, self.workspace_bytes(h.shape[0], training)[1], want_dy,
                                                       want_dh)
        return ((self._nll_backward_call(h, z, dvals, training, saved, slab, dy, finalize_into),
                 self._tail_call(h, saved, slab, training, dh, dparams)), (dy, dh, dparams))

    def launch_nll_backward(self, h, z, dvals, training: bool, saved, want_dy: bool, want_dh: bool,
                            finalize_into=None):
        launches, out = self._nll_backward_calls(h, z, dvals, training, saved, want_dy, want_dh, finalize_into)
        for launch in launches:
            N.call(*launch)
        return out

    # ------------------------------------------------------------------ folded linear feature network
    def fold_supported(self, in_features: int) -> bool:
        """Whether a single nn.Linear [in_features -> n_conditions] feature network can be folded into the
        condition projection (bcnf_pack_params_fold; include/bcnf_amd.h)."""
        return N.query_status("bcnf_fold_bytes", self._pdesc, int(in_features))[0] == N.OK

    # bcnf_fold_train_forward (the pack-free folded forward, one launch) where its table applies; False: always the
    # two-launch form (pack + fold, then the forward), which tests and tools set on an instance as a reference
    use_raw_forward = True

    def raw_table(self, X: int):
        """The device copy of bcnf_fold_raw_table for in_features X (built once per device), or None where the
        pack-free forward does not apply."""
        if not self.use_raw_forward:
            return None
        dev = self.flat.device
        key = (X, str(dev))
        if key not in self._raw_tables:
            if torch.cuda.is_current_stream_capturing():
                return None                     # no host -> device copy inside a graph capture
            rc, (nb,) = N.query_status("bcnf_fold_raw_table_bytes", self._pdesc, X)
            if rc != N.OK:
                self._raw_tables[key] = None
            else:
                host = torch.empty(nb // 4, dtype=torch.int32)
                N.call("bcnf_fold_raw_table", self._pdesc, X, host)
                self._raw_tables[key] = host.to(dev)
        return self._raw_tables[key]

    def _fold_forward_calls(self, y, x, wf, bf, training, finalize, gather):
        self._check_device(y, x, wf, bf)
        B, X = x.shape
        if y.dim() != 2 or y.shape != (B, self.cfg.size):
            raise ValueError(f"bcnf_amd folded forward: y {tuple(y.shape)} vs x {tuple(x.shape)}")
        if B == 0:
            raise ValueError("bcnf_amd: the NLL of an empty batch is undefined")
        stream = N.stream_handle(y.device)
        pk = self._empty_pack()
        table = self.raw_table(X)
        z, ldj, rng, ws = self._forward_buffers(y, training)
        vals = torch.empty(3, dtype=torch.float32, device=y.device)
        guard = self.guard if finalize else None
        if table is not None:
            launches = (("bcnf_fold_train_forward", self._pdesc, self.flat, self.qflat, table, wf, bf, X, gather, y, x,
                         x.stride(0), B, pk, z, ldj, training, rng, ws, finalize, vals, guard, stream),)
        else:
            fold = torch.empty(N.query_i64("bcnf_fold_bytes", self._pdesc, X) // 4, dtype=torch.float32,
                               device=y.device)
            launches = (("bcnf_pack_params_fold", self._pdesc, self.flat, self.qflat, wf, bf, X, pk, fold, gather,
                         stream),
                        ("bcnf_fold_nll_forward", self._pdesc, pk, fold, X, y, x, x.stride(0), B, z, ldj, training,
                         rng, ws, finalize, vals, guard, stream))
        return launches, (z, ldj, vals, (ws, pk))

    def launch_fold_nll_forward(self, y, x, wf, bf, training: bool, finalize: bool = True, gather=None):
        """launch_nll_forward with h = x Wf^T + bf never formed as a tensor. Pack-free form (raw_table applies):
        ONE launch, bcnf_fold_train_forward, builds its records from the parameters and computes h of its rows
        on the fly. Otherwise the pack launch also folds the Linear into the projection weights (Wc = W1h Wf,
        bc = b1 + W1h bf) and the projection runs on x. gather (an N.BcnfGather2 that fills y and x): the batch
        gather runs inside the first launch."""
        launches, out = self._fold_forward_calls(y, x, wf, bf, training, finalize, gather)
        for launch in launches:
            N.call(*launch)
        return out

    # A BcnfFoldAdam for the next folded backward (TrainStep, multi-step graphs): consumed by that launch.
    pending_adam = None
    # (bucket, (flat offset, feature W offset, feature b offset)): TrainStep's data-parallel gradient bucket, which
    # the folded backward writes its gradients into.
    grad_bucket = None

    def _fold_backward_calls(self, x, z, dvals, wf, bf, training, saved, want_feat, finalize_into=None, adam=None):
        ws, pk = saved
        B, X = x.shape
        sb = N.query_i64("bcnf_fold_slab_bytes", self._pdesc, X, B)
        slab = torch.empty(max(sb // 4, 1), dtype=torch.float32, device=x.device)
        gb = self.grad_bucket
        if gb is not None and want_feat:
            # data parallel (TrainStep): the gradients land in the all-reduce bucket itself, as fresh views that
            # autograd adopts as .grad, so no bucket copy follows the backward
            bucket, offs = gb
            dparams = bucket.narrow(0, offs[0], self.flat.numel()).view_as(self.flat)
            dwf = bucket.narrow(0, offs[1], wf.numel()).view_as(wf)
            dbf = bucket.narrow(0, offs[2], bf.numel()).view_as(bf) if bf is not None else None
        else:
            dparams = torch.empty_like(self.flat)
            dwf = torch.empty_like(wf) if want_feat else None
            dbf = torch.empty_like(bf) if (want_feat and bf is not None) else None
        tail = ("bcnf_fold_backward_tail", self._pdesc, pk, slab, x, x.stride(0), X, wf, bf, ws, B, training, dparams,
                dwf, dbf, adam, N.stream_handle(x.device))
        return ((self._nll_backward_call(x, z, dvals, training, saved, slab, None, finalize_into), tail),
                (dparams, dwf, dbf))

    def launch_fold_nll_backward(self, x, z, dvals, wf, bf, training: bool, saved, want_feat: bool,
                                 finalize_into=None, adam=None):
        """Fused NLL backward of the folded pass: (dparams, dWf, dbf); no dL/dh, no dL/dx. adam (an
        N.BcnfFoldAdam): the optimizer update of every parameter runs inside the backward tail."""
        launches, out = self._fold_backward_calls(x, z, dvals, wf, bf, training, saved, want_feat, finalize_into, adam)
        for launch in launches:
            N.call(*launch)
        return out

    @torch.no_grad()
    def time_kernels(self, y, h, training: bool = True, iters: int = 20, fold=None):
        """Average device time (us) of each launch of one NLL training pass (_time_calls), the reduction deferred and
        never run, so no call advances the dropout offset: 'k_forward' (k_hp + k_forward), 'k_backward' (the backward
        kernel alone) and 'tail' (dh + slab reduce + W1 condition part). fold = (x, Wf, bf): the folded path instead
        -- 'k_pack_fold' (pack + fold; absent where the pack-free forward applies), 'k_forward' (k_hp on x +
        k_forward), 'k_backward', 'tail' (slab reduce + split-K on x, Gx reduce, dW1h / dWf / dbf)."""
        if fold is None:
            forward, (z, _, _, saved) = self._nll_forward_call(y, h, training, finalize=False)
            (backward, tail), _ = self._nll_backward_calls(h, z, None, training, saved, want_dy=False, want_dh=True)
            calls = {"k_forward": forward}
        else:
            x, wf, bf = fold
            forwards, (z, _, _, saved) = self._fold_forward_calls(y, x, wf, bf, training, finalize=False, gather=None)
            (backward, tail), _ = self._fold_backward_calls(x, z, None, wf, bf, training, saved, want_feat=True)
            calls = dict(zip(("k_pack_fold", "k_forward")[-len(forwards):], forwards))
        calls.update(k_backward=backward, tail=tail)
        return self._time_calls(calls, iters)

    # ------------------------------------------------------------------ inverse (StackBase.launch_inverse)
    def _inverse_scratch_bytes(self, feature_rows, n):
        return N.query_i64("bcnf_inverse_scratch_bytes", self._pdesc, feature_rows)

    def _native_inverse(self, z, h, cond_index, y, training, rng, scratch):
        N.call("bcnf_stack_inverse", self._pdesc, self.packed(), z, h, h.shape[0], cond_index, z.shape[0], y, training,
               rng, scratch, N.stream_handle(z.device))

    def _native_inverse_logdet(self, z, h, cond_index, y, training, ldj, logp, scratch):
        N.call("bcnf_stack_inverse_logdet", self._pdesc, self.packed(), z, h, h.shape[0], cond_index, z.shape[0], y,
               ldj, logp, scratch, N.stream_handle(z.device))
        return y, ldj, logp


class _StackForward(torch.autograd.Function):
    """z, ldj = stack(y, h). Backward runs the fused HIP backward once and returns dL/dy, dL/dh and the
    whole flat parameter gradient (one AccumulateGrad for `flat_param`)."""

    @staticmethod
    def forward(ctx, y, h, flat_param, stack: StackBase, training: bool):
        needs = ctx.needs_input_grad
        save = any(needs[:3])
        z, ldj, _, saved = stack.launch_forward(y, h, training, save=save)
        ctx.stack = stack
        ctx.training = training
        ctx.saved = saved
        ctx.save_for_backward(h)
        return z, ldj

    @staticmethod
    def backward(ctx, dz, dldj):
        (h,) = ctx.saved_tensors
        stack = ctx.stack
        if dz is not None:
            dz = dz.contiguous()
        if dldj is not None:
            dldj = dldj.contiguous()
        need_y, need_h, need_p = ctx.needs_input_grad[0], ctx.needs_input_grad[1], ctx.needs_input_grad[2]
        dy, dh, dparams = stack.launch_backward(h, dz, dldj, ctx.training, ctx.saved, want_dy=need_y, want_dh=need_h)
        return dy, dh, (dparams if need_p else None), None, None


class _StackNLL(torch.autograd.Function):
    """vals = [loss, nll, mse] of inn_nll_loss(stack(y, h)) in one fused launch; backward is the fused NLL
    backward (no dz / dldj tensors, no elementwise loss kernels)."""

    @staticmethod
    def forward(ctx, y, h, flat_param, stack: StackBase, training: bool, defer: bool):
        z, _, vals, saved = stack.launch_nll_forward(y, h, training, finalize=not defer)
        ctx.stack = stack
        ctx.training = training
        ctx.saved = saved
        ctx.defer = defer
        ctx.save_for_backward(h, z, vals)
        return vals

    @staticmethod
    def backward(ctx, dvals):
        h, z, vals = ctx.saved_tensors
        need_y, need_h, need_p = ctx.needs_input_grad[0], ctx.needs_input_grad[1], ctx.needs_input_grad[2]
        dy, dh, dparams = ctx.stack.launch_nll_backward(h, z, dvals.contiguous(), ctx.training, ctx.saved,
                                                        want_dy=need_y, want_dh=need_h,
                                                        finalize_into=vals if ctx.defer else None)
        return dy, dh, (dparams if need_p else None), None, None, None


def stack_nll(stack: StackBase, y, h, training: bool, defer: bool = False):
    """[loss, nll, mse] (mse = 0, hybrid_weight = 0) of the Trainer's loss on the fused stack. defer=True
    (for a backward that certainly follows, e.g. TrainStep) lets the backward do the loss reduction and
    the dropout-RNG advance: one launch less, but vals is only valid after the backward."""
    y = y.contiguous()
    h = h.contiguous()
    stack.sync_grad_state()
    params_grad = stack.trainable[0].requires_grad
    fp = stack.flat_param
    if torch.is_grad_enabled() and (params_grad or y.requires_grad or h.requires_grad):
        return _StackNLL.apply(y, h, fp if params_grad else fp.detach(), stack, training, defer)
    return stack.launch_nll_forward(y, h, training)[2]


def head_workspace(B: int, K: int, D: int, device):
    """Caller-owned workspace of the prediction-head kernels (bcnf_head_work_bytes): residual, MSE partials, split-K
    partials of dW / dbias."""
    return torch.empty(N.query_i64("bcnf_head_work_bytes", B, K, D) // 4, dtype=torch.float32, device=device)


def launch_head_forward(h, wp, bp, y, work):
    """r = h Wp^T + bp - y and the squared-error partials into `work` (bcnf_head_mse_forward)."""
    B, K = h.shape
    N.call("bcnf_head_mse_forward", h, h.stride(0), K, wp, bp, y, B, y.shape[1], work, N.stream_handle(h.device))


def launch_head_backward(h, wp, work, dvals, weight: float, D: int, dwp, dbp, dh, accumulate: bool):
    """dWp, dbp and dL/dh (added into `dh` with accumulate) of w / (1 + w) * mse (bcnf_head_mse_backward)."""
    B, K = h.shape
    N.call("bcnf_head_mse_backward", h, h.stride(0), K, wp, work, dvals, weight, B, D, dwp, dbp, dh,
           dh.stride(0) if dh is not None else K, accumulate, N.stream_handle(h.device))


def launch_hybrid_finalize(vals, work, B: int, D: int, weight: float, guard):
    """vals = [nll, nll, 0] -> [(nll + w mse) / (1 + w), nll, mse] (bcnf_hybrid_finalize)."""
    N.call("bcnf_hybrid_finalize", vals, work, B, D, weight, guard, N.stream_handle(vals.device))


class _HybridNLL(torch.autograd.Function):
    """vals = [loss, nll, mse] of the Trainer's hybrid loss (trainer.py:261-269), loss = (nll + w mse) / (1 + w) with
    mse = MSE(h Wp^T + bp, y), as ONE node: the fused NLL forward of the stack's family + the head forward; backward =
    the stack's NLL backward with cotangent [dv0 / (1 + w), dv1, 0], the head backward adding its dL/dh into the
    stack's, and (deferred reduction) the finalize of all three values."""

    @staticmethod
    def forward(ctx, y, h, flat_param, wp, bp, stack: StackBase, training: bool, defer: bool, weight: float):
        z, _, vals, saved = stack.launch_nll_forward(y, h, training, finalize=not defer)
        B, D = y.shape
        work = head_workspace(B, h.shape[1], D, y.device)
        launch_head_forward(h, wp, bp, y, work)
        if not defer:
            launch_hybrid_finalize(vals, work, B, D, weight, stack.hybrid_guard())
        ctx.stack, ctx.training, ctx.saved, ctx.defer, ctx.weight, ctx.work = stack, training, saved, defer, weight, work
        ctx.has_bias = bp is not None
        ctx.save_for_backward(h, z, vals, wp)
        return vals

    @staticmethod
    def backward(ctx, dvals):
        h, z, vals, wp = ctx.saved_tensors
        stack, w, work = ctx.stack, ctx.weight, ctx.work
        need_y, need_h, need_p, need_w, need_b = ctx.needs_input_grad[:5]
        dvals = dvals.contiguous()
        B, D = z.shape
        hc = stack.hybrid_cot        # TrainStep: (its constant cotangent, that cotangent's stack form)
        if hc is not None and hc[2] == w and dvals.data_ptr() == hc[0].data_ptr():
            cot = hc[1]
        else:
            cot = dvals * dvals.new_tensor([1.0 / (1.0 + w), 1.0, 0.0])
        dy, dh, dparams = stack.launch_nll_backward(h, z, cot, ctx.training, ctx.saved, want_dy=need_y,
                                                    want_dh=need_h, finalize_into=vals if ctx.defer else None)
        dwp = torch.empty_like(wp) if need_w else None
        dbp = torch.empty(D, dtype=torch.float32, device=wp.device) if (need_b and ctx.has_bias) else None
        if need_h or need_w or dbp is not None:
            launch_head_backward(h, wp, work, dvals, w, D, dwp, dbp, dh, accumulate=True)
        if need_y:       # d mse / dy = -e (rare: y is data); e = (2 g / (B D)) r, r = the workspace's first B * D floats
            g = dvals[0] * (w / (1.0 + w)) + dvals[2]
            dy = dy - (2.0 * g / (B * D)) * work[:B * D].view(B, D)
        if ctx.defer:
            launch_hybrid_finalize(vals, work, B, D, w, stack.hybrid_guard())
        return dy, dh, (dparams if need_p else None), dwp, dbp, None, None, None, None


def stack_hybrid(stack: StackBase, y, h, wp, bp, weight: float, training: bool, defer: bool = False):
    """[loss, nll, mse] of the hybrid loss on the fused stack + head kernels. h is materialised (the head reads it), so
    neither family's feature fold applies. Without grad: finalized values (the Trainer's validation triple)."""
    y = y.contiguous()
    h = h.contiguous()
    stack._check_device(y, h, wp, bp)
    if tuple(wp.shape) != (y.shape[1], h.shape[1]) or not wp.is_contiguous() or \
            (bp is not None and not bp.is_contiguous()):
        raise ValueError(f"bcnf_amd hybrid loss: prediction head {tuple(wp.shape)} does not map features "
                         f"{tuple(h.shape)} to {tuple(y.shape)}")
    stack.sync_grad_state()
    params_grad = stack.trainable[0].requires_grad
    fp = stack.flat_param
    any_grad = params_grad or y.requires_grad or h.requires_grad or wp.requires_grad or \
        (bp is not None and bp.requires_grad)
    if torch.is_grad_enabled() and any_grad:
        return _HybridNLL.apply(y, h, fp if params_grad else fp.detach(), wp, bp, stack, training, defer,
                                float(weight))
    z, _, vals, _ = stack.launch_nll_forward(y, h, training)
    B, D = y.shape
    work = head_workspace(B, h.shape[1], D, y.device)
    launch_head_forward(h, wp, bp, y, work)
    launch_hybrid_finalize(vals, work, B, D, float(weight), stack.hybrid_guard())
    return vals


class _FoldNLL(torch.autograd.Function):
    """_StackNLL with the feature network's single nn.Linear folded into the condition projection: inputs
    (y, x, Wf, bf, flat_param); gradients for Wf, bf and flat_param (not for y or x)."""

    @staticmethod
    def forward(ctx, y, x, wf, bf, flat_param, stack: FusedStack, training: bool, defer: bool, gather):
        z, _, vals, saved = stack.launch_fold_nll_forward(y, x, wf, bf, training, finalize=not defer, gather=gather)
        ctx.stack = stack
        ctx.training = training
        ctx.saved = saved
        ctx.defer = defer
        ctx.save_for_backward(x, wf, bf, z, vals)
        return vals

    @staticmethod
    def backward(ctx, dvals):
        x, wf, bf, z, vals = ctx.saved_tensors
        need = ctx.needs_input_grad
        adam, ctx.stack.pending_adam = ctx.stack.pending_adam, None
        dparams, dwf, dbf = ctx.stack.launch_fold_nll_backward(x, z, dvals.contiguous(), wf, bf, ctx.training,
                                                               ctx.saved, want_feat=need[2] or need[3] or
                                                               adam is not None,
                                                               finalize_into=vals if ctx.defer else None, adam=adam)
        return (None, None, dwf if need[2] else None, dbf if need[3] else None, dparams if need[4] else None,
                None, None, None, None)


def stack_nll_fold(stack: FusedStack, y, x, wf, bf, training: bool, defer: bool = False, gather=None):
    """stack_nll(stack, y, x Wf^T + bf) without forming the features (see launch_fold_nll_forward). gather: the
    batch gather that fills y and x, run inside the pack launch (TrainStep); y and x are then its outputs."""
    if gather is not None and not (y.is_contiguous() and x.stride(1) == 1):
        raise ValueError("bcnf_amd: a deferred gather needs its own (contiguous) output buffers")
    y = y.contiguous()
    if x.stride(1) != 1 or x.stride(0) < x.shape[1]:
        x = x.contiguous()              # rows may be padded (ldx = stride(0) > X: TrainStep's zero-padded pool)
    stack.sync_grad_state()
    params_grad = stack.trainable[0].requires_grad
    fp = stack.flat_param
    feat_grad = wf.requires_grad or (bf is not None and bf.requires_grad)
    if torch.is_grad_enabled() and (params_grad or feat_grad):
        return _FoldNLL.apply(y, x, wf, bf, fp if params_grad else fp.detach(), stack, training, defer, gather)
    return stack.launch_fold_nll_forward(y, x, wf, bf, training, gather=gather)[2]


class _StackInverse(torch.autograd.Function):
    @staticmethod
    def forward(ctx, z, h, stack: StackBase, cond_index, training: bool, want_ldj: bool = False):
        out = stack.launch_inverse(z, h, cond_index, training, want_ldj)
        if want_ldj:
            ctx.mark_non_differentiable(*out[1:])
        return out

    @staticmethod
    def backward(ctx, dy, *unused):
        raise NotImplementedError("bcnf_amd: CondRealNVP_v2.inverse is not differentiable (sampling path); "
                                  "run it under torch.no_grad().")


def _set_standalone_params(stack: StackBase, flat, device):
    stack.flat = flat.detach().contiguous()
    if stack.qflat is None or stack.qflat.device != device:
        stack.qflat = torch.zeros(1, dtype=torch.float32, device=device)


def stack_forward(stack: StackBase, y, h, training: bool, flat=None):
    y = y.contiguous()
    h = h.contiguous()
    if flat is not None:
        _set_standalone_params(stack, flat, y.device)
        fp = flat
        params_grad = flat.requires_grad
    else:
        stack.sync_grad_state()
        params_grad = stack.trainable[0].requires_grad
        fp = stack.flat_param
    if torch.is_grad_enabled():
        if params_grad or y.requires_grad or h.requires_grad:
            return _StackForward.apply(y, h, fp if params_grad else fp.detach(), stack, training)
    z, ldj, _, _ = stack.launch_forward(y, h, training, save=False)
    return z, ldj


def stack_inverse(stack: StackBase, z, h, cond_index=None, training: bool = False, flat=None,
                  want_ldj: bool = False):
    """want_ldj=True: (y, ldj, log_prob) -- see StackBase.launch_inverse."""
    z = z.contiguous()
    h = h.contiguous()
    if flat is not None:
        _set_standalone_params(stack, flat, z.device)
    if torch.is_grad_enabled() and (z.requires_grad or h.requires_grad):
        return _StackInverse.apply(z, h, stack, cond_index, training, want_ldj)
    return stack.launch_inverse(z, h, cond_index, training, want_ldj)
