"""Trainer-semantics training step on the fused kernels, with HIP-graph capture and data parallelism.

`TrainStep.step(y, traj)` performs exactly one `bcnf.train.Trainer._train_batch`
(src/bcnf/train/trainer.py:244-277):

    optimizer.zero_grad()
    z, h = model(y, *conditions, log_det_J=True, return_features=True)
    mse = MSE(prediction_head(h), y) if hybrid_weight > 0 else 0     # configs/runs/hybrid/*: hybrid_weight 1
    nll = inn_nll_loss(z, model.log_det_J)
    loss = (nll + mse * w) / (1 + w)
    loss.backward()
    [data parallel: every gradient packed into one bucket, ONE RCCL all-reduce (mean), grads = bucket views]
    optimizer.step()                                   # Adam
    clip_grad_norm_(parameters, max_norm=1.0)          # after the step, as the reference does
    loss.item(), nll.item(), mse.item()

MI355X specifics:
* hybrid_weight == 0 (configs/runs/old/*): forward + loss are ONE fused launch (`model.nll_loss`,
  bcnf_nll_forward) and loss.backward() is the fused NLL backward + deterministic slab reduce. A feature
  network that is one nn.Linear (trajectory_FC_small) is folded into the condition projection (no h, no
  dL/dh); other feature networks run on the library's MFMA GEMMs / PyTorch-ROCm.
* hybrid_weight > 0 (configs/runs/hybrid/*, half of the reference's run configs): `model.hybrid_loss` -- one
  autograd node: the same fused NLL kernels on the materialised h (no feature fold: the head reads h), the
  prediction head + MSE as HIP kernels (bcnf_head_mse_forward / _backward, the head's dL/dh added into the
  stack's in place) and bcnf_hybrid_finalize for the three logged values. Capture, run_epoch's multi-step
  graphs and the device divergence guard (judging the combined loss) work as for hybrid_weight == 0; the folded
  fused-Adam tail and the in-pack gather stay hybrid_weight == 0 only. `fuse_hybrid = False` keeps the generic
  route (torch nn.Linear + MSELoss + autograd, one replay and one host sync per batch in run_epoch).
* the coupling-stack parameters are ONE flat leaf (model.flat_parameters()); Adam is ONE launch over
  all parameters (bcnf_amd.optim.FusedAdam) that also emits the squared-gradient partials, so the
  clip after the step is one more launch.
* the whole step is captured once into a HIP graph and replayed (world > 1: the RCCL all-reduce runs
  between two captured segments). `step_indexed` also captures the batch gather from a
  device-resident pool (inside the folded path's pack launch), so a replay needs only the index copy.
* `run_epoch` replays 8 device-driven steps per graph. Only the last step of such a graph clips: the
  clip after the step (trainer.py:275) scales gradients the next step's backward overwrites and its norm
  is discarded, so every other step ("hidden") runs Adam with the bookkeeping instead -- on the folded
  path inside the backward tail itself (BcnfFoldAdam), with no Adam launch. run_epoch equals the per-step
  loop bit for bit (tests/test_gpu_train.py).
* the three logged values are stored by the clip launch straight into pinned host memory (a history
  row per batch of the epoch), so no copy node and, with `run_epoch`, no host sync per step: the epoch's
  steps are replayed back to back and the Trainer's per-batch divergence check (trainer.py:168) runs
  on the device (guard, include/bcnf_amd.h), halting the epoch in the state the reference raises in.
* the Adam launches take lr by value, so a captured step holds the rate it was captured with: a scheduler's
  change goes through `set_lr`, which drops the captured graphs for the next step to recapture
  (bcnf_amd/trainer.py calls it after every scheduler step that moved the rate).

This module holds the step itself; the device pool with its epoch walk and graph schedule live in bcnf_amd/epoch.py
(shared with the validation pass), the data-parallel gradient bucket in bcnf_amd/bucket.py.
"""
from __future__ import annotations

import contextlib
import math

import torch
import torch.distributed as dist

from bcnf_amd.bucket import GradBucket
from bcnf_amd.epoch import DevicePool, EpochWalk, check_indices, graph_schedule
from bcnf_amd.errors import TrainingDivergedError
from bcnf_amd.optim import FusedAdam, clip_grad_norm_
from bcnf_amd.utils import inn_nll_loss

GUARD_CHECK, GUARD_DIVERGED, GUARD_HALTED, GUARD_CHECK_GLOBAL, GUARD_WORDS = 0, 1, 2, 3, 4    # include/bcnf_amd.h


class _PackedParameters:
    """The optimizer's view of a feature network with more parameter tensors than one Adam / clip launch takes
    (N.MAX_TENSORS; a Transformer has 16 per block): the member parameters become views of ONE flat parameter, and
    after each backward their gradients are gathered into ONE flat gradient (a torch.cat, capturable) of which each
    member's .grad is then a view -- so the update, the clip after the step, the logged values and the divergence guard
    keep their single-launch form, and p.grad shows the clipped gradient as it does for every other model."""

    def __init__(self, members):
        self.members = list(members)
        dev = self.members[0].device
        flat = torch.empty(sum(p.numel() for p in self.members), dtype=torch.float32, device=dev)
        self.slices = []
        off = 0
        with torch.no_grad():
            for p in self.members:
                n = p.numel()
                flat[off:off + n].copy_(p.detach().reshape(-1))
                p.data = flat[off:off + n].view(p.shape)
                self.slices.append((off, off + n))
                off += n
        self.param = torch.nn.Parameter(flat)
        self.flat_grad = torch.zeros_like(flat)

    def intact(self) -> bool:
        """The members still are the views (Module.to / .float() after the TrainStep was built replaces them)."""
        base = self.param.data_ptr()
        return all(p.data_ptr() == base + 4 * lo for p, (lo, _) in zip(self.members, self.slices))

    def clear(self):
        for p in self.members:
            p.grad = None

    def gather(self):
        grads = [p.grad for p in self.members]
        if any(g is None for g in grads):
            raise RuntimeError("bcnf_amd TrainStep: a feature-network parameter received no gradient")
        torch.cat([g.reshape(-1) for g in grads], out=self.flat_grad)
        for p, (lo, hi) in zip(self.members, self.slices):
            p.grad = self.flat_grad[lo:hi].view(p.shape)
        self.param.grad = self.flat_grad


class _Captured:
    """The captured step: its static input buffers, its graphs and the gradient buffers they own. set_lr drops it."""

    def __init__(self, y, traj, idx):
        self.y, self.traj, self.idx = y, traj, idx      # static inputs (idx: step_indexed's; None for step())
        self.g1 = None          # the step (world > 1: up to the bucket pack; the all-reduce follows, then g2)
        self.vals = None        # g1's logged (loss, nll, mse)
        self.g2 = None          # data parallel: the update segment
        self.g2_hidden = None   # data parallel: update segment without the (unobservable) clip
        self.g21 = None         # data parallel: hidden update + the next step's forward/backward, one graph
        self.single_grads = None   # what .grad shows after a g1 replay
        self.multi = {}         # steps -> (graph, grads): run_epoch's multi-step graphs (world 1)
        self.rebind = False     # .grad currently points at buffers other than the single-step graph's


class TrainStep:
    def __init__(self, model, lr: float = 2e-4, hybrid_weight: float = 0.0, capture: bool = True,
                 max_norm: float = 1.0, process_group=None, overlap_ranges: int = 0):
        # An AnyGLU coupling stack (layer="AnyGLU", reference layers.py:9-31, dev configs) has no fused kernel family:
        # it runs layer by layer (its Linear layers on the library's MFMA GEMMs, autograd), so its step is the same
        # Trainer step run eagerly over model.parameters() -- FusedAdam, the clip after the step, the bucket
        # all-reduce -- without graph capture or the device divergence guard (the loss is checked on the host).
        self.layerwise = getattr(model, "_path", "fused") == "layerwise"
        self.model = model
        self.params = [p for p in model.parameters() if p.requires_grad] if self.layerwise \
            else model.flat_parameters()
        self._packed = None
        from bcnf_amd import _native as N
        if not self.layerwise and len(self.params) > N.MAX_TENSORS and model.n_conditions > 0:
            members = {id(p) for p in model.feature_network_stack.parameters()}
            feature = [p for p in self.params if id(p) in members]
            if feature and all(p.is_cuda and p.dtype == torch.float32 for p in feature):
                self._packed = _PackedParameters(feature)
                self.params = [p for p in self.params if id(p) not in members]
                self.params.insert(1, self._packed.param)
        self.hybrid_weight = float(hybrid_weight)
        self.max_norm = max_norm
        self.capture = capture and not self.layerwise
        self.pg = process_group
        self.world = dist.get_world_size(process_group) if (dist.is_available() and dist.is_initialized()) else 1
        self.opt = FusedAdam(self.params, lr=lr)
        self.mse = torch.nn.MSELoss()
        self.fused_loss = self.hybrid_weight == 0.0
        self._cot_stack = None
        self._cot = None
        self._cap = None        # the captured step (_Captured); None until the first captured step and after set_lr
        self.pool = None        # DevicePool (set_pool)
        self.walk = None        # EpochWalk over the pool (set_epoch): the device-cursor batch walk
        # data parallel: every gradient in one buffer, one all-reduce per step
        self.bucket = GradBucket(self.params, process_group, self.world) if self.world > 1 else None
        self.last_clip_norm = None   # device scalar: total gradient norm before the last observable clip
        # data parallel, wide family: the backward runs in `overlap_ranges` block ranges and each finished range's
        # bucket slice is all-reduced (async) while the rest of the backward runs; eager steps (the collectives are
        # issued between kernel launches, outside any captured graph), joined before the update
        self.overlap_ranges = 0
        from bcnf_amd.wide import WideStack
        if self.world > 1 and overlap_ranges > 0 and isinstance(getattr(model, "fused", None), WideStack):
            self.overlap_ranges = min(int(overlap_ranges), model.fused.cfg.n_blocks)
            self.capture = False
        dev = self.params[0].device
        self._guard = None
        self._hist = None
        self._book = None       # Adam's finished-workgroup counter (bcnf_adam_step_bookkeep)
        if dev.type == "cuda":
            self._guard = torch.zeros(GUARD_WORDS, dtype=torch.int32, device=dev)
            self._book = torch.zeros(1, dtype=torch.int32, device=dev)
            model.fused.guard = self._guard
            self._hist = torch.zeros((1, 3), dtype=torch.float32, pin_memory=True)

    # ------------------------------------------------------------------ step pieces
    def _forward_backward(self, y, traj, gather=None, adam=None):
        if self._packed is not None:
            if not self._packed.intact():
                raise RuntimeError("bcnf_amd TrainStep: the model's feature-network parameters were replaced (moved or "
                                   "cast) after this TrainStep packed them; build a new TrainStep")
            self._packed.clear()
        hooks = self.bucket.stack_hooks(self.model.fused) if self.bucket is not None else contextlib.nullcontext()
        with hooks:
            vals = self._forward_backward_body(y, traj, gather, adam)
        if self._packed is not None:
            self._packed.gather()
        return vals

    def _forward_backward_body(self, y, traj, gather=None, adam=None):
        self.opt.zero_grad(set_to_none=True)
        if self.fused_loss:
            # reduced in the backward launch; a deferred gather runs inside the pack launch
            vals = self.model.nll_loss(y, traj, defer_reduction=True, gather=gather)
            cot = self._cotangent(vals.device)
            if adam is not None:                          # the optimizer step, inside the folded backward tail
                self.model.fused.pending_adam = adam(vals)
            torch.autograd.backward(vals, cot)            # loss.backward()
            if adam is not None and self.model.fused.pending_adam is not None:
                self.model.fused.pending_adam = None
                raise RuntimeError("bcnf_amd TrainStep: the folded backward did not take the fused Adam update")
            return vals.detach()
        if self.hybrid:
            vals = self.model.hybrid_loss(y, traj, hybrid_weight=self.hybrid_weight, defer_reduction=True)
            cot = self._cotangent(vals.device)
            st = self.model.fused
            st.hybrid_cot = (cot, self._cot_stack, self.hybrid_weight)
            st.hybrid_judge = self.world == 1       # data parallel: the all-reduced loss is judged (check_global)
            try:
                torch.autograd.backward(vals, cot)            # loss.backward()
            finally:
                st.hybrid_cot = None
                st.hybrid_judge = True
            return vals.detach()
        z, h = self.model(y, traj, log_det_J=True, return_features=True)
        nll = inn_nll_loss(z, self.model.log_det_J)
        mse = self.mse(self.model.prediction_head(h), y)
        loss = (nll + mse * self.hybrid_weight) / (1 + self.hybrid_weight)
        loss.backward()
        return torch.stack([loss.detach(), nll.detach(), mse.detach()])

    def _cotangent(self, dev):
        """d(loss) / d(loss, nll, mse) for loss.backward() on the three logged values; the hybrid step also keeps the
        coupling stack's share of it, 1 / (1 + w)."""
        if self._cot is None or self._cot.device != dev:
            self._cot = torch.tensor([1.0, 0.0, 0.0], device=dev)
            if self.hybrid:
                self._cot_stack = torch.tensor([1.0 / (1.0 + self.hybrid_weight), 0.0, 0.0], device=dev)
        return self._cot

    def _update(self, vals=None, clip: bool = True, epoch_book: bool = True):
        """Adam, then clip_grad_norm_ after the step (trainer.py:273-275); the clip launch also advances the
        Adam step count and, in epoch mode, the batch cursor, and stores the logged values into the pinned
        history (end-of-step bookkeeping, no extra launch). epoch_book=False: a batch from outside the epoch
        order (step_indexed while an order is set) -- no cursor advance and no history row."""
        if self.bucket is not None and vals is not None:
            vals = self.bucket.gvals        # every rank logs the global values and halts on the same step
            self.bucket.check_global(self._guard)
        cursor = self._cursor() if epoch_book else None
        log = (vals, self._hist) if (vals is not None and self._hist is not None and epoch_book) else None
        if not clip:
            # a step inside a multi-step graph that the next step's backward follows: its clip-after-step
            # would only scale gradients that are overwritten before anyone can read them (the reference
            # discards the norm), so Adam's last workgroup does the step's bookkeeping and no clip runs
            self.opt.step(guard=self._guard, bookkeep=(cursor, log, self._book))
            return
        if self.layerwise:
            # eager only: the values go back to the caller directly (no history row); no device guard, and the
            # parameter list may span several Adam launches (the generic clip of FusedAdam)
            self.opt.step(defer_step_count=True)
            self.opt.clip_grad_norm_after_step(self.max_norm, cursor=cursor)
            return
        self.opt.step(defer_step_count=True, guard=self._guard)
        # the pre-clip total norm (device scalar; the reference discards clip_grad_norm_'s return value)
        self.last_clip_norm = self.opt.clip_grad_norm_after_step(self.max_norm, cursor=cursor, log=log,
                                                                 guard=self._guard)

    def broadcast_parameters(self, src: int = 0):
        """Identical initial replicas (the RNG-seeded init differs per process otherwise)."""
        if self.world == 1:
            return
        with torch.no_grad():
            frozen = [] if self.layerwise else [self.model.fused.qflat]   # layerwise: Q are model parameters
            for p in list(self.model.parameters()) + frozen:
                dist.broadcast(p.data, src=src, group=self.pg)

    # ------------------------------------------------------------------ eager / graph
    def _cursor(self):
        """(device cursor, modulo) for the launch that ends a step to advance, in epoch mode."""
        return (self.walk.cursor, self.walk.n_batches) if self.walk is not None else None

    def _setup_bucket(self):
        self.bucket.setup(self.model, self.fused_loss and not self.layerwise, self.overlap_ranges)

    def eager_step(self, y, traj, gather=None, epoch_book: bool = True):
        if self.bucket is not None:
            self.bucket.drain_slices()
            self._setup_bucket()
        vals = self._forward_backward(y, traj, gather)
        if self.bucket is not None:
            vals = self.bucket.allreduce(vals)
        self._update(vals, epoch_book=epoch_book)
        if self._cap is not None:
            self._cap.rebind = True     # .grad now holds this step's buffers, not a graph's
        # world > 1: vals is a view of the bucket tail, which the next step overwrites
        return vals.clone() if self.bucket is not None else vals

    def _gather(self, idx=None, defer: bool = False):
        """Pool rows of the current batch, both tensors in one native launch: by the index buffer `idx`, or (epoch
        mode) batch `cursor` of the device-resident epoch order, the cursor advancing on the device.
        defer=True returns (y, traj, spec): when the step takes the folded path, spec is the gather (not yet
        launched) for the pack launch to run (bcnf_pack_params_fold), else None and the gather has run."""
        pool, walk = self.pool, self.walk
        out = pool.empty_batch(walk.batch if walk is not None else idx.shape[0])
        if defer and self.fused_loss and self.fuse_gather and not self.layerwise and \
                self.model._foldable_linear(out[0], (pool.unpad(out[1]),)) is not None:
            return walk.gather_spec(out) if walk is not None else pool.gather_spec(idx, idx.shape[0], out=out)
        y, t = walk.gather(out) if walk is not None else pool.gather_rows(idx, out)
        return (y, t, None) if defer else (y, t)

    def _snapshot(self):
        with torch.no_grad():
            params = [p.detach().clone() for p in self.model.parameters()]
            opt = {id(p): {k: v.clone() for k, v in st.items() if torch.is_tensor(v)}
                   for p, st in self.opt.state.items()}
            rng = self.model.fused.rng_state().clone()
            cur = self.walk.cursor.clone() if self.walk is not None else None
        return params, opt, rng, cur

    def _restore(self, snap):
        params, opt, rng, cur = snap
        with torch.no_grad():
            if cur is not None:
                self.walk.cursor.copy_(cur)
            for p, v in zip(self.model.parameters(), params):
                p.copy_(v)
            for p, st in self.opt.state.items():
                saved = opt.get(id(p))
                for k, v in st.items():
                    if torch.is_tensor(v):
                        v.copy_(saved[k]) if saved is not None else v.zero_()
            self.model.fused.rng_state().copy_(rng)

    def _build_graphs(self, y, traj, idx=None, warmup: int = 2):
        """Warm up (allocations, kernel attributes) on a side stream, undo the warm-up's updates, then
        capture: the first step() applies exactly one update, like every later one."""
        bucket = self.bucket
        if bucket is not None:
            self._setup_bucket()
        cap = _Captured(y.clone(), traj.clone(), None if idx is None else idx.clone())
        sy, st = cap.y, cap.traj
        indexed = idx is not None
        snap = self._snapshot()
        s = torch.cuda.Stream()
        s.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(s):
            for _ in range(warmup):
                if indexed:
                    self.eager_step(*self._gather(cap.idx, defer=True))
                else:
                    self.eager_step(sy, st)
            self._restore(snap)
        torch.cuda.current_stream().wait_stream(s)
        self.opt.zero_grad(set_to_none=True)
        # the three logged values are stored into the pinned history by the clip launch: the host reads
        # them after a stream sync, without a device-to-host copy node
        cap.g1 = torch.cuda.CUDAGraph()
        with torch.cuda.graph(cap.g1):
            spec = None
            if indexed:
                sy, st, spec = self._gather(cap.idx, defer=True)
            vals = cap.vals = self._forward_backward(sy, st, spec)
            if bucket is None:
                self._update(vals)
            else:
                bucket.pack_grads()         # the bucket copy is part of the captured step
                bucket.gvals.copy_(vals)    # the logged values travel with the gradients
        if bucket is not None:
            bucket.bind_grads()             # the update reads the reduced bucket
            cap.g2 = torch.cuda.CUDAGraph()
            with torch.cuda.graph(cap.g2):
                bucket.scale()
                self._update(vals)
            # the update segment of a step whose clip-after-step is unobservable (every run_epoch step but the
            # last: the next step's backward overwrites the gradients): Adam with the bookkeeping, no clip launch
            if self.skip_hidden_clips and self.opt.can_bookkeep():
                cap.g2_hidden = torch.cuda.CUDAGraph()
                with torch.cuda.graph(cap.g2_hidden):
                    bucket.scale()
                    self._update(vals, clip=False)
                if indexed:
                    # step i's hidden update and step i+1's gather / forward / backward / bucket in ONE graph: one
                    # inter-graph idle per step instead of two (run_epoch); step i+1's logged values are copied
                    # into g1's buffer, which every update segment logs from
                    cap.g21 = torch.cuda.CUDAGraph()
                    with torch.cuda.graph(cap.g21):
                        bucket.scale()
                        self._update(vals, clip=False)
                        sy2, st2, spec2 = self._gather(cap.idx, defer=True)
                        vals2 = self._forward_backward(sy2, st2, spec2)
                        bucket.pack_grads()
                        bucket.gvals.copy_(vals2)
                        vals.copy_(vals2)
                    bucket.bind_grads()
        cap.single_grads = [p.grad for p in self.params]   # what .grad shows after a g1 replay
        self._cap = cap

    def set_lr(self, lr: float):
        """The learning rate of every later step (a scheduler's change, trainer.py:222-227). The Adam launches take
        lr by value, so a captured graph holds the rate it was captured with and an edit of `opt.param_groups` alone
        never reaches it: this drops every captured graph, with the gradient bindings that belong to them, and the
        next step captures again through _build_graphs (whose snapshot / restore undo the warm-up), exactly as the
        first step did. The optimizer state, the dropout RNG offset, the epoch cursor, the history and the pool are
        kept; an eager TrainStep only has its param groups edited."""
        for group in self.opt.param_groups:
            group["lr"] = float(lr)
        self._cap = None

    def step(self, y, traj):
        """One training step; returns (loss, nll, mse) as Python floats (the Trainer's three .item())."""
        vals = self.step_async(y, traj)
        if not self.capture:
            return tuple(vals.tolist())
        return self._host_values()

    def _host_values(self, row: int = 0):
        """The step's three logged values (the Trainer's .item() calls): one stream sync, then a read of the
        pinned history row the clip launch stored them in."""
        torch.cuda.current_stream().synchronize()
        return tuple(self._hist[row].tolist())

    def step_async(self, y, traj):
        if not self.capture:
            return self.eager_step(y, traj)
        if self._cap is None:
            self._build_graphs(y, traj)
        sy, st = self._cap.y, self._cap.traj
        if y.shape != sy.shape or traj.shape != st.shape:
            # a batch of another size (the DataLoader's last, drop_last=False): the captured graph holds buffers of
            # the first batch's size, so this one runs eagerly on the same kernels and optimizer state
            return self.eager_step(y, traj)
        sy.copy_(y, non_blocking=True)
        st.copy_(traj, non_blocking=True)
        return self._replay()

    # ------------------------------------------------------------------ device-resident data pool
    def set_pool(self, y_pool, traj_pool):
        """Serve batches by index from device-resident tensors (the gather becomes part of the graph)."""
        if self._cap is not None:
            raise RuntimeError("set_pool() must precede the first step")
        # the folded feature Linear (cnf.py fold_pool_width) reads x rows with float4 loads when they are 16-byte
        # aligned: the pool zero-pads its rows (90 -> 92 floats for FC_small) once, here
        w = self.model.fold_pool_width(traj_pool) if hasattr(self.model, "fold_pool_width") else None
        self.pool = DevicePool(y_pool, traj_pool, row_width=w)

    def step_indexed(self, idx):
        """step(pool_y[idx], pool_traj[idx]) with the gather captured in the graph."""
        if self.pool is None:
            raise RuntimeError("step_indexed() needs set_pool()")
        check_indices(idx, self.pool.n)
        idx = idx.to(device=self.pool.device, dtype=torch.int64).contiguous()
        if self.walk is not None:
            # a batch outside the epoch order (the ragged remainder of an epoch, drop_last=False): the epoch graphs
            # walk the device cursor and write history rows, so this one runs eagerly on the same kernels and
            # optimizer state without touching the cursor or the history
            return tuple(self.eager_step(*self.pool.rows(idx), epoch_book=False).tolist())
        if not self.capture:
            return tuple(self.eager_step(*self._gather(idx)).tolist())
        if self._cap is None:
            self._build_graphs(*self.pool.rows(idx), idx=idx)
        if self._cap.idx is None or idx.shape != self._cap.idx.shape:
            return tuple(self.eager_step(*self.pool.rows(idx)).tolist())     # another batch size: eager
        self._cap.idx.copy_(idx, non_blocking=True)
        self._replay()
        return self._host_values()

    # ------------------------------------------------------------------ device-resident epoch order
    def set_epoch(self, order, batch: int):
        """Walk `order` (device int64, n_batches * batch pool indices, e.g. concatenated shuffled epochs)
        batch by batch with step_epoch(); the graph reads batch `cursor` and advances the cursor itself, so
        a step needs no host-to-device traffic. A later call replaces the order (same size) and rewinds."""
        if self.pool is None:
            raise RuntimeError("set_epoch() needs set_pool()")
        order = order.to(dtype=torch.int64).contiguous()
        if self.walk is not None:
            self.walk.reset(order, batch)
            return
        if self._cap is not None:
            raise RuntimeError("set_epoch() must precede the first step of a non-epoch TrainStep")
        self.walk = EpochWalk(self.pool, order, batch)
        self._hist = torch.zeros((self.walk.n_batches, 3), dtype=torch.float32, pin_memory=True)

    def step_epoch(self):
        """The next batch of the epoch order (see set_epoch)."""
        if self.walk is None:
            raise RuntimeError("step_epoch() needs set_epoch()")
        row = self.walk.host_cursor
        self.walk.host_cursor = (row + 1) % self.walk.n_batches
        if not self.capture:
            return tuple(self.eager_step(*self._gather()).tolist())
        self._ensure_epoch_graphs()
        self._replay()
        return self._host_values(row)

    def _ensure_epoch_graphs(self):
        if self._cap is None:
            y, t = self._gather()
            self._build_graphs(y, t, idx=torch.zeros(1, dtype=torch.int64, device=y.device))

    def run_epoch(self, n_steps=None, check_divergence: bool = False):
        """The remaining batches of the epoch order (or the next n_steps of them) replayed back to back with
        ONE host sync at the end; returns their (loss, nll, mse) triples in order -- the values the
        Trainer's per-batch .item() calls read (trainer.py:166-173). With check_divergence (the Trainer
        checks after epoch 10) a loss > 1e5 or NaN halts the epoch on the device right after that step's
        update and TrainingDivergedError is raised here, with the model, optimizer, RNG offset and cursor
        as the reference leaves them when it raises (only .grad holds the discarded next batch's gradient)."""
        walk = self.walk
        if walk is None:
            raise RuntimeError("run_epoch() needs set_epoch()")
        nb = walk.n_batches
        start = walk.host_cursor
        n = nb - start if n_steps is None else int(n_steps)
        if n < 0 or start + n > nb:
            raise ValueError(f"run_epoch: {n} steps from batch {start} exceed the epoch's {nb} batches")
        if n == 0:
            return []
        if not self.capture or self._no_fused_loss():  # per-step host check (the device guard sits in
            out = []                                     # the fused loss finalize), right after each update
            for i in range(n):                           # as trainer.py:166-168 does
                v = self.step_epoch()
                out.append(v)
                if check_divergence and (v[0] > 1e5 or math.isnan(v[0])):
                    raise TrainingDivergedError(f"Loss exploded to {v[0]} at batch {start + i}")
            return out
        self._ensure_epoch_graphs()
        cap = self._cap
        self._guard.zero_()
        if check_divergence:
            # data parallel: judged on the all-reduced loss, the same on every rank. Hybrid: the reference judges
            # loss, not nll (trainer.py:168), so the stack's finalize must not judge nll alone -- the combined loss is
            # judged by bcnf_hybrid_finalize (world 1) / bcnf_guard_check_global (world > 1)
            self._guard[GUARD_CHECK if (self.world == 1 and not self.hybrid) else GUARD_CHECK_GLOBAL] = 1
        i = 0
        if self.world == 1:
            sched = graph_schedule(n, self.epoch_unroll, 2)
            for k in dict.fromkeys(sched):              # each size's graph, as often as it fits, largest first
                g, grads = self._multi_graph(k)
                for _ in range(sched.count(k)):
                    g.replay()
                self._bind(grads)
                cap.rebind = True
            i = sum(sched)
        if self.world > 1 and cap.g21 is not None and n >= 2:
            cap.g1.replay()                   # g1, then (all-reduce, g21) per later step, then the last update
            for _ in range(n - 1):
                self.bucket.reduce()
                cap.g21.replay()
            self.bucket.reduce()
            cap.g2.replay()
            i = n
        while i < n:
            self._replay(hidden=i < n - 1)
            i += 1
        torch.cuda.current_stream().synchronize()
        vals = [tuple(r) for r in self._hist[start:start + n].tolist()]
        walk.host_cursor = (start + n) % nb
        if check_divergence and int(self._guard[GUARD_DIVERGED].item()):
            for i, v in enumerate(vals):
                if v[0] > 1e5 or math.isnan(v[0]):
                    walk.host_cursor = (start + i + 1) % nb
                    self._guard.zero_()
                    raise TrainingDivergedError(f"Loss exploded to {v[0]} at batch {start + i}")
        return vals

    # Steps per captured graph in run_epoch: run_epoch replays `epoch_unroll` device-driven steps (cursor, RNG
    # offset, Adam step, history row all advance on the device) per launch and the remainder in graphs of
    # epoch_unroll / 2, / 4, ... steps (epoch.graph_schedule) and a last single step.
    epoch_unroll = 8
    # The captured step runs the batch gather inside the folded path's pack launch (one launch fewer).
    fuse_gather = True
    # Inside a multi-step graph only the last step's clip-after-step is observable (see _update).
    skip_hidden_clips = True

    def _multi_graph(self, k: int):
        cap = self._cap
        if k not in cap.multi:
            self._bind(cap.single_grads)           # every multi-step graph is captured from the same .grad state
            g = torch.cuda.CUDAGraph()
            with torch.cuda.graph(g):
                slots = self._fold_adam_slots()
                for i in range(k):
                    hidden = i < k - 1 and self.skip_hidden_clips
                    sy, st, spec = self._gather(cap.idx, defer=True)
                    if hidden and slots is not None and self.model._foldable_linear(sy, (st,)) is not None:
                        # Adam of this step runs inside its folded backward tail (bcnf_fold_backward_tail)
                        self._forward_backward(sy, st, spec, adam=lambda v: self._fold_adam(slots, v))
                        continue
                    vals = self._forward_backward(sy, st, spec)
                    self._update(vals, clip=not (hidden and self.opt.can_bookkeep()))
            cap.multi[k] = (g, [p.grad for p in self.params])
            self._bind(cap.single_grads)
            cap.rebind = False
        return cap.multi[k]

    # Hidden steps of a folded model update their parameters inside the backward tail (no Adam launch).
    fuse_adam = True
    # hybrid_weight > 0 runs model.hybrid_loss (the head + MSE kernels, one autograd node). False: the generic route
    # (torch nn.Linear + MSELoss, dz / dldj tensors, per-batch host sync in run_epoch) -- tests and A/B runs.
    fuse_hybrid = True

    @property
    def hybrid(self) -> bool:
        """hybrid_weight > 0 on a fused-stack model with fuse_hybrid on: the step runs model.hybrid_loss."""
        return self.hybrid_weight > 0.0 and not self.layerwise and self.fuse_hybrid

    def _no_fused_loss(self) -> bool:
        """No fused loss finalize (hence no device guard, no multi-step graphs): an AnyGLU stack, or hybrid_weight > 0
        with fuse_hybrid off."""
        return self.layerwise or (self.hybrid_weight > 0.0 and not self.hybrid)

    def _fold_adam_slots(self):
        """(coupling flat parameter, feature weight, feature bias) when the fused-Adam tail applies: the model
        folds its feature Linear and those are exactly this optimizer's parameters; else None."""
        if not self.fuse_adam or self.world != 1 or not self.fused_loss:
            return None
        lin = self.model._fold_linear() if hasattr(self.model, "_fold_linear") else None
        if lin is None:
            return None
        slots = (self.model.fused.flat_param, lin.weight, lin.bias)
        live = [p for p in slots if p is not None]
        if [id(p) for p in sorted(live, key=id)] != [id(p) for p in sorted(self.params, key=id)]:
            return None
        return slots

    def _fold_adam(self, slots, vals):
        log = (vals, self._hist) if self._hist is not None else None
        spec = self.opt.fold_adam_spec(slots, cursor=self._cursor(), log=log, counter=self._book, guard=self._guard)
        if spec is None:
            raise RuntimeError("bcnf_amd TrainStep: the optimizer does not match the fused-Adam slots")
        return spec

    def _bind(self, grads):
        """.grad = the gradient buffers of the graph that ran last (each captured graph owns its own)."""
        if grads is None:
            return
        for p, gr in zip(self.params, grads):
            p.grad = gr

    def prepare_epoch(self, n_steps: int):
        """Capture, without running anything, every graph a later run_epoch(n_steps) replays (the step graphs and,
        at world 1, the multi-step graph), so no capture lands inside a timed region."""
        if self.walk is None or not self.capture or self._no_fused_loss():
            return
        self._ensure_epoch_graphs()
        if self.world == 1:
            for k in dict.fromkeys(graph_schedule(n_steps, self.epoch_unroll, 2)):
                self._multi_graph(k)

    def _replay(self, hidden: bool = False):
        cap = self._cap
        if cap.rebind:
            self._bind(cap.single_grads)
            cap.rebind = False
        cap.g1.replay()
        if cap.g2 is not None:
            self.bucket.reduce()            # the one collective of the step, between the two graph segments
            (cap.g2_hidden if hidden and cap.g2_hidden is not None else cap.g2).replay()
        return cap.vals


__all__ = ["TrainStep", "FusedAdam", "clip_grad_norm_", "TrainingDivergedError"]
