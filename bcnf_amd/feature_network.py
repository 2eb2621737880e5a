"""Conditioning (feature) networks — PyTorch-ROCm, as the north star prescribes.

Restated from the reference's behaviour (src/bcnf/models/feature_network.py); their output h
(B, n_conditions) is the input boundary of the HIP coupling stack and dL/dh comes back out of it.

* FeatureNetworkStack          feature_network.py:28-73  (consumes one condition per ConcatenateCondition)
* ConcatenateCondition         feature_network.py:76-88
* FullyConnectedFeatureNetwork feature_network.py:114-145 (x.view(B,-1); Linear/[BN]/act/[Dropout] ...)
* LSTMFeatureNetwork           feature_network.py:148-178 — reference pools over dim 0 (the BATCH axis
  of a batch_first LSTM), which crashes for batch != seq_len. `pool_dim=0` keeps that
  behaviour bit-for-bit; `pool_dim=1` pools over time (documented fix used for trajectory_LSTM_large).
* MultiHeadAttention / TransformerBlock / Transformer  feature_network.py:183-307 and DualDomainTransformer
  feature_network.py:401-471 — same kwargs, submodule names and state_dict keys; on fp32 GPU tensors the Linear
  layers run on the MFMA GEMMs over (B S, d) rows and the attention core and each residual + LayerNorm as one HIP
  launch per direction (bcnf_amd/csrc/bcnf_attn.hip); CPU tensors and shapes outside the kernels' limits run the
  reference's chain of torch ops. A head split that does not divide (trf_size % n_heads != 0) raises on forward.
* VerboseLSTM / DualDomainLSTM  feature_network.py:310-398 -- same kwargs, submodule names and state_dict keys (single-
  layer nn.LSTM modules in a ModuleList); on fp32 GPU tensors with hidden % 16 == 0, 16 <= hidden <= 128 each layer
  runs its input projection on the MFMA GEMMs and the recurrence of both directions as one HIP launch
  (bcnf_amd/csrc/bcnf_lstm.hip); CPU tensors and other shapes run the nn.LSTM modules.
* CNN  models/cnn.py -- in bcnf_amd/cnn.py (it registers itself in FEATURE_NETWORKS below); FeatureRngMixin here is the
  dropout Philox state it shares with FullyConnectedFeatureNetwork.
"""
from __future__ import annotations

import math
import weakref
from typing import Any, Type

import numpy as np
import torch
from torch import nn


class _LinearFn(torch.autograd.Function):
    """y = x W^T + b on the HIP GEMM kernels (bcnf_linear_forward / bcnf_linear_backward)."""

    @staticmethod
    def forward(ctx, x, weight, bias):
        from bcnf_amd import _native as N
        rows, k = x.shape
        n = weight.shape[0]
        y = torch.empty((rows, n), dtype=torch.float32, device=x.device)
        N.call("bcnf_linear_forward", x, weight, bias, rows, k, n, y, N.stream_handle(x.device))
        ctx.save_for_backward(x, weight)
        ctx.has_bias = bias is not None
        return y

    @staticmethod
    def backward(ctx, dy):
        from bcnf_amd import _native as N
        x, weight = ctx.saved_tensors
        dy = dy.contiguous()
        rows, k = x.shape
        n = weight.shape[0]
        need_x, need_w, need_b = ctx.needs_input_grad
        dx = torch.empty_like(x) if need_x else None
        dw = torch.empty_like(weight) if (need_w or need_b) else None
        db = torch.empty(n, dtype=torch.float32, device=x.device) if (need_b and ctx.has_bias) else None
        work = None
        if dw is not None:
            wb = N.call_raw("bcnf_linear_work_bytes", rows, k, n)
            work = torch.empty(max(wb // 4, 1), dtype=torch.float32, device=x.device)
        N.call("bcnf_linear_backward", x, weight, dy, rows, k, n, dx, dw, db, work, N.stream_handle(x.device))
        return dx, (dw if need_w else None), db


class _LinearGeluFn(torch.autograd.Function):
    """a = dropout(GELU(x W^T + b)) in ONE launch (bcnf_linear_gelu_forward), the backward from the saved
    g = mask GELU'(pre) in the dX / dW GEMMs' operand loads (bcnf_linear_gelu_backward): no ATen GELU, dropout,
    GELU-backward or masked-scale launches."""

    @staticmethod
    def forward(ctx, x, weight, bias, p, rng, salt, need_g):
        from bcnf_amd import _native as N
        rows, k = x.shape
        n = weight.shape[0]
        a = torch.empty((rows, n), dtype=torch.float32, device=x.device)
        g = torch.empty_like(a) if need_g else None
        N.call("bcnf_linear_gelu_forward", x, weight, bias, rows, k, n, float(p), rng, int(salt), a, g,
               N.stream_handle(x.device))
        ctx.save_for_backward(x, weight, g)
        ctx.has_bias = bias is not None
        return a

    @staticmethod
    def backward(ctx, da):
        from bcnf_amd import _native as N
        x, weight, g = ctx.saved_tensors
        if g is None:
            raise RuntimeError("bcnf_amd: fused Linear + GELU layer ran without saving its derivative")
        da = da.contiguous()
        rows, k = x.shape
        n = weight.shape[0]
        need_x, need_w, need_b = ctx.needs_input_grad[:3]
        dx = torch.empty_like(x) if need_x else None
        dw = torch.empty_like(weight) if (need_w or need_b) else None
        db = torch.empty(n, dtype=torch.float32, device=x.device) if (need_b and ctx.has_bias) else None
        work = None
        if dw is not None:
            wb = N.call_raw("bcnf_linear_work_bytes", rows, k, n)
            work = torch.empty(max(wb // 4, 1), dtype=torch.float32, device=x.device)
        N.call("bcnf_linear_gelu_backward", x, weight, da, g, rows, k, n, dx, dw, db, work, N.stream_handle(x.device))
        return dx, (dw if need_w else None), db, None, None, None, None


class HIPLinear(nn.Linear):
    """nn.Linear (same parameters / state_dict keys) whose fp32 GPU forward and backward run on the
    library's MFMA GEMM kernels; other devices / dtypes use torch's own linear."""

    def forward(self, x: torch.Tensor) -> torch.Tensor:
        if x.is_cuda and x.dtype == torch.float32 and x.dim() == 2 and self.weight.dtype == torch.float32:
            return _LinearFn.apply(x.contiguous(), self.weight, self.bias)
        return super().forward(x)


# feature network -> weakref to the CondRealNVP_v2 whose coupling Philox state its fused dropout shares
_RNG_OWNERS: "weakref.WeakKeyDictionary[nn.Module, weakref.ref]" = weakref.WeakKeyDictionary()


def bind_rng_owner(fn: nn.Module, owner: nn.Module) -> None:
    _RNG_OWNERS[fn] = weakref.ref(owner)


class FeatureNetwork(nn.Module):
    input_size: int
    output_size: int

    @property
    def n_params(self) -> int:
        return sum(p.numel() for p in self.parameters())

    def forward(self, x: torch.Tensor) -> torch.Tensor:  # pragma: no cover - abstract
        raise NotImplementedError


class ConcatenateCondition(FeatureNetwork):
    def __init__(self, input_size: int | None, output_size: int, dim: int = -1) -> None:
        super().__init__()
        self.input_size = input_size
        self.output_size = output_size
        self.dim = dim

    def forward(self, x: torch.Tensor) -> torch.Tensor:
        return x


class FeatureRngMixin:
    """The device Philox (seed, offset) state a feature network's fused dropout draws from (FullyConnected's
    Linear + GELU + Dropout layers, the CNN's convolution blocks)."""

    # Philox stream of the fused dropout: the owning CondRealNVP_v2's coupling (seed, offset) state when one is bound
    # (bind_rng_owner; a registry outside the module, so deepcopy / pickle of this module never carry a reference to
    # another model -- CondRealNVP_v2 re-binds its copies), so one device offset serves the feature and the coupling
    # dropout and `model.fused.set_seed` / TrainStep's snapshot cover both; else this module's own state.
    # Advancing: the owner's coupling launch bumps the shared offset once per training step when the coupling itself
    # drops out (and a feature draw that no coupling launch followed -- this network run on its own -- is advanced
    # at the next draw, StackBase.feature_rng_state); otherwise (coupling dropout 0, the owner in eval mode or
    # elsewhere, no owner) the network bumps it after its last fused dropout layer -- a device-side add,
    # replay-safe in HIP graphs -- so every training step draws fresh feature masks.
    _own_rng = None

    def rng_state(self, device) -> torch.Tensor:
        return self._rng(device, draw=False)[0]

    def _rng(self, device, draw: bool = True) -> tuple[torch.Tensor, bool]:
        """(device (seed, offset) state, whether the owner's coupling launch advances it this step); draw: the
        caller draws from it now (marks the draw on the owner's stack, see StackBase.feature_rng_state)."""
        ref = _RNG_OWNERS.get(self)
        owner = ref() if ref is not None else None
        fused = owner.__dict__.get("_fused") if owner is not None else None
        if fused is not None and hasattr(fused, "rng_state") and getattr(fused, "flat", None) is not None \
                and fused.flat.device == device:
            cfg = getattr(fused, "cfg", None)
            if not draw:
                return fused._rng_tensor(), False
            if owner.training and cfg is not None and cfg.dropout > 0.0:
                return fused.feature_rng_state(), True
            return fused._rng_tensor(), False
        if self._own_rng is None or self._own_rng.device != device:
            seed = (torch.cuda.initial_seed() * 0x9E3779B97F4A7C15 + 0xFEA7) & ((1 << 62) - 1)
            self._own_rng = torch.tensor([seed, 0], dtype=torch.int64, device=device)
        return self._own_rng, False


class FullyConnectedFeatureNetwork(FeatureRngMixin, FeatureNetwork):
    def __init__(self, sizes: list[int], activation: Type[nn.Module] = nn.GELU, dropout: float = 0.0,
                 batch_norm: bool = False) -> None:
        super().__init__()
        self.input_size = sizes[0]
        self.output_size = sizes[-1]
        self.output_size_lin = sizes[-1]
        self.nn = nn.Sequential()
        if len(sizes) < 2:
            self.nn.append(nn.Identity())
            return
        for a, b in zip(sizes[:-2], sizes[1:-1]):
            self.nn.append(HIPLinear(a, b))
            if batch_norm:
                self.nn.append(nn.BatchNorm1d(b))
            self.nn.append(activation())
            if dropout > 0.0:
                self.nn.append(nn.Dropout(dropout))
        self.nn.append(HIPLinear(sizes[-2], sizes[-1]))

    def forward(self, x: torch.Tensor) -> torch.Tensor:
        return self.run(x.view(x.size(0), -1))

    def run(self, x: torch.Tensor, upto: int | None = None) -> torch.Tensor:
        """Modules [0, upto) of the MLP on the flattened input. Each Linear -> GELU(exact) [-> Dropout] group of fp32
        CUDA tensors runs as ONE fused launch (bcnf_linear_gelu_forward, salt = its module index); the rest as the
        modules themselves (BatchNorm, other activations, CPU)."""
        mods = list(self.nn)[:upto]
        i = 0
        bump = None                       # the state to advance after the last fused dropout layer, if run() must
        rng = None                        # one state lookup per call (the owner's feature_rng_state marks one draw)
        while i < len(mods):
            m = mods[i]
            act = mods[i + 1] if i + 1 < len(mods) else None
            if isinstance(m, nn.Linear) and isinstance(act, nn.GELU) and act.approximate == "none" \
                    and x.is_cuda and x.dtype == torch.float32 and x.dim() == 2 and m.weight.dtype == torch.float32:
                drop = mods[i + 2] if i + 2 < len(mods) and isinstance(mods[i + 2], nn.Dropout) else None
                p = drop.p if (drop is not None and drop.training) else 0.0
                if p > 0.0 and rng is None:
                    rng, owner_bumps = self._rng(x.device)
                    bump = None if owner_bumps else rng
                need_g = torch.is_grad_enabled() and (x.requires_grad or m.weight.requires_grad or
                                                      (m.bias is not None and m.bias.requires_grad))
                x = _LinearGeluFn.apply(x.contiguous(), m.weight, m.bias, p, rng if p > 0.0 else None, i, need_g)
                i += 3 if drop is not None else 2
                continue
            x = m(x)
            i += 1
        if bump is not None:
            bump[1:2].add_(1)
        return x


class LSTMFeatureNetwork(FeatureNetwork):
    def __init__(self, input_size: int, hidden_size: int, output_size: int, num_layers: int, dropout: float = 0.0,
                 bidirectional: bool = False, pooling: str = "mean", pool_dim: int = 0) -> None:
        super().__init__()
        if pooling not in ("mean", "max"):
            raise ValueError(f'Pooling method {pooling} not supported. Use either "mean" or "max".')
        self.input_size = input_size
        self.output_size = output_size
        self.lstm = nn.LSTM(input_size=input_size, hidden_size=hidden_size, num_layers=num_layers, dropout=dropout,
                            bidirectional=bidirectional, batch_first=True)
        self.linear = nn.Linear(hidden_size * (2 if bidirectional else 1), output_size)
        self.pooling = pooling
        self.pool_dim = pool_dim

    def lstm_out(self, x: torch.Tensor) -> torch.Tensor:
        """The LSTM's output sequence (B, T, hidden * directions). The LSTM itself stays on PyTorch-ROCm (north star):
        MIOpen's fused RNN kernels, measured against torch's native per-step kernels in DESIGN §5
        (profiles/r04c_lstm_miopen_vs_native.txt)."""
        return self.lstm(x)[0]

    def forward(self, x: torch.Tensor) -> torch.Tensor:
        x = self.linear(self.lstm_out(x))
        if self.pooling == "mean":
            return x.mean(dim=self.pool_dim)
        return x.max(dim=self.pool_dim).values


ATTN_MAX_SEQ = 64          # bcnf_attn_*: S <= 64, head_dim <= 64 (include/bcnf_amd.h)
ATTN_MAX_HEAD_DIM = 64
ADD_LN_MAX_D = 1024        # bcnf_add_layernorm_*: d <= 1024
_LN_WORK_FLOATS: dict = {}  # (rows, d) -> floats of the backward's partials (bcnf_add_layernorm_work_bytes)


class _AttnFn(torch.autograd.Function):
    """softmax(q k^T / sqrt(hd)) v per (sample, head) on the (B S, heads hd) rows of the q / k / v Linear layers, in
    ONE launch each way (bcnf_attn_forward / bcnf_attn_backward): no head transposes, no score or probability tensor;
    the forward keeps the (B, heads, S) log-sum-exp."""

    @staticmethod
    def forward(ctx, q, k, v, batch, seq, heads, hd):
        from bcnf_amd import _native as N
        out = torch.empty_like(q)
        lse = torch.empty((batch, heads, seq), dtype=torch.float32, device=q.device)
        N.call("bcnf_attn_forward", q, k, v, batch, seq, heads, hd, q.shape[1], out, lse, N.stream_handle(q.device))
        ctx.save_for_backward(q, k, v, out, lse)
        ctx.dims = (batch, seq, heads, hd)
        return out

    @staticmethod
    def backward(ctx, dout):
        from bcnf_amd import _native as N
        q, k, v, out, lse = ctx.saved_tensors
        batch, seq, heads, hd = ctx.dims
        dout = dout.contiguous()
        dq, dk, dv = torch.empty_like(q), torch.empty_like(k), torch.empty_like(v)
        N.call("bcnf_attn_backward", q, k, v, out, lse, dout, batch, seq, heads, hd, q.shape[1], dq, dk, dv,
               N.stream_handle(q.device))
        return dq, dk, dv, None, None, None, None


class _AddLayerNormFn(torch.autograd.Function):
    """y = LayerNorm(x + r) in ONE launch (bcnf_add_layernorm_forward); the backward (one launch, plus the fixed-order
    reduce of the gamma / beta partials) returns the one dx = dr for both inputs."""

    @staticmethod
    def forward(ctx, x, r, gamma, beta, eps):
        from bcnf_amd import _native as N
        rows, d = x.shape
        y = torch.empty_like(x)
        stats = torch.empty((2, rows), dtype=torch.float32, device=x.device)       # mean | rstd
        N.call("bcnf_add_layernorm_forward", x, r, gamma, beta, rows, d, float(eps), y, stats[0], stats[1],
               N.stream_handle(x.device))
        ctx.save_for_backward(x, r, gamma, stats)
        return y

    @staticmethod
    def backward(ctx, dy):
        from bcnf_amd import _native as N
        x, r, gamma, stats = ctx.saved_tensors
        rows, d = x.shape
        dy = dy.contiguous()
        need_x, need_r, need_g, need_b = ctx.needs_input_grad[:4]
        dx = torch.empty_like(x) if (need_x or need_r) else None
        dg = db = work = None
        if need_g or need_b:
            wf = _LN_WORK_FLOATS.get((rows, d))
            if wf is None:
                wf = _LN_WORK_FLOATS[(rows, d)] = max(N.query_i64("bcnf_add_layernorm_work_bytes", rows, d) // 4, 1)
            dg, db = torch.empty((2, d), dtype=torch.float32, device=x.device).unbind(0)
            work = torch.empty(wf, dtype=torch.float32, device=x.device)
        N.call("bcnf_add_layernorm_backward", x, r, gamma, stats[0], stats[1], dy, rows, d, dx,
               dg if need_g else None, db if need_b else None, work, N.stream_handle(x.device))
        return (dx if need_x else None), (dx if need_r else None), (dg if need_g else None), \
            (db if need_b else None), None


def _on_kernels(x: torch.Tensor, *params: torch.Tensor) -> bool:
    return x.is_cuda and x.dtype == torch.float32 and all(p is None or p.dtype == torch.float32 for p in params)


def _rows_linear(lin: nn.Linear, x: torch.Tensor) -> torch.Tensor:
    """lin(x) for x (..., k): fp32 GPU tensors go through HIPLinear as (rows, k); the rest is torch's linear."""
    if x.dim() > 2 and _on_kernels(x, lin.weight):
        return lin(x.reshape(-1, x.shape[-1])).view(*x.shape[:-1], lin.out_features)
    return lin(x)


class MultiHeadAttention(nn.Module):
    """feature_network.py:183-229. fp32 GPU tensors with S <= 64 and head_dim <= 64: the Linear layers on the MFMA GEMMs
    over (B S, d) rows and the attention core in one launch (_AttnFn); everything else, and `fused = False`, runs the
    reference's chain of torch ops."""

    fused = True        # False: the attention core on torch ops (fallback tests, tools/transformer_feature_ab.py)

    def __init__(self, d_model: int, n_heads: int) -> None:
        super().__init__()
        self.d_model = d_model
        self.n_heads = n_heads
        self.head_dim = d_model // n_heads
        self.q_linear = HIPLinear(d_model, d_model)
        self.k_linear = HIPLinear(d_model, d_model)
        self.v_linear = HIPLinear(d_model, d_model)
        self.fc_out = HIPLinear(d_model, d_model)

    def forward(self, query: torch.Tensor, key: torch.Tensor, value: torch.Tensor, mask=None) -> torch.Tensor:
        if self.d_model % self.n_heads != 0:
            # the reference's view(B, -1, n_heads, head_dim) fails here (or, where it happens to fit, silently mixes
            # time steps into heads): t_PTRF_small (46 / 4), t_DPTRF_medium (70 / 8)
            raise RuntimeError(f"bcnf_amd: MultiHeadAttention cannot split d_model = trf_size = {self.d_model} into "
                               f"n_heads = {self.n_heads} heads ({self.d_model} % {self.n_heads} != 0)")
        batch = query.size(0)
        q = _rows_linear(self.q_linear, query)
        k = _rows_linear(self.k_linear, key)
        v = _rows_linear(self.v_linear, value)
        seq = q.shape[1] if q.dim() == 3 else -1
        if (self.fused and mask is None and q.dim() == 3 and q.shape == k.shape == v.shape and _on_kernels(q)
                and 1 <= seq <= ATTN_MAX_SEQ and self.head_dim <= ATTN_MAX_HEAD_DIM and batch > 0):
            rows = batch * seq
            out = _AttnFn.apply(q.reshape(rows, self.d_model), k.reshape(rows, self.d_model),
                                v.reshape(rows, self.d_model), batch, seq, self.n_heads, self.head_dim)
            out = out.view(batch, seq, self.d_model)
        else:
            q = q.view(batch, -1, self.n_heads, self.head_dim).transpose(1, 2)
            k = k.view(batch, -1, self.n_heads, self.head_dim).transpose(1, 2)
            v = v.view(batch, -1, self.n_heads, self.head_dim).transpose(1, 2)
            scores = torch.matmul(q, k.transpose(-2, -1)) / math.sqrt(self.head_dim)
            if mask is not None:
                scores = scores.masked_fill(mask == 0, -1e9)
            out = torch.matmul(torch.softmax(scores, dim=-1), v)
            out = out.transpose(1, 2).contiguous().view(batch, -1, self.d_model)
        return _rows_linear(self.fc_out, out)


class TransformerBlock(nn.Module):
    """feature_network.py:232-260, post-norm: norm1(x + drop(attn(x))), norm2(x + drop(ffn(x))) with ONE Dropout module.
    fp32 GPU tensors: each residual + LayerNorm in one launch (_AddLayerNormFn, d <= 1024) and the FFN's Linear + GELU
    in one (_LinearGeluFn, p = 0); `fused = False` keeps the two norms on torch ops."""

    fused = True        # False: x + r and LayerNorm on torch ops

    def __init__(self, d_model: int, n_heads: int, ff_size: int, dropout: float = 0.1) -> None:
        super().__init__()
        self.attention = MultiHeadAttention(d_model, n_heads)
        self.norm1 = nn.LayerNorm(d_model)
        self.norm2 = nn.LayerNorm(d_model)
        self.ffn = nn.Sequential(HIPLinear(d_model, ff_size), nn.GELU(), HIPLinear(ff_size, d_model))
        self.dropout = nn.Dropout(dropout)

    def _add_norm(self, norm: nn.LayerNorm, x: torch.Tensor, r: torch.Tensor) -> torch.Tensor:
        d = x.shape[-1]
        if (self.fused and norm.elementwise_affine and norm.bias is not None and d <= ADD_LN_MAX_D
                and x.shape == r.shape and x.numel() > 0 and _on_kernels(x, norm.weight) and r.dtype == x.dtype):
            y = _AddLayerNormFn.apply(x.reshape(-1, d).contiguous(), r.reshape(-1, d).contiguous(), norm.weight,
                                      norm.bias, norm.eps)
            return y.view(x.shape)
        return norm(x + r)

    def _ffn(self, x: torch.Tensor) -> torch.Tensor:
        lin0, lin1 = self.ffn[0], self.ffn[2]
        if x.dim() == 3 and x.numel() > 0 and _on_kernels(x, lin0.weight):
            rows = x.reshape(-1, x.shape[-1]).contiguous()
            need_g = torch.is_grad_enabled() and (rows.requires_grad or lin0.weight.requires_grad or
                                                  (lin0.bias is not None and lin0.bias.requires_grad))
            a = _LinearGeluFn.apply(rows, lin0.weight, lin0.bias, 0.0, None, 0, need_g)
            return lin1(a).view(*x.shape[:-1], lin1.out_features)
        return self.ffn(x)

    def forward(self, x: torch.Tensor) -> torch.Tensor:
        x = self._add_norm(self.norm1, x, self.dropout(self.attention(x, x, x)))
        return self._add_norm(self.norm2, x, self.dropout(self._ffn(x)))


class Transformer(FeatureNetwork):
    """feature_network.py:263-307: features Linear, ONE Dropout(dropout) applied after it and again after the last
    block to the whole (B, S, d) tensor, positional table added in between, then `output` of the first token."""

    def __init__(self, input_size: int, trf_size: int, n_heads: int, ff_size: int, n_blocks: int, output_size: int,
                 dropout: float = 0.5, trf_dropout: float = 0.1, add_positional_embeddings: bool = False) -> None:
        super().__init__()
        self.input_size = input_size
        self.output_size = output_size
        self.add_positional_embeddings = add_positional_embeddings
        self.trf_size = trf_size
        self.features = HIPLinear(input_size, trf_size)
        self.layers = nn.ModuleList([TransformerBlock(trf_size, n_heads, ff_size, trf_dropout)
                                     for _ in range(n_blocks)])
        self.output = HIPLinear(trf_size, output_size)
        self.dropout = nn.Dropout(dropout)
        self._tables: dict = {}        # (S, device) -> table; a plain cache, not a buffer: no state_dict key

    def positional_table(self, seq_len: int, device) -> torch.Tensor:
        """The reference's (S, trf_size) table (feature_network.py:289-295): only columns j < input_size are filled,
        sin for even j and cos for odd j of i / 10000 ** (2 j / input_size), evaluated in float64 and stored as
        float32. Built once per (S, device)."""
        key = (int(seq_len), str(device))
        table = self._tables.get(key)
        if table is None:
            host = torch.zeros(seq_len, self.trf_size)
            for i in range(seq_len):
                for j in range(self.input_size):
                    angle = i / 10000 ** (2 * j / self.input_size)
                    host[i, j] = np.sin(angle) if j % 2 == 0 else np.cos(angle)
            table = self._tables[key] = host.to(device)
        return table

    def first_token(self, x: torch.Tensor) -> torch.Tensor:
        """Everything before `output`: the dropped-out first token (B, trf_size) of the last block."""
        x = self.dropout(_rows_linear(self.features, x))
        if self.add_positional_embeddings:
            x = x + self.positional_table(x.size(1), x.device)
        for layer in self.layers:
            x = layer(x)
        return self.dropout(x)[:, 0, :]

    def forward(self, x: torch.Tensor) -> torch.Tensor:
        return self.output(self.first_token(x))


class DualDomainTransformer(FeatureNetwork):
    """feature_network.py:401-471: a Transformer on x, one on cat(rfft(x, dim=1).real, .imag) (S // 2 + 1 bins of
    2 input_size values), and a FullyConnectedFeatureNetwork on their concatenated (B, 2 trf_size) outputs."""

    def __init__(self, input_size: int, trf_size: int, n_heads: int, ff_size: int, n_blocks: int, fc_sizes: list[int],
                 fc_dropout: float = 0.5, trf_dropout: float = 0.1, dropout: float = 0.5,
                 add_positional_embeddings: bool = False) -> None:
        super().__init__()
        self.input_size = input_size
        self.output_size = fc_sizes[-1]
        self.add_positional_embeddings = add_positional_embeddings
        kwargs = dict(trf_size=trf_size, n_heads=n_heads, ff_size=ff_size, n_blocks=n_blocks, output_size=trf_size,
                      dropout=dropout, trf_dropout=trf_dropout, add_positional_embeddings=add_positional_embeddings)
        self.time_transformer = Transformer(input_size=input_size, **kwargs)
        self.frequency_transformer = Transformer(input_size=input_size * 2, **kwargs)
        self.fc_sizes = [trf_size * 2] + list(fc_sizes)
        self.fc = FullyConnectedFeatureNetwork(sizes=self.fc_sizes, dropout=fc_dropout)

    def combined(self, x: torch.Tensor) -> torch.Tensor:
        """The input of `fc`: (B, 2 trf_size) = [time branch | frequency branch]."""
        x_out = self.time_transformer(x)
        freq = torch.fft.rfft(x, dim=1)
        x_frequency_out = self.frequency_transformer(torch.cat([freq.real, freq.imag], dim=-1))
        return torch.cat([x_out, x_frequency_out], dim=1)

    def forward(self, x: torch.Tensor) -> torch.Tensor:
        return self.fc(self.combined(x))


LSTM_MIN_HIDDEN = 16       # bcnf_lstm_*: hidden % 16 == 0, 16 <= hidden <= 128 (include/bcnf_amd.h)
LSTM_MAX_HIDDEN = 128


def _linear_work(N, rows: int, k: int, n: int, device) -> torch.Tensor:
    wb = N.call_raw("bcnf_linear_work_bytes", rows, k, n)
    return torch.empty(max(wb // 4, 1), dtype=torch.float32, device=device)


class _LSTMLayerFn(torch.autograd.Function):
    """One single-layer nn.LSTM (batch_first, zero initial state) on its own parameter tensors: per direction the input
    projection P = x W_ih^T + b_ih over all (B S) rows as one GEMM (bcnf_linear_forward), then the recurrence of both
    directions in ONE launch (bcnf_lstm_forward), which writes direction d at columns d H .. of the (B, S, dirs H)
    output -- no cat, no per-step kernels. Backward: one bcnf_lstm_backward for dP, then bcnf_linear_backward for
    (dx, dW_ih, db_ih) on x and for dW_hh on h_prev, the output shifted one step against the direction;
    db_hh = db_ih."""

    @staticmethod
    def forward(ctx, x, hidden, *params):
        from bcnf_amd import _native as N
        dirs = len(params) // 4
        batch, seq, k = x.shape
        rows = batch * seq
        x2 = x.reshape(rows, k)
        st = N.stream_handle(x.device)
        opts = dict(dtype=torch.float32, device=x.device)
        proj = torch.empty((dirs, rows, 4 * hidden), **opts)
        for d in range(dirs):
            w_ih, _, b_ih, _ = params[4 * d:4 * d + 4]
            N.call("bcnf_linear_forward", x2, w_ih, b_ih, rows, k, 4 * hidden, proj[d], st)
        out = torch.empty((batch, seq, dirs * hidden), **opts)
        save = any(ctx.needs_input_grad)     # all False under no_grad: nothing is saved at inference
        gates = torch.empty((dirs, rows, 4 * hidden), **opts) if save else None
        cells = torch.empty((dirs, rows, hidden), **opts) if save else None
        rev = 4 if dirs == 2 else 0
        N.call("bcnf_lstm_forward", proj[0], proj[1] if dirs == 2 else None, 4 * hidden, params[1],
               params[rev + 1] if dirs == 2 else None, params[3], params[rev + 3] if dirs == 2 else None, batch, seq,
               hidden, dirs, out, dirs * hidden, gates, cells, st)
        if save:
            ctx.save_for_backward(x2, out, gates, cells, *params)
        ctx.dims = (batch, seq, k, hidden, dirs)
        return out

    @staticmethod
    def backward(ctx, dout):
        from bcnf_amd import _native as N
        x2, out, gates, cells, *params = ctx.saved_tensors
        batch, seq, k, hidden, dirs = ctx.dims
        rows = batch * seq
        st = N.stream_handle(x2.device)
        dout = dout.contiguous()
        dproj = torch.empty((dirs, rows, 4 * hidden), dtype=torch.float32, device=x2.device)
        N.call("bcnf_lstm_backward", dout, dirs * hidden, gates, cells, params[1], params[5] if dirs == 2 else None,
               batch, seq, hidden, dirs, dproj[0], dproj[1] if dirs == 2 else None, 4 * hidden, st)
        need = ctx.needs_input_grad
        dx = None
        grads = []
        for d in range(dirs):
            w_ih, w_hh, b_ih, b_hh = params[4 * d:4 * d + 4]
            n_ih, n_hh, n_bi, n_bh = need[2 + 4 * d:6 + 4 * d]
            dxd = torch.empty_like(x2) if need[0] else None
            need_b = (n_bi and b_ih is not None) or (n_bh and b_hh is not None)
            dw_ih = torch.empty_like(w_ih) if (n_ih or need_b) else None
            db = torch.empty(4 * hidden, dtype=torch.float32, device=x2.device) if need_b else None
            if dxd is not None or dw_ih is not None:
                work = _linear_work(N, rows, k, 4 * hidden, x2.device) if dw_ih is not None else None
                N.call("bcnf_linear_backward", x2, w_ih, dproj[d], rows, k, 4 * hidden, dxd, dw_ih, db, work, st)
            dw_hh = None
            if n_hh:
                # h_prev: h of the forward's previous step, zeros at its first
                hp = torch.zeros((batch, seq, hidden), dtype=torch.float32, device=x2.device)
                if seq > 1:
                    h = out[:, :, d * hidden:(d + 1) * hidden]
                    if d == 0:
                        hp[:, 1:].copy_(h[:, :-1])
                    else:
                        hp[:, :-1].copy_(h[:, 1:])
                dw_hh = torch.empty_like(w_hh)
                N.call("bcnf_linear_backward", hp, w_hh, dproj[d], rows, hidden, 4 * hidden, None, dw_hh, None,
                       _linear_work(N, rows, hidden, 4 * hidden, x2.device), st)
            if dxd is not None:
                dx = dxd if dx is None else dx.add_(dxd)
            grads += [dw_ih if n_ih else None, dw_hh, db if (n_bi and b_ih is not None) else None,
                      db.clone() if (n_bh and b_hh is not None) else None]
        return (dx.view(batch, seq, k) if dx is not None else None), None, *grads


class VerboseLSTM(nn.Module):
    """feature_network.py:310-347: `lstm`, a ModuleList of single-layer batch_first nn.LSTM modules with an nn.Dropout
    between them when dropout > 0 (same state_dict keys, the Dropout entries' index gaps included). fp32 GPU tensors
    with hidden % 16 == 0 and 16 <= hidden <= 128 run each layer as projection GEMM(s) + one recurrence launch on the
    nn.LSTM's own parameters (_LSTMLayerFn; its backward works in eval mode); everything else, and `fused = False`,
    runs the nn.LSTM modules themselves."""

    fused = True        # False: the nn.LSTM modules (fallback tests, tools/dlstm_feature_ab.py)

    def __init__(self, input_size: int, hidden_size: int, num_layers: int, dropout: float = 0.0,
                 bidirectional: bool = False) -> None:
        super().__init__()
        self.input_size = input_size
        self.hidden_size = hidden_size
        self.num_layers = num_layers
        self.dropout = dropout
        self.bidirectional = bidirectional
        self.lstm = nn.ModuleList()
        for _ in range(num_layers - 1):
            self.lstm.append(nn.LSTM(input_size=input_size, hidden_size=hidden_size, num_layers=1,
                                     bidirectional=bidirectional, batch_first=True))
            input_size = hidden_size * (2 if bidirectional else 1)
            if dropout > 0:
                self.lstm.append(nn.Dropout(p=dropout))
        self.lstm.append(nn.LSTM(input_size=input_size, hidden_size=hidden_size, num_layers=1,
                                 bidirectional=bidirectional, batch_first=True))

    def _layer(self, layer: nn.LSTM, x: torch.Tensor) -> torch.Tensor:
        hidden = layer.hidden_size
        names = [n for names in layer._all_weights for n in names]
        params = [getattr(layer, n) for n in names]
        if (self.fused and x.dim() == 3 and x.numel() > 0 and layer.bias and layer.proj_size == 0
                and hidden % 16 == 0 and LSTM_MIN_HIDDEN <= hidden <= LSTM_MAX_HIDDEN and _on_kernels(x, *params)
                and all(p.is_cuda for p in params)):
            return _LSTMLayerFn.apply(x.contiguous(), hidden, *params)
        return layer(x)[0]

    def forward(self, x: torch.Tensor, return_h: bool = True):
        """(x, h): the last layer's output (B, S, dirs H) and every layer's, (B, num_layers, S, dirs H), as the
        reference; return_h=False skips filling h and returns (x, None)."""
        h = torch.empty(self.num_layers, x.size(0), x.size(1), self.hidden_size * (2 if self.bidirectional else 1),
                        device=x.device) if return_h else None
        lstm_index = 0
        for layer in self.lstm:
            if isinstance(layer, nn.LSTM):
                x = self._layer(layer, x)
                if return_h:
                    h[lstm_index] = x
                lstm_index += 1
            else:
                x = layer(x)
        return x, (h.permute(1, 0, 2, 3) if return_h else None)


class DualDomainLSTM(FeatureNetwork):
    """feature_network.py:350-398: a VerboseLSTM on x, one on cat(rfft(x, dim=1).real, .imag) (S // 2 + 1 bins of
    2 input_size values), both pooled over dim 1 (mean or max), and a FullyConnectedFeatureNetwork on the concatenated
    (B, 2 H dirs) result."""

    def __init__(self, input_size: int, hidden_size: int, fc_sizes: list[int], fc_dropout: float = 0.0,
                 num_layers: int = 1, dropout: float = 0.0, bidirectional: bool = False, pooling: str = "mean") -> None:
        super().__init__()
        if pooling not in ("mean", "max"):
            raise ValueError(f"Invalid pooling method: {pooling}")
        self.input_size = input_size
        self.output_size = fc_sizes[-1]
        self.pooling = pooling
        self.lstm = VerboseLSTM(input_size, hidden_size, num_layers, dropout, bidirectional)
        self.frequency_lstm = VerboseLSTM(input_size * 2, hidden_size, num_layers, dropout, bidirectional)
        self.fc_sizes = [hidden_size * (2 if bidirectional else 1) * 2] + list(fc_sizes)
        self.fc = FullyConnectedFeatureNetwork(sizes=self.fc_sizes, dropout=fc_dropout)

    def _pool(self, x: torch.Tensor) -> torch.Tensor:
        if self.pooling == "mean":
            return x.mean(dim=1)
        if self.pooling == "max":
            return x.max(dim=1).values
        raise ValueError(f"Invalid pooling method: {self.pooling}")

    def combined(self, x: torch.Tensor) -> torch.Tensor:
        """The input of `fc`: (B, 2 H dirs) = [pooled time branch | pooled frequency branch]."""
        x_lstm, _ = self.lstm(x, return_h=False)
        freq = torch.fft.rfft(x, dim=1)
        x_freq, _ = self.frequency_lstm(torch.cat([freq.real, freq.imag], dim=-1), return_h=False)
        return torch.cat([self._pool(x_lstm), self._pool(x_freq)], dim=1)

    def forward(self, x: torch.Tensor) -> torch.Tensor:
        return self.fc(self.combined(x))


class FeatureNetworkStack(FeatureNetwork):
    def __init__(self, feature_networks: list[nn.Module | None] | None = None) -> None:
        super().__init__()
        if feature_networks is None or all(fn is None for fn in feature_networks):
            raise ValueError("Feature network stack must contain at least one feature network.")
        self.feature_networks = nn.Sequential(*[fn for fn in feature_networks if fn is not None])
        self.n_distinct_conditions = sum(isinstance(fn, ConcatenateCondition) for fn in self.feature_networks)
        self.input_size = getattr(self.feature_networks[0], "input_size", None)
        self.output_size = getattr(self.feature_networks[-1], "output_size", None)

    def forward(self, *conditions: torch.Tensor) -> torch.Tensor:
        if len(conditions) != self.n_distinct_conditions:
            raise ValueError(f"Expected {self.n_distinct_conditions} conditions, but got {len(conditions)}.")
        feats = None
        used = 0
        for fn in self.feature_networks:
            if isinstance(fn, ConcatenateCondition):
                c = conditions[used]
                feats = fn(c) if feats is None else fn(torch.cat([feats, c], dim=fn.dim))
                used += 1
            else:
                feats = fn(feats)
        return feats


FEATURE_NETWORKS: dict[str, Any] = {
    "FullyConnected": FullyConnectedFeatureNetwork,
    "LSTM": LSTMFeatureNetwork,
    "Transformer": Transformer,
    "DualDomainTransformer": DualDomainTransformer,
    "DualDomainLSTM": DualDomainLSTM,
    "ConcatenateCondition": ConcatenateCondition,
}
