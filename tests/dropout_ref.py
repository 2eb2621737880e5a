"""Test-side restatement of the FC_small kernels' dropout draw (bcnf_device.h: philox4x32_10, dropout_bits), numpy.

Not the reference's RNG: the reference draws nn.Dropout masks with torch's generator (cnf.py:82-83), which no
in-kernel generator can reproduce, so training parity is gated against the fp64 oracle fed the kernels' own masks
(keep_callable below hands them over). This module pins the kernel's own stream bit for bit:
Philox4x32-10 (Salmon et al. 2011, checked against the Random123 known-answer vectors in tests/test_dropout_rule.py)
and the keep rule "u32 >= round(p 2^32)". feature_keep restates the feature-MLP layers' draw (k_lin / k_gemm) the same
way, for the fp64 oracle of tests/test_gpu_linear.py.
"""
import numpy as np

_M0, _M1 = np.uint64(0xD2511F53), np.uint64(0xCD9E8D57)
_W0, _W1 = np.uint64(0x9E3779B9), np.uint64(0xBB67AE85)
_U32 = np.uint64(0xFFFFFFFF)


def philox4x32_10(c0, c1, c2, c3, k0, k1):
    """Vectorised Philox4x32-10 on uint32-valued arrays (any broadcastable shapes); returns four uint64 arrays."""
    c0, c1, c2, c3, k0, k1 = (np.asarray(v, dtype=np.uint64) & _U32 for v in (c0, c1, c2, c3, k0, k1))
    for _ in range(10):
        p0 = _M0 * c0
        p1 = _M1 * c2
        c0, c1, c2, c3 = (p1 >> np.uint64(32)) ^ c1 ^ k0, p1 & _U32, (p0 >> np.uint64(32)) ^ c3 ^ k1, p0 & _U32
        k0 = (k0 + _W0) & _U32
        k1 = (k1 + _W1) & _U32
    return c0, c1, c2, c3


def thresh32(p):
    """round(p 2^32) of the float32 p the library stores (BcnfStackDesc.dropout), clamped to 2^32 - 1."""
    return int(min(4294967295.0, np.floor(float(np.float32(p)) * 4294967296.0 + 0.5)))


def _halves(r):
    out = []
    for w in r:
        out += [w & np.uint64(0xFFFF), w >> np.uint64(16)]
    return out                                        # the 8 16-bit halves in the kernel's unit order


def keep_bits(p, seed, offset, sample, block, lane, tag=0, nu=7):
    """uint32 array of keep bits per (sample, block, lane) (broadcast) for a stack of nu hidden layers, bit i = unit i
    (hidden layer i + 1): keep iff u_i >= thresh32(p), u_i = (high 16 bits: half i of the draw, low 16 bits: the draw's
    eighth half when nu < 8, else half i of a second draw with counter tag bit 29)."""
    seed, offset = int(seed) & (2**64 - 1), int(offset) & (2**64 - 1)
    sample = np.asarray(sample, dtype=np.int64).astype(np.uint64)
    block = np.asarray(block, dtype=np.uint64)
    lane = np.asarray(lane, dtype=np.uint64)
    c1 = ((sample >> np.uint64(32)) ^ (block << np.uint64(8)) ^ np.uint64(tag)) & _U32
    k0, k1 = seed & 0xFFFFFFFF, ((seed >> 32) ^ (offset >> 32)) & 0xFFFFFFFF
    hi = _halves(philox4x32_10(sample & _U32, c1, lane, offset & 0xFFFFFFFF, k0, k1))
    if nu < 8:
        lo = [hi[7]] * 8
    else:
        lo = _halves(philox4x32_10(sample & _U32, c1 ^ np.uint64(0x20000000), lane, offset & 0xFFFFFFFF, k0, k1))
    t = np.uint64(thresh32(p))
    bits = np.zeros(np.broadcast(sample, block, lane).shape, dtype=np.uint32)
    for i in range(nu):
        u = (hi[i] << np.uint64(16)) | lo[i]
        bits |= (u >= t).astype(np.uint32) << np.uint32(i)
    return bits


def launch_sample(batch, workgroups=None):
    """Sample index dropout_bits sees per launch row (k_forward / k_inverse: bc = min(b, B - 1)): rows past the batch
    in the last 16-sample workgroup replay the last sample, masks included."""
    rows = batch if workgroups is None else 16 * workgroups
    return np.minimum(np.arange(rows), batch - 1)


def keep_callable(p, seed, offset, n_blocks, hidden, batch, tag=0):
    """The oracle's `keep` callable (oracle/cnf_oracle.py: model_forward / model_inverse) for one small-family launch:
    keep(k, "a", li) = bool [batch, hidden[li]], unit (sample b, block k, lane j, hidden layer li + 1) of keep_bits.
    The counter is (sample = launch row, block = coupling number, lane = hidden unit j of the 16-lane row layout);
    tag 0 for k_forward, 0x40000000 for the training-mode k_inverse. The small family has no two_way couplings."""
    import torch
    hidden = list(hidden)
    bits = keep_bits(p, seed, offset, launch_sample(batch)[None, :, None], np.arange(n_blocks)[:, None, None],
                     np.arange(16)[None, None, :], tag=tag, nu=len(hidden))          # [block][sample][lane]

    def keep(k, half, li):
        assert half == "a" and 0 <= k < n_blocks and 0 <= li < len(hidden)
        return torch.from_numpy(((bits[k, :, :hidden[li]] >> np.uint32(li)) & np.uint32(1)).astype(bool))
    return keep


def feature_keep(p, seed, offset, salt, rows, cols):
    """bool [rows, cols] keep mask of one fused feature layer (bcnf_train.hip: the ACT epilogue of k_lin / k_gemm,
    bcnf_linear_gelu_forward): unit (row, column) is word row & 3 of the draw with counter (column, row >> 2, offset
    low, offset high) and key (seed low ^ salt 0x9E3779B9, seed high ^ 0x80000000); keep iff u32 >= thresh32(p)."""
    seed, offset = int(seed) & (2**64 - 1), int(offset) & (2**64 - 1)
    k0 = (seed & 0xFFFFFFFF) ^ (((int(salt) & 0xFFFFFFFF) * 0x9E3779B9) & 0xFFFFFFFF)
    k1 = ((seed >> 32) ^ 0x80000000) & 0xFFFFFFFF
    quads = (rows + 3) // 4
    col = np.arange(cols, dtype=np.uint64)[None, :]
    quad = np.arange(quads, dtype=np.uint64)[:, None]
    words = philox4x32_10(col, quad, offset & 0xFFFFFFFF, offset >> 32, k0, k1)      # four [quads, cols]
    u = np.stack([np.broadcast_to(w, (quads, cols)) for w in words], axis=1).reshape(4 * quads, cols)[:rows]
    return u >= np.uint64(thresh32(p))


# The small-family (register-resident k_forward / k_backward / k_inverse) shapes the training-parity tests use besides
# FC_small: NH = 8 (the second-draw path), hidden widths below 16 with NH = 2 and no ActNorm, NH = 1 with a padded C,
# NH = 8 with width 4.
SMALL_TRAIN_SHAPES = {
    "nh8_p50": dict(size=19, nested_sizes=[16] * 8, n_blocks=3, n_conditions=80, dropout=0.5, act_norm=True),
    "d7_h12_9": dict(size=7, nested_sizes=[12, 9], n_blocks=3, n_conditions=5, dropout=0.1, act_norm=False),
    "d32_nh1": dict(size=32, nested_sizes=[16], n_blocks=2, n_conditions=120, dropout=0.25, act_norm=True),
    "d2_h4x8": dict(size=2, nested_sizes=[4] * 8, n_blocks=5, n_conditions=3, dropout=0.3, act_norm=True),
}


def shape_config(shape):
    """from_config dict of a coupling stack fed its condition directly (ConcatenateCondition only: h = the condition)."""
    return {"global": {"parameter_selection": [f"p{i}" for i in range(shape["size"])]},
            "model": {"kwargs": dict(shape)},
            "feature_networks": [{"type": "ConcatenateCondition",
                                  "kwargs": {"input_size": None, "output_size": shape["n_conditions"]}}]}
