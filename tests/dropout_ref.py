"""Test-side restatement of the FC_small kernels' dropout draw (bcnf_device.h: philox4x32_10, dropout_bits), numpy.

Not the reference's RNG: the reference draws nn.Dropout masks with torch's generator (cnf.py:82-83), which no
in-kernel generator can reproduce, so training parity is gated against the fp64 oracle fed the kernels' own masks
(keep_callable below hands them over). This module pins the kernel's own stream bit for bit:
Philox4x32-10 (Salmon et al. 2011, checked against the Random123 known-answer vectors in tests/test_dropout_rule.py)
and the keep rule "u32 >= round(p 2^32)". feature_keep restates the feature-MLP layers' draw (k_lin / k_gemm) the same
way, for the fp64 oracle of tests/test_gpu_linear.py. wide_keep_bits restates the wide family's two draw rules
(bcnf_wide.hip: drop4 in the link kernels, epi_rnd / epi4 in the chain GEMM's epilogue) and its truncating threshold;
tests/test_gpu_wide_dropout.py holds every mask of a launch to it, and wide_keep_callable feeds the fp64 oracle of
tests/test_gpu_train_parity.py.
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


# ------------------------------------------------------------------------------------------ wide family
# bcnf_wide.hip draws with two rules, both keyed (seed low, seed high ^ offset high) and both "keep iff u32 >= thresh":
#   layer 0 (the link kernels, drop4):      unit (row b, hidden unit c) is word c & 3 of the draw with counter
#                                           (b, (c & ~3) | 0x80000000, 16 v, offset low);
#   layers 1 .. NH - 1 (the chain GEMM's EPI_ACT epilogue, epi_rnd / epi4; tag set in hidden_fwd):
#                                           unit (row b, column c) is word b & 3 of the draw with counter
#                                           (b & ~3, c, 16 v + l, offset low).
# v is the virtual block (real block * S + side, S = 2 for two_way); BCNF_MAX_HIDDEN = 8 < 16, so no two tags meet.
# Every EPI_ACT instance holds its accumulators in groups of four consecutive rows that start at a multiple of 4, so
# the draw is a function of (seed, offset, v, l, b, c) alone, whatever GEMM tiling the dispatcher picks. The forward
# (saving or not, folded or not) and wide_inverse use the same tags; the inverse's rows are the latent rows.
def wide_thresh32(p):
    """(uint32_t)((double)float32(p) 2^32), clamped to 2^32 - 1 (wide_layout in bcnf_wide.hip): truncation, where the
    small family's thresh32 rounds to nearest. The two differ only for p < 2^-8, where float32(p) 2^32 has a
    fractional part."""
    t = float(np.float32(p)) * 4294967296.0                 # exact in binary64: a 24-bit significand times 2^32
    return 0xFFFFFFFF if t >= 4294967295.0 else int(t)


def wide_keep_bits(p, seed, offset, v, l, rows, H):
    """bool [rows, H]: the keep mask of hidden layer l (0 .. NH - 1) of virtual block v in one wide-family launch of
    `rows` rows at (seed, offset)."""
    seed, offset = int(seed) & (2**64 - 1), int(offset) & (2**64 - 1)
    assert 0 <= l < 16 and v >= 0 and rows >= 0 and H >= 0
    k0, k1 = seed & 0xFFFFFFFF, ((seed >> 32) ^ (offset >> 32)) & 0xFFFFFFFF
    olo = offset & 0xFFFFFFFF
    if l == 0:
        quads = (H + 3) // 4
        b = np.arange(rows, dtype=np.uint64)[:, None]
        c4 = (np.arange(quads, dtype=np.uint64)[None, :] * np.uint64(4)) | np.uint64(0x80000000)
        words = philox4x32_10(b, c4, 16 * v, olo, k0, k1)                        # four [rows, quads]
        u = np.stack([np.broadcast_to(w, (rows, quads)) for w in words], axis=2).reshape(rows, 4 * quads)[:, :H]
    else:
        quads = (rows + 3) // 4
        b4 = np.arange(quads, dtype=np.uint64)[:, None] * np.uint64(4)
        c = np.arange(H, dtype=np.uint64)[None, :]
        words = philox4x32_10(b4, c, 16 * v + l, olo, k0, k1)                    # four [quads, H]
        u = np.stack([np.broadcast_to(w, (quads, H)) for w in words], axis=1).reshape(4 * quads, H)[:rows]
    return u >= np.uint64(wide_thresh32(p))


def wide_keep_callable(p, seed, offset, n_blocks, two_way, hidden, rows):
    """The oracle's `keep` callable (oracle/cnf_oracle.py: model_forward / model_inverse / sample) for one wide-family
    launch of `rows` rows: keep(k, half, li) = bool [rows, hidden[li]] of virtual block v = k S + (half == "b"). Each
    mask is formed on first use and kept."""
    import torch
    hidden = list(hidden)
    S = 2 if two_way else 1
    cache = {}

    def keep(k, half, li):
        assert 0 <= k < n_blocks and half in ("a", "b")[:S] and 0 <= li < len(hidden)
        v = k * S + (half == "b")
        if (v, li) not in cache:
            cache[v, li] = torch.from_numpy(wide_keep_bits(p, seed, offset, v, li, rows, hidden[li]))
        return cache[v, li]
    return keep


# The small-family (register-resident k_forward / k_backward / k_inverse) shapes the training-parity tests use besides
# FC_small: NH = 8 (the second-draw path), hidden widths below 16 with NH = 2 and no ActNorm, NH = 1 with a padded C,
# NH = 8 with width 4.
SMALL_TRAIN_SHAPES = {
    "nh8_p50": dict(size=19, nested_sizes=[16] * 8, n_blocks=3, n_conditions=80, dropout=0.5, act_norm=True),
    "d7_h12_9": dict(size=7, nested_sizes=[12, 9], n_blocks=3, n_conditions=5, dropout=0.1, act_norm=False),
    "d32_nh1": dict(size=32, nested_sizes=[16], n_blocks=2, n_conditions=120, dropout=0.25, act_norm=True),
    "d2_h4x8": dict(size=2, nested_sizes=[4] * 8, n_blocks=5, n_conditions=3, dropout=0.3, act_norm=True),
    # The template arms NH = 3 .. 6 and the shape edges no other case reaches (tests/small_arms.py names the arm each
    # one takes; tests/test_small_arms_cpu.py holds the lists to them). Each of these runs at a weight gain
    # (SMALL_TRAIN_GAIN), so that no gated tensor sits below its gate's absolute floor.
    # NH = 4 (ActRec 2 + 3); 12 / 12, the last PERM layout; C = 17: Cp = 32, rows not 16-byte aligned (non-VEC)
    "nh4_d24_c17": dict(size=24, nested_sizes=[16] * 4, n_blocks=3, n_conditions=17, dropout=0.2, act_norm=True),
    # NH = 5 (3 + 1; the second dropout float4 opens); 13 / 12, the first non-PERM layout; uneven widths; C = KC
    "nh5_d25_c128": dict(size=25, nested_sizes=[16, 7, 16, 3, 11], n_blocks=4, n_conditions=128, dropout=0.3,
                         act_norm=True),
    # NH = 6 (3 + 3; BwdJobs' exact fill); 10 / 10 without the 10 / 9 broadcast form; C = KC + 1; NKp = 128
    "nh6_d20_c129": dict(size=20, nested_sizes=[16] * 6, n_blocks=5, n_conditions=129, dropout=0.25, act_norm=True),
    # Da = 2, Db = 1; C = 1; no ActNorm
    "nh6_d3_c1": dict(size=3, nested_sizes=[5] * 6, n_blocks=2, n_conditions=1, dropout=0.1, act_norm=False),
    # 16 / 15; the widest C, in training
    "nh4_d31_c208": dict(size=31, nested_sizes=[16] * 4, n_blocks=2, n_conditions=208, dropout=0.4, act_norm=True),
    # NH = 3 in training (no other oracle-gated training case has it), on the 10 / 9 broadcast form
    "nh3_d19_c80": dict(size=19, nested_sizes=[16] * 3, n_blocks=4, n_conditions=80, dropout=0.2, act_norm=True),
    # nh8_p50 and d2_h4x8 again, at inputs their gates can see
    "nh8_p50_g2": dict(size=19, nested_sizes=[16] * 8, n_blocks=3, n_conditions=80, dropout=0.5, act_norm=True),
    "d2_h4x8_g3": dict(size=2, nested_sizes=[4] * 8, n_blocks=5, n_conditions=3, dropout=0.3, act_norm=True),
    # behind ConcatenateCondition(X) + FullyConnected [X, C] (SMALL_TRAIN_FOLD_X): the pack-free folded forward at
    # layouts other than FC_small's (fold_nh8_d22: every limit of its table at once), and the two-launch form at NH = 4
    "fold_nh6_d19": dict(size=19, nested_sizes=[16] * 6, n_blocks=3, n_conditions=80, dropout=0.3, act_norm=True),
    "fold_nh8_d22": dict(size=22, nested_sizes=[16] * 8, n_blocks=2, n_conditions=128, dropout=0.2, act_norm=True),
    "fold_nh5_d18": dict(size=18, nested_sizes=[16] * 5, n_blocks=3, n_conditions=13, dropout=0.3, act_norm=True),
    "fold_nh4_d24": dict(size=24, nested_sizes=[16] * 4, n_blocks=3, n_conditions=17, dropout=0.2, act_norm=True),
}
# apply_gain's factor per shape (absent: the weights stay as drawn)
SMALL_TRAIN_GAIN = {"nh4_d24_c17": 2.0, "nh5_d25_c128": 2.0, "nh6_d20_c129": 2.0, "nh6_d3_c1": 2.5,
                    "nh4_d31_c208": 2.0, "nh3_d19_c80": 2.0, "nh8_p50_g2": 2.0, "d2_h4x8_g3": 3.0,
                    "fold_nh6_d19": 2.0, "fold_nh8_d22": 2.0, "fold_nh5_d18": 2.0, "fold_nh4_d24": 2.0}
# in_features X of the single feature Linear [X, C] of the folded shapes (the input is (X / 3, 3) per sample), and
# whether the pack-free forward's table applies to the layout (fold_nh4_d24: D^2 = 576 > 512 Q slots)
SMALL_TRAIN_FOLD_X = {"fold_nh6_d19": 90, "fold_nh8_d22": 96, "fold_nh5_d18": 21, "fold_nh4_d24": 21}
SMALL_TRAIN_RAW = {"fold_nh6_d19": True, "fold_nh8_d22": True, "fold_nh5_d18": True, "fold_nh4_d24": False}


def shape_config(shape):
    """from_config dict of a coupling stack fed its condition directly (ConcatenateCondition only: h = the condition)."""
    return {"global": {"parameter_selection": [f"p{i}" for i in range(shape["size"])]},
            "model": {"kwargs": dict(shape)},
            "feature_networks": [{"type": "ConcatenateCondition",
                                  "kwargs": {"input_size": None, "output_size": shape["n_conditions"]}}]}


def fold_config(shape, X):
    """from_config dict of the stack behind ConcatenateCondition(X) + FullyConnected [X, C] without feature dropout:
    the single nn.Linear the folded training path takes in."""
    cfg = shape_config(shape)
    cfg["feature_networks"] = [{"type": "ConcatenateCondition", "kwargs": {"input_size": None, "output_size": X}},
                               {"type": "FullyConnected", "kwargs": {"sizes": [X, shape["n_conditions"]],
                                                                     "dropout": 0.0}}]
    return cfg


def apply_gain(target, gain):
    """Multiply every 2-D `layers.*` weight (the coupling MLPs' Linears; never an orthonormal_matrix) of a model or
    of a state dict (torch tensors or numpy arrays) by `gain`, in place; returns `target`. With default nn.Linear
    init every GELU layer shrinks the signal, and at NH >= 6 the deepest gradients fall below the absolute floor of
    their gate (conftest.close), where zeros pass; a gain of 2 .. 3 keeps them above it. Call it after the weights
    are set and before the oracle's copy is taken, so model and oracle hold the same values."""
    import torch
    items = target.items() if isinstance(target, dict) else target.state_dict().items()
    with torch.no_grad():
        for k, v in items:
            if k.startswith("layers.") and v.ndim == 2 and not k.endswith("orthonormal_matrix"):
                v *= gain                        # state_dict() tensors share the parameters' storage
    return target
