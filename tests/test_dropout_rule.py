"""CPU checks of the FC_small kernels' dropout rule as restated in tests/dropout_ref.py (the GPU kernels are checked
bit for bit against it in tests/test_gpu_dropout.py): Philox4x32-10 against the Random123 known-answer vectors, and
the keep rule's effective p equal to nn.Dropout's p (cnf.py:82-83) to 2^-32 at every p, including p < 2^-17, which
round 5's 16-bit rule ran as no dropout at all. The feature layers' draw (feature_keep; the GPU kernels against it
in tests/test_gpu_linear.py): its counter / key layout unit by unit, p = 0, the keep rate, and that the salt and both
halves of the offset reach the draw. The wide family's two rules (wide_keep_bits; the GPU kernels against it in
tests/test_gpu_wide_dropout.py): each against its sentence-level statement unit by unit, no (counter, word) pair used
twice in a launch, the truncating threshold, the keep rate, and that every input of the draw reaches it."""
import numpy as np
import pytest

from dropout_ref import (feature_keep, keep_bits, philox4x32_10, thresh32, wide_keep_bits, wide_keep_callable,
                         wide_thresh32)


@pytest.mark.parametrize("ctr,key,out", [
    ((0, 0, 0, 0), (0, 0), (0x6627E8D5, 0xE169C58D, 0xBC57AC4C, 0x9B00DBD8)),
    ((0xFFFFFFFF,) * 4, (0xFFFFFFFF,) * 2, (0x408F276D, 0x41C83B0E, 0xA20BC7C6, 0x6D5451FD)),
    ((0x243F6A88, 0x85A308D3, 0x13198A2E, 0x03707344), (0xA4093822, 0x299F31D0),
     (0xD16CFE09, 0x94FDCCEB, 0x5001E420, 0x24126EA1)),
])
def test_philox_known_answers(ctr, key, out):
    got = philox4x32_10(*ctr, *key)
    assert tuple(int(v) for v in got) == out


@pytest.mark.parametrize("p", [0.383, 0.244, 0.407, 1e-6, 3e-9, 0.5, 0.0])
def test_threshold_is_p_to_2_pow_32(p):
    t = thresh32(p)
    assert abs(t / 2**32 - float(np.float32(p))) <= 2.0**-33
    if p > 0:
        assert t > 0                                   # round 5: round(p 2^16) = 0 for p < 2^-17


def test_keep_rule_statistics():
    """7M units at p = 0.383 (7 units per draw, the eighth half the shared low half): the drop fraction within 4 sigma
    of p; at p = 1e-6 over 64M units of 8-unit draws the drops are Poisson(64) within 4 sigma (the second-draw tie
    path, high half == 0, decides every one of them)."""
    rng = np.random.default_rng(5)
    s = rng.integers(0, 2**40, size=1 << 20)
    b = keep_bits(0.383, 1234, 77, s, 3, 5)
    drop = 7 * b.size - int(np.unpackbits(b.view(np.uint8)).sum())
    n = 7 * b.size
    assert abs(drop / n - 0.383) < 4 * np.sqrt(0.383 * 0.617 / n)
    drops = 0
    for blk in range(8):
        b = keep_bits(1e-6, 99, 3, s, blk, 7, nu=8)
        drops += 8 * b.size - int(np.unpackbits(b.view(np.uint8)).sum())
    n = 8 * 8 * s.size
    lam = 1e-6 * n
    assert drops > 0 and abs(drops - lam) < 4 * np.sqrt(lam), (drops, lam)


FEATURE_STATE = (0x123456789ABCDEF, 2**32 + 5)           # (seed, offset): both halves of both nonzero


def test_feature_keep_layout_unit_by_unit():
    """The vectorised mask against the rule written out per unit: counter (column, row >> 2, offset low, offset
    high), key (seed low ^ salt 0x9E3779B9, seed high ^ 0x80000000), word row & 3."""
    seed, offset = FEATURE_STATE
    p, salt, rows, cols = 0.3, 6, 11, 5
    got = feature_keep(p, seed, offset, salt, rows, cols)
    assert got.shape == (rows, cols) and got.dtype == np.bool_
    k0 = (seed & 0xFFFFFFFF) ^ ((salt * 0x9E3779B9) & 0xFFFFFFFF)
    k1 = (seed >> 32) ^ 0x80000000
    for r in range(rows):
        for c in range(cols):
            w = philox4x32_10(c, r >> 2, offset & 0xFFFFFFFF, offset >> 32, k0, k1)
            assert bool(got[r, c]) == (int(w[r & 3]) >= thresh32(p)), (r, c)


def test_feature_keep_p0_keeps_everything():
    assert feature_keep(0.0, *FEATURE_STATE, 3, 37, 33).all()


@pytest.mark.parametrize("p", [0.111, 0.5])
def test_feature_keep_rate(p):
    keep = feature_keep(p, *FEATURE_STATE, 3, 1024, 1024)          # 2^20 units
    n, q = keep.size, 1.0 - thresh32(p) / 2**32
    assert n >= 10**6
    assert abs(keep.mean() - q) < 4 * np.sqrt(q * (1 - q) / n), (keep.mean(), q)


def test_feature_keep_salt_and_offset_halves_reach_the_draw():
    seed, offset = FEATURE_STATE
    base = feature_keep(0.5, seed, offset, 3, 64, 64)
    assert np.array_equal(base, feature_keep(0.5, seed, offset, 3, 64, 64))
    for other in (feature_keep(0.5, seed, offset, 4, 64, 64),              # salt
                  feature_keep(0.5, seed, offset + 1, 3, 64, 64),          # offset, low half
                  feature_keep(0.5, seed, offset + 2**32, 3, 64, 64),      # offset, high half
                  feature_keep(0.5, seed ^ 1, offset, 3, 64, 64),          # seed, low half
                  feature_keep(0.5, seed ^ 2**32, offset, 3, 64, 64)):     # seed, high half
        assert 0.4 < (other != base).mean() < 0.6                          # an independent draw, not a shift


# ------------------------------------------------------------------------------------------ wide family
WIDE_STATE = (0xA11CE00000123, (5 << 32) + 3)             # (seed, offset): both halves of both nonzero


def _wide_unit(p, seed, offset, v, l, b, c):
    """The rule as DESIGN.md section 4 states it, one unit at a time."""
    k0, k1 = seed & 0xFFFFFFFF, (seed >> 32) ^ (offset >> 32)
    if l == 0:
        ctr, word = (b, (c & ~3) | 0x80000000, 16 * v, offset & 0xFFFFFFFF), c & 3
    else:
        ctr, word = (b & ~3, c, 16 * v + l, offset & 0xFFFFFFFF), b & 3
    return ctr, word, int(philox4x32_10(*ctr, k0, k1)[word]) >= wide_thresh32(p)


@pytest.mark.parametrize("v,l", [(0, 0), (3, 0), (0, 1), (5, 7)])
def test_wide_keep_layout_unit_by_unit(v, l):
    """Ragged in both directions: rows = 11 leaves a three-row last group, H = 5 a one-unit last quad."""
    seed, offset = WIDE_STATE
    p, rows, H = 0.3, 11, 5
    got = wide_keep_bits(p, seed, offset, v, l, rows, H)
    assert got.shape == (rows, H) and got.dtype == np.bool_
    for b in range(rows):
        for c in range(H):
            assert bool(got[b, c]) == _wide_unit(p, seed, offset, v, l, b, c)[2], (b, c)


def test_wide_keep_callable_maps_blocks_and_halves():
    seed, offset = WIDE_STATE
    keep = wide_keep_callable(0.3, seed, offset, 3, True, [9, 9], 11)
    for k in range(3):
        for s, half in enumerate("ab"):
            for li in range(2):
                m = keep(k, half, li)
                assert m.dtype.is_floating_point is False and tuple(m.shape) == (11, 9)
                assert np.array_equal(m.numpy(), wide_keep_bits(0.3, seed, offset, 2 * k + s, li, 11, 9))
    one = wide_keep_callable(0.3, seed, offset, 3, False, [9, 7], 4)
    assert np.array_equal(one(2, "a", 1).numpy(), wide_keep_bits(0.3, seed, offset, 2, 1, 4, 7))
    with pytest.raises(AssertionError):
        one(0, "b", 0)                                     # a one-way stack has no second half


def test_wide_draws_of_a_launch_are_distinct():
    """NH = 8 (the largest tag), two_way, nb = 3, rows = 9, H = 9: every unit of the launch has its own (counter,
    word) pair, layer 0 against the chain layers included (bit 31 of the second counter word separates them)."""
    seed, offset = WIDE_STATE
    NH, nv, rows, H = 8, 6, 9, 9
    seen = set()
    for v in range(nv):
        for l in range(NH):
            for b in range(rows):
                for c in range(H):
                    ctr, word, _ = _wide_unit(0.5, seed, offset, v, l, b, c)
                    seen.add((ctr, word))
    assert len(seen) == nv * NH * rows * H


def test_wide_threshold_truncates():
    assert wide_thresh32(0.0) == 0
    for v, l in ((0, 0), (2, 3)):
        assert wide_keep_bits(0.0, *WIDE_STATE, v, l, 37, 33).all()
    for p in (0.2, 0.3, 0.407, 0.5, 1e-6):
        t = wide_thresh32(p)
        assert 0 <= float(np.float32(p)) - t / 2**32 < 2.0**-32, p      # truncated, never rounded up
    assert wide_thresh32(1e-6) > 0
    assert wide_thresh32(1e-6) == 4294 and thresh32(1e-6) == 4295        # float32(1e-6) 2^32 = 4294.967...
    assert wide_thresh32(1.0) == 0xFFFFFFFF


@pytest.mark.parametrize("p", [0.111, 0.5])
@pytest.mark.parametrize("l", [0, 2])
def test_wide_keep_rate(p, l):
    keep = wide_keep_bits(p, *WIDE_STATE, 1, l, 1024, 1024)          # 2^20 units
    n, q = keep.size, 1.0 - wide_thresh32(p) / 2**32
    assert n >= 10**6
    assert abs(keep.mean() - q) < 4 * np.sqrt(q * (1 - q) / n), (keep.mean(), q)


@pytest.mark.parametrize("l", [0, 2])
def test_wide_every_input_reaches_the_draw(l):
    seed, offset = WIDE_STATE
    base = wide_keep_bits(0.5, seed, offset, 1, l, 64, 64)
    assert np.array_equal(base, wide_keep_bits(0.5, seed, offset, 1, l, 64, 64))
    others = [wide_keep_bits(0.5, seed ^ 1, offset, 1, l, 64, 64),           # seed, low half
              wide_keep_bits(0.5, seed ^ 2**32, offset, 1, l, 64, 64),       # seed, high half
              wide_keep_bits(0.5, seed, offset + 1, 1, l, 64, 64),           # offset, low half
              wide_keep_bits(0.5, seed, offset + 2**32, 1, l, 64, 64),       # offset, high half
              wide_keep_bits(0.5, seed, offset, 2, l, 64, 64),               # the virtual block
              wide_keep_bits(0.5, seed, offset, 1, 1 if l else 3, 64, 64)]   # the layer (rule 0 against a chain layer too)
    for other in others:
        assert 0.4 < (other != base).mean() < 0.6                            # an independent draw, not a shift
    assert np.array_equal(base[:37, :33], wide_keep_bits(0.5, seed, offset, 1, l, 37, 33))    # not the launch's size
