"""Inputs and restatements shared by tests/test_resim_stats_cpu.py and tests/test_gpu_resim_stats.py.

`kernel_error` and `kernel_impacts` restate, in plain Python / numpy scalars, what include/bcnf_amd.h says the two
kernels of bcnf_amd/csrc/bcnf_resim_stats.hip compute (the per-draw mean in index order, the median as a sort of the
bit patterns with NaN above +inf, the searchsorted bin rule). The CPU tests hold them against numpy's own
nanmean / nanmedian / histogram2d, so the definition the kernels implement is checked where no GPU is needed; the
GPU tests hold the kernels against numpy directly.
"""
import numpy as np

BINS = np.linspace(-42, 42, 128)          # the notebook's hist2d edges


def kernel_error(x, observed):
    x = np.asarray(x, dtype=np.float64)
    o = np.asarray(observed).astype(np.float64)
    n, m, s, _ = x.shape
    out = np.full((n, s), np.nan)
    nan_key = np.uint64(0xFFFFFFFFFFFFFFFF)
    with np.errstate(all="ignore"):
        for i in range(n):
            for t in range(s):
                keys = np.full(m, nan_key, dtype=np.uint64)
                for j in range(m):
                    total, count = np.float64(0.0), 0
                    for k in range(3):
                        d = x[i, j, t, k] - o[i, t, k]
                        sq = d * d
                        if sq == sq:
                            total = total + sq
                            count += 1
                    if count:
                        keys[j] = (total / np.float64(count)).view(np.uint64)
                keys.sort()
                c = int((keys != nan_key).sum())
                if c % 2:
                    out[i, t] = keys[c // 2].view(np.float64)
                elif c:
                    out[i, t] = (keys[c // 2 - 1].view(np.float64) + keys[c // 2].view(np.float64)) / np.float64(2.0)
    return out


def kernel_bin(edges, v):
    """np.searchsorted(edges, v, 'right') - 1, the last edge in the last bin, -1 outside / NaN."""
    if not (v >= edges[0]) or not (v <= edges[-1]):
        return -1
    lo = sum(1 for e in edges if e <= v)
    return len(edges) - 2 if lo == len(edges) else lo - 1


def kernel_impacts(x, edges=None):
    x = np.asarray(x, dtype=np.float64)
    n, m, s, _ = x.shape
    step = np.full((n, m), -1, dtype=np.int32)
    position = np.full((n, m, 3), np.nan)
    transitions = np.zeros((n, m), dtype=np.int32)
    hist = None if edges is None else np.zeros((n, len(edges) - 1, len(edges) - 1), dtype=np.int32)
    for i in range(n):
        for j in range(m):
            for t in range(s - 1):
                if x[i, j, t, 2] > 0 and not x[i, j, t + 1, 2] > 0:
                    if step[i, j] < 0:
                        step[i, j] = t
                        position[i, j] = x[i, j, t]
                    transitions[i, j] += 1
                    if hist is not None:
                        bx, by = kernel_bin(edges, x[i, j, t, 0]), kernel_bin(edges, x[i, j, t, 1])
                        if bx >= 0 and by >= 0:
                            hist[i, bx, by] += 1
    return {"step": step, "position": position, "transitions": transitions, "hist": hist}


def notebook_error(x, observed):
    """The notebook's statement, literally."""
    import warnings
    X_resim, X = x, np.asarray(observed).astype(np.float64)
    with warnings.catch_warnings(), np.errstate(all="ignore"):
        warnings.simplefilter("ignore", RuntimeWarning)
        return np.nanmedian(np.nanmean((X_resim - X[:, None])**2, axis=3), axis=1)


def notebook_impacts(x, i):
    """The notebook's statement for trajectory i, literally: (draw, step) index arrays."""
    X_resim = x
    return np.where(np.diff((X_resim[i, :, :, -1] > 0).astype(int), axis=1) == -1)


# z patterns by draw (j % 7), each a function of the number of steps: signs of z, 0 = exactly zero, nan = NaN
def _z_signs(kind, s, rng):
    z = np.ones(s)
    if kind == 0:                      # no transition
        pass
    elif kind == 1:                    # transition at s = 0 (onto z == 0: not above)
        z[1:] = -1
        if s > 1:
            z[1] = 0
    elif kind == 2:                    # transition at s = S - 2
        z[s - 1:] = -1
    elif kind == 3:                    # two transitions (0 and 2) when S >= 4
        z[1::2] = -1
        z[4:] = -1
    elif kind == 4:                    # NaN from some step on: above -> NaN counts as a transition
        z[(s + 1) // 2:] = np.nan
    elif kind == 5:                    # starts below ground, rises, falls
        z[0] = -1
        z[3:] = -1
    else:
        z = np.sign(rng.standard_normal(s))
    return z


def make_case(n, m, s, seed, obs_dtype=np.float32, edges=BINS):
    """x (n, m, s, 3) float64 and observed (n, s, 3) of obs_dtype with every special column the issue names, all
    finite values <= 1e300."""
    rng = np.random.Generator(np.random.PCG64(seed))
    x = rng.standard_normal((n, m, s, 3)) * np.array([25.0, 25.0, 1.0])
    obs = (rng.standard_normal((n, s, 3)) * 10).astype(obs_dtype)
    mag = rng.uniform(0.1, 5.0, (n, m, s))
    for j in range(m):
        for i in range(n):
            x[i, j, :, 2] = _z_signs((j + i) % 7, s, rng) * mag[i, j]
    # positions of the s = 0 transitions (kind 1) on, at and just outside the edges, NaN and inf
    special = [edges[0], edges[-1], edges[len(edges) // 2], np.nextafter(edges[-1], np.inf),
               np.nextafter(edges[0], -np.inf), np.nan, np.inf, -np.inf, edges[1], 0.0]
    for i in range(n):
        for j in range(m):
            if (j + i) % 7 == 1:
                q = (j // 7) % (2 * len(special))
                x[i, j, 0, q % 2] = special[q // 2]
    # error columns
    x[0, :, 0, :2] = np.nan                                     # (0, 0): NaN in two components of every draw ...
    x[0, ::2, 0, 2] = np.nan                                    # ... and all three in every other one
    if s > 1:
        x[0, :, 1, :] = np.nan                                  # an all-NaN column
        x[n - 1, ::3, s - 1, :] = np.nan                        # M - ceil(M / 3) values left
        x[n - 1, 1::5, s - 1, 1] = np.nan                       # a NaN in one component only
    if s > 2:
        x[0, : m // 2 + 1, 2, :] = x[0, 0, 2, :]                # ties
        x[0, m // 2:, 2, 0] = np.inf                            # +inf values (with ties among them)
        x[n - 1, :1, 2, :] = np.nan                             # M - 1 values: the other parity
        x[n - 1, 1::2, 2, :] = obs[n - 1, 2].astype(np.float64)   # zeros
        if s > 4:
            obs[0, 3, 2] = np.nan                               # a NaN in the observation: count 2 for every draw
            obs[n - 1, 4, :] = np.nan                           # ... and an all-NaN column from the observation
    return x, obs
