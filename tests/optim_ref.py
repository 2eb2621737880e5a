"""Float64 restatement of the optimizer step, for the tests of the Adam / clip kernels (tests/test_gpu_optim.py), and
the inputs those tests use. Plain numpy and torch: nothing of the project is imported here, and
tests/test_optim_ref_cpu.py pins the restatement to torch's own float64 results.

adam64   torch/optim/adam.py::_single_tensor_adam (L2 weight decay, amsgrad = maximize = False), elementwise
clip64   torch.nn.utils.clip_grad_norm_ (2-norm): coef = min(max_norm / (norm + 1e-6), 1)
sumsq64  float64 sum of squared gradients
"""
import functools
import math

import numpy as np
import torch

CHUNK = 1024            # elements per workgroup and group of the kernels under test
MAX_TENSORS = 48
LR, EPS = 2e-3, 1e-8
BETAS = ((0.9, 0.999), (0.5, 0.9))
WDS = (0.0, 0.01)
STEP0S = (0, 7, 5000)

# element counts per tensor
LISTS = {
    "seams": [1, 3, 4, 1021, 2, 1024, 5, 0, 2049, 7],
    "views": [1030] * 5,
    "one_wg_1023": [1023],
    "one_wg_1024": [1024],
    "one_wg_1025": [1025],
    "max_tensors": [37] * MAX_TENSORS,
    "prereduce_g1": [2_000_003, 2050 * 1024 + 5 - 2_000_003],
    "g2_exact": [(1 << 22) - 1_234_567, 1_234_567],
    "g2_ragged": [1_000_001, 2_000_003, (1 << 22) + 2048 + 3 - 3_000_004],
}
SMALL = ("seams", "views", "one_wg_1023", "one_wg_1024", "one_wg_1025", "max_tensors")
LARGE = ("prereduce_g1", "g2_exact", "g2_ragged")
# float offset of (p, g, m, v) of each `views` tensor from a 16-byte aligned address: all aligned; all off alike; all
# different (twice); only v off
VIEW_OFFSETS = [(0, 0, 0, 0), (1, 1, 1, 1), (0, 1, 2, 3), (3, 0, 1, 0), (0, 0, 0, 1)]


def adam64(p, g, m, v, step_next, lr, b1, b2, eps, wd):
    """One Adam step on float64 arrays; step_next = the step count after this step. Returns the new (p, m, v)."""
    p, g, m, v = (np.asarray(a, dtype=np.float64) for a in (p, g, m, v))
    if wd != 0:
        g = g + wd * p
    m = m + (g - m) * (1.0 - b1)
    v = v * b2 + (1.0 - b2) * g * g
    bc1 = 1.0 - b1 ** step_next
    bc2 = 1.0 - b2 ** step_next
    denom = np.sqrt(v) / math.sqrt(bc2) + eps
    p = p - (lr / bc1) * (m / denom)
    return p, m, v


def sumsq64(grads):
    return float(sum(float(np.sum(np.asarray(g, dtype=np.float64) ** 2)) for g in grads))


def clip64(grads, max_norm):
    """(total norm, coef, clipped float64 gradients)."""
    norm = math.sqrt(sumsq64(grads))
    coef = min(max_norm / (norm + 1e-6), 1.0)
    return norm, coef, [np.asarray(g, dtype=np.float64) * coef for g in grads]


# ---- inputs (flat over the concatenated index space; the tests cut them at the tensor seams) ----------------------
@functools.lru_cache(maxsize=None)
def state_inputs(n, seed=0):
    """fp32 (p, m, v): |p| ~ 1 and never 0, m ~ 1e-2, v ~ 1e-4 U(0, 1) with v = 0 at every 11th element."""
    rng = np.random.Generator(np.random.PCG64(1000 + seed))
    p = rng.standard_normal(n) + np.where(rng.random(n) < 0.5, -0.25, 0.25)
    m = 1e-2 * rng.standard_normal(n)
    v = 1e-4 * rng.random(n)
    v[0::11] = 0.0
    out = tuple(a.astype(np.float32) for a in (p, m, v))
    for a in out:
        a.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def grad_inputs(n, launch, seed=0):
    """fp32 gradients of launch 0, 1, 2: magnitudes 10^U(-12, 3) with random signs; exact zeros at every 11th element
    (where v starts at 0) and the one after it; g within a few ulp of the starting m at elements 2 mod 13; the last
    element large."""
    rng = np.random.Generator(np.random.PCG64(2000 + 10 * seed + launch))
    g = np.sign(rng.random(n) - 0.5) * 10.0 ** rng.uniform(-12.0, 3.0, n)
    m = state_inputs(n, seed)[1].astype(np.float64)
    near = np.arange(n) % 13 == 2
    g[near] = (m * (1.0 + 3e-7 * rng.integers(-4, 5, n)))[near]
    g[0::11] = 0.0
    g[1::11] = 0.0
    g[n - 1] = 777.0        # the element every clamped load past the end reads: a sum that counted it twice shows
    g = g.astype(np.float32)
    g.setflags(write=False)
    return g


def units(got, ref, what):
    """max error of `got` against float64 `ref` in the project's tolerance units: p |d| / (2e-6 |ref| + 1e-7), the
    moments |d| / (1e-6 |ref| + 1e-6 max |ref|) (tests/test_gpu_train.py::test_fused_adam_matches_torch_adam)."""
    got = np.asarray(got, dtype=np.float64)
    ref = np.asarray(ref, dtype=np.float64)
    if ref.size == 0:
        return 0.0
    d = np.abs(got - ref)
    if what == "p":
        return float(np.max(d / (2e-6 * np.abs(ref) + 1e-7)))
    return float(np.max(d / (1e-6 * np.abs(ref) + 1e-6 * np.max(np.abs(ref)))))


@functools.lru_cache(maxsize=None)
def reference(n, wd, betas, step0, launches=3):
    """adam64 from state_inputs(n) over grad_inputs(n, 0..launches-1): [(p, m, v) after launch 1, 2, ...]."""
    p, m, v = state_inputs(n)
    out = []
    for k in range(launches):
        p, m, v = adam64(p, grad_inputs(n, k), m, v, step0 + k + 1, LR, betas[0], betas[1], EPS, wd)
        out.append((p, m, v))
    return out


@functools.lru_cache(maxsize=None)
def torch_fp32_errors(n, wd, betas, step0, launches=3):
    """The reference's error: torch.optim.Adam on fp32 CPU tensors over the same inputs, against adam64, in `units`:
    {(launches done, "p" / "m" / "v"): error} after 1 and after `launches` launches."""
    p, m, v = (torch.from_numpy(a.copy()) for a in state_inputs(n))
    p.requires_grad_()
    opt = torch.optim.Adam([p], lr=LR, betas=betas, eps=EPS, weight_decay=wd, foreach=False)
    opt.state[p] = {"step": torch.tensor(float(step0)), "exp_avg": m, "exp_avg_sq": v}
    ref = reference(n, wd, betas, step0, launches)
    out = {}
    for k in range(launches):
        p.grad = torch.from_numpy(grad_inputs(n, k).copy())
        opt.step()
        if k in (0, launches - 1):
            st = opt.state[p]
            for what, got, want in (("p", p.detach(), ref[k][0]), ("m", st["exp_avg"], ref[k][1]),
                                    ("v", st["exp_avg_sq"], ref[k][2])):
                out[(k + 1, what)] = units(got.numpy(), want, what)
    assert float(opt.state[p]["step"]) == step0 + launches
    return out


def adam_cases():
    """(list, wd, betas, step0): the full cross on the small lists, one pair per large list."""
    cases = [(name, wd, b, s) for name in SMALL for wd in WDS for b in BETAS for s in STEP0S]
    cases += [("prereduce_g1", 0.0, BETAS[0], 0), ("prereduce_g1", 0.01, BETAS[1], 5000),
              ("g2_exact", 0.01, BETAS[0], 7), ("g2_exact", 0.0, BETAS[1], 0),
              ("g2_ragged", 0.0, BETAS[0], 5000), ("g2_ragged", 0.01, BETAS[1], 7)]
    return cases
