"""tests/optim_ref.py is the float64 reference of tests/test_gpu_optim.py: here it is pinned to torch's own float64
Adam and clip, and the error of torch's fp32 CPU Adam against it -- "the reference's error" that bounds the kernels
there -- is measured on the very inputs of the GPU cases. No GPU."""
import math

import numpy as np
import pytest
import torch

import optim_ref as R


def rel(a, b):
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    return float(np.max(np.abs(a - b) / np.maximum(np.abs(b), 1e-300))) if b.size else 0.0


@pytest.mark.parametrize("step0", R.STEP0S)
@pytest.mark.parametrize("betas", R.BETAS)
@pytest.mark.parametrize("wd", R.WDS)
def test_adam64_equals_torch_float64_adam(wd, betas, step0):
    """Three steps of adam64 == torch.optim.Adam on float64 CPU tensors within 1e-14 relative (p, exp_avg,
    exp_avg_sq), on the `seams` inputs: zeros in g and v, g next to m, thirteen decades of |g|. exp_avg_sq is a sum
    of non-negative terms: relative to the element. exp_avg = m + (1 - b1)(g - m) and p = p - update cancel at some
    elements (g near -m b1 / (1 - b1): seen, 2.8e-14 of such an element), where two correctly rounded float64
    evaluations differ by 1e-16 of the terms, not of the result: relative to the larger of the element and the terms
    it was summed from in any of the three steps."""
    n = sum(R.LISTS["seams"])
    p0, m0, v0 = (a.astype(np.float64) for a in R.state_inputs(n))
    tp = torch.from_numpy(p0.copy()).requires_grad_()
    opt = torch.optim.Adam([tp], lr=R.LR, betas=betas, eps=R.EPS, weight_decay=wd, foreach=False)
    opt.state[tp] = {"step": torch.tensor(float(step0)), "exp_avg": torch.from_numpy(m0.copy()),
                     "exp_avg_sq": torch.from_numpy(v0.copy())}
    p, m, v = p0, m0, v0
    terms_p, terms_m = np.abs(p0), np.abs(m0)
    for k in range(3):
        g = R.grad_inputs(n, k).astype(np.float64)
        tp.grad = torch.from_numpy(g.copy())
        opt.step()
        terms_m = np.maximum(terms_m, np.abs(g + wd * p))
        p_new, m, v = R.adam64(p, g, m, v, step0 + k + 1, R.LR, betas[0], betas[1], R.EPS, wd)
        terms_p = np.maximum(terms_p, np.abs(p_new - p))
        p = p_new
    st = opt.state[tp]
    assert tp.dtype == torch.float64 and float(st["step"]) == step0 + 3
    for got, ref, terms in ((p, tp.detach().numpy(), terms_p), (m, st["exp_avg"].numpy(), terms_m)):
        assert np.all(np.abs(got - ref) <= 1e-14 * np.maximum(np.abs(ref), terms))
    assert rel(v, st["exp_avg_sq"].numpy()) <= 1e-14


@pytest.mark.parametrize("max_norm", [1.0, 1e30])
def test_clip64_equals_torch_float64_clip(max_norm):
    sizes = R.LISTS["seams"]
    flat = R.grad_inputs(sum(sizes), 0).astype(np.float64)
    cuts = np.cumsum([0] + sizes)
    grads = [flat[a:b] for a, b in zip(cuts[:-1], cuts[1:])]
    params = [torch.zeros(len(g), dtype=torch.float64, requires_grad=True) for g in grads]
    for q, g in zip(params, grads):
        q.grad = torch.from_numpy(g.copy())
    n_ref = float(torch.nn.utils.clip_grad_norm_(params, max_norm))
    norm, coef, clipped = R.clip64(grads, max_norm)
    assert abs(norm - n_ref) <= 1e-14 * n_ref
    assert abs(norm * norm - R.sumsq64(grads)) <= 1e-14 * norm * norm
    assert coef == 1.0 if max_norm == 1e30 else coef < 1e-3
    for q, c in zip(params, clipped):
        assert rel(c, q.grad.numpy()) <= 1e-14


def test_inputs_hold_the_cases_the_kernels_are_tested_on():
    n = sum(R.LISTS["seams"])
    p, m, v = R.state_inputs(n)
    g = R.grad_inputs(n, 0)
    assert p.dtype == m.dtype == v.dtype == g.dtype == np.float32
    assert np.all(p != 0) and np.all(v >= 0)
    assert np.any((g == 0) & (v == 0)) and np.any((g == 0) & (v > 0))
    near = (np.arange(n) % 13 == 2) & (g != 0) & (np.arange(n) < n - 1)
    assert g[n - 1] == 777.0
    assert np.any(near) and np.all(np.abs(g[near] - m[near]) <= 2e-6 * np.abs(m[near]))
    mag = np.abs(g[g != 0])
    assert mag.min() < 1e-11 and mag.max() > 1e2
    for name, sizes in R.LISTS.items():
        assert len(sizes) <= R.MAX_TENSORS, name
    assert sum(R.LISTS["prereduce_g1"]) == 2050 * 1024 + 5 and sum(R.LISTS["g2_exact"]) == 1 << 22
    assert sum(R.LISTS["g2_ragged"]) == (1 << 22) + 2048 + 3
    assert all(s % 2 == 1 for s in R.LISTS["g2_ragged"][:2])


@pytest.mark.parametrize("name,wd,betas,step0", R.adam_cases())
def test_torch_fp32_adam_error_against_adam64(name, wd, betas, step0):
    """The reference's error, printed (pytest -s): torch's fp32 CPU Adam against adam64 after 1 and 3 launches on the
    inputs of the GPU case, in the project's tolerance units. The GPU test bounds the kernel by max(1, 2 x this), so
    it must be a number."""
    n = sum(R.LISTS[name])
    errs = R.torch_fp32_errors(n, wd, betas, step0)
    print(f"{name} wd={wd} betas={betas} step0={step0}: " +
          " ".join(f"{k}x{what}={e:.3f}" for (k, what), e in sorted(errs.items())))
    assert set(errs) == {(k, w) for k in (1, 3) for w in "pmv"}
    assert all(math.isfinite(e) and e >= 0 for e in errs.values())
