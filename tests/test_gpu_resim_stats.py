"""bcnf_resim_error_median and bcnf_resim_impacts (bcnf_amd/csrc/bcnf_resim_stats.hip) against the numpy statements
of notebooks/resimulation.ipynb, and resimulation_summary against the same statements on resimulate_device's positions.

Tolerance: zero. Both sides are the same IEEE operations in the same order (include/bcnf_amd.h), the median is an
exact selection and the histogram integer counting, so every comparison is np.array_equal(..., equal_nan=True). All
finite values stay below 1e300 (numpy's (v + v) / 2 for an odd count below 600 rows would overflow above DBL_MAX / 2,
the one documented deviation).

Shapes: M = 1, 2, 3 (no sort, one compare, an odd column), 63 / 64 / 65 (around a wave and a power of two), 257 (more
draws than the error kernel's 256 threads), 1000 (the notebook's), 16383 (just below the limit: one 128 KB column per
workgroup, 1024 threads); S = 1 (no diff at all), 2, 7 (not a multiple of the step tile), 30 (the configs'); N = 1, 5.
"""
import os
import types
import warnings

import numpy as np
import pytest
import torch

from bcnf_amd import resimulation_stats as RS
from bcnf_amd.resimulation import resimulate_device
from bcnf_amd.utils import ParameterIndexMapping
from resim_stats_cases import BINS, make_case, notebook_error

G14 = os.path.join(os.path.dirname(__file__), "golden", "g14_resim.npz")
KEYS = ("step", "position", "transitions", "hist")


def _resim_inputs(d):
    """names and data_dict of the g14 fixture, as tests/test_resim.py builds them."""
    from bcnf_amd.resimulation import PHYSICS_PARAMETERS
    names = [str(s) for s in d["names"]]
    fixed = d["fixed_phys"]
    n = fixed.shape[0]
    data_dict = {q: list(fixed[:, c]) for c, q in enumerate(PHYSICS_PARAMETERS)}
    data_dict.update(g=list(d["g_extra"]), A=list(d["A_extra"]), Cd=[0.2] * n,
                     trajectories=[np.zeros((30, 3)) for _ in range(n)])
    return names, data_dict


def _same(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and np.array_equal(a, b, equal_nan=True)


def _np(d):
    return {k: None if d[k] is None else d[k].cpu().numpy() for k in KEYS}


@pytest.mark.gpu
@pytest.mark.parametrize("s", [1, 2, 7, 30])
@pytest.mark.parametrize("m", [1, 2, 3, 63, 64, 65, 257, 1000, RS.MAX_DRAWS - 1])
def test_kernels_equal_numpy(m, s):
    for n in (1, 5):
        x, obs32 = make_case(n, m, s, seed=1000 * m + 10 * s + n, obs_dtype=np.float32)
        xd = torch.from_numpy(x).cuda()
        for obs in (obs32, obs32.astype(np.float64) * 1.0000001):          # float32 and float64 observations
            want = notebook_error(x, obs)
            got = RS.resimulation_error_device(xd, torch.from_numpy(obs).cuda()).cpu().numpy()
            bad = np.argwhere(~((got == want) | (np.isnan(got) & np.isnan(want))))
            print(f"n={n} m={m} s={s} {obs.dtype}: {len(bad)} of {want.size} differ")
            assert _same(got, want), (n, m, s, obs.dtype, bad[:4])
            assert _same(RS.resimulation_error_host(x, obs), want)
        want = RS.impacts_host(x, BINS)
        got = _np(RS.impacts_device(xd, BINS))
        for k in KEYS:
            assert _same(got[k], want[k]), (n, m, s, k)
        nohist = RS.impacts_device(xd)
        assert nohist["hist"] is None
        for k in KEYS[:3]:
            assert _same(nohist[k].cpu().numpy(), want[k]), (n, m, s, k)


@pytest.mark.gpu
def test_special_columns_and_impact_cases_are_present():
    """The inputs of test_kernels_equal_numpy hold what they are meant to: an all-NaN column, NaN counts leaving odd and
    even remainders, ties, +inf and zeros among the error columns; no transition, one at s = 0, one at S - 2, two in
    one draw, a NaN from some step on and a start below ground among the draws -- and the kernels get each right."""
    n, m, s = 5, 65, 7
    x, obs = make_case(n, m, s, seed=4242)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore", RuntimeWarning)                           # "Mean of empty slice"
        v = np.nanmean((x - obs.astype(np.float64)[:, None])**2, axis=3)         # (n, m, s) per-draw values
    counts = (~np.isnan(v)).sum(axis=1)
    assert (counts == 0).any() and (counts[counts > 0] % 2 == 0).any() and (counts % 2 == 1).any()
    assert np.isinf(v).any() and (v == 0).any()
    assert any(len(np.unique(v[i, :, t][~np.isnan(v[i, :, t])])) < counts[i, t] for i in range(n) for t in range(s))
    xd = torch.from_numpy(x).cuda()
    err = RS.resimulation_error_device(xd, torch.from_numpy(obs).cuda()).cpu().numpy()
    assert _same(err, notebook_error(x, obs))
    assert np.isnan(err).any() and np.isinf(err).any()
    got = _np(RS.impacts_device(xd, BINS))
    step, tr = got["step"][2], got["transitions"][2]              # trajectory 2: no error column was planted in it
    kind = (np.arange(m) + 2) % 7
    assert (step[kind == 0] == -1).all() and (tr[kind == 0] == 0).all()
    assert (step[kind == 1] == 0).all() and (step[kind == 2] == s - 2).all()
    assert (step[kind == 3] == 0).all() and (tr[kind == 3] == 2).all()
    assert (step[kind == 4] == (s + 1) // 2 - 1).all() and (step[kind == 5] == 2).all()
    assert np.isnan(got["position"][2][kind == 0]).all() and not np.isnan(got["position"][2][kind == 2]).any()
    assert 0 < got["hist"].sum() < got["transitions"].sum()       # some binned, some dropped outside the edges
    want = RS.impacts_host(x, BINS)
    for k in KEYS:
        assert _same(got[k], want[k]), k


@pytest.mark.gpu
def test_long_trajectories_and_edge_tables():
    """S above one wave's 64 steps (the chunk loop, a transition across the chunk boundary) and edge tables of 2 edges
    (one bin) and of the limit."""
    x, _ = make_case(2, 9, 130, seed=7)
    x[1, 3, :, 2] = 1.0
    x[1, 3, 64:, 2] = -1.0                                         # above at s = 63, below at s = 64
    x[1, 4, :, 2] = np.where(np.arange(130) % 2 == 0, 1.0, -2.0)   # 65 transitions
    xd = torch.from_numpy(x).cuda()
    for edges in (np.array([-30.0, 30.0]), np.linspace(-50, 50, RS.MAX_EDGES), BINS):
        want = RS.impacts_host(x, edges)
        got = _np(RS.impacts_device(xd, edges))
        for k in KEYS:
            assert _same(got[k], want[k]), (len(edges), k)
    assert want["step"][1, 3] == 63 and want["transitions"][1, 4] == 65
    # views and empty inputs
    part = RS.impacts_device(xd[:, 2:7])
    assert _same(part["step"].cpu().numpy(), want["step"][:, 2:7])
    empty = RS.impacts_device(xd[:, :0], BINS)
    assert empty["step"].shape == (2, 0) and empty["hist"].shape == (2, 127, 127) and not empty["hist"].any()
    e0 = RS.resimulation_error_device(xd[:, :0], torch.zeros(2, 130, 3).cuda())
    assert e0.shape == (2, 130) and bool(torch.isnan(e0).all())


@pytest.mark.gpu
def test_limits_raise_and_launch_nothing():
    x = torch.zeros(1, RS.MAX_DRAWS + 1, 1, 3, dtype=torch.float64).cuda()
    with pytest.raises(ValueError, match=f"at most {RS.MAX_DRAWS} draws"):
        RS.resimulation_error_device(x, torch.zeros(1, 1, 3).cuda())
    with pytest.raises(ValueError, match=f"at most {RS.MAX_EDGES} edges"):
        RS.impacts_device(x, bins=np.arange(RS.MAX_EDGES + 1.0))
    from bcnf_amd import _native as N
    err = torch.full((1, 1), 7.0, dtype=torch.float64).cuda()
    st = N.stream_handle(x.device)
    assert N.call_raw("bcnf_resim_error_median", x, torch.zeros(1, 1, 3).cuda(), 0, 1, RS.MAX_DRAWS + 1, 1, err,
                      st) == N.ERR_UNSUPPORTED
    torch.cuda.synchronize()
    assert float(err[0, 0]) == 7.0                                  # untouched


@pytest.mark.gpu
def test_summary_does_not_depend_on_the_slicing():
    d = np.load(G14)
    names, data_dict = _resim_inputs(d)
    pim = ParameterIndexMapping(names)
    model = types.SimpleNamespace(parameter_index_mapping=pim, device="cuda:0")
    observed = d["resim"][:, 0]
    res = [RS.resimulation_summary(model, 2, 1 / 15, data_dict, d["y_hat"], observed=observed, break_on_impact=True,
                                   chunk_trajectories=c, verbose=False) for c in (1, 2, None)]
    for other in res[1:]:
        assert other.keys() == res[0].keys()
        for k in res[0]:
            assert _same(other[k], res[0][k]), k
    x = resimulate_device(d["y_hat"], 2, 1 / 15, data_dict, pim, break_on_impact=True).cpu().numpy()
    assert x.shape == (5, 6, 30, 3)
    got = res[0]
    assert _same(got["errors"], RS.resimulation_error_host(x, observed))
    want = RS.impacts_host(x, BINS)
    for k in KEYS:
        assert _same(got["impact_" + k], want[k]), k
    assert got["impact_transitions"].sum() > 0 and (got["impact_step"] >= 0).any()
    ow = RS.impacts_host(observed[:, None])
    assert _same(got["observed_impact_step"], ow["step"][:, 0])
    assert _same(got["observed_impact_position"], ow["position"][:, 0])
    assert got["status_counts"].tolist() == [30, 0, 0]
    nob = RS.resimulation_summary(model, 2, 1 / 15, data_dict, torch.from_numpy(d["y_hat"]).cuda(),
                                  observed=torch.from_numpy(observed).float(), break_on_impact=True, bins=None,
                                  verbose=False)
    assert nob["impact_hist"] is None and _same(nob["impact_step"], got["impact_step"])
    assert _same(nob["errors"], RS.resimulation_error_host(x, observed.astype(np.float32)))
