"""Resimulation error and impact statistics (notebooks/resimulation.ipynb), the parts that need no GPU.

The host statements (`resimulation_error_host`, `impacts_host`) against the notebook's literal numpy expressions on
the g14 fixture and on crafted columns; the definition the kernels implement (tests/resim_stats_cases.py restates
include/bcnf_amd.h in scalar Python) against the same numpy statements, bit for bit; the histogram rule against
np.histogram2d at the edges; argument and limit errors; the calibration residuals; exports.
"""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

import bcnf_amd
from bcnf_amd import _native as N
from bcnf_amd import resimulation_stats as RS
from bcnf_amd.calibration import CDF, brownian_confidence_interval, compute_CDF_residuals
from conftest import ROOT
from resim_stats_cases import (BINS, kernel_bin, kernel_error, kernel_impacts, make_case, notebook_error,
                               notebook_impacts)

G14 = os.path.join(os.path.dirname(__file__), "golden", "g14_resim.npz")


def _same(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and np.array_equal(a, b, equal_nan=True)


def _check_impacts_against_notebook(x, got):
    """step / position / transitions / hist of `got` are the notebook's (draw, step) lists, re-expressed."""
    for i in range(x.shape[0]):
        draw, s = notebook_impacts(x, i)
        assert np.array_equal(got["indices"][i][0], draw) and np.array_equal(got["indices"][i][1], s)
        assert np.array_equal(np.bincount(draw, minlength=x.shape[1]), got["transitions"][i])
        for j in range(x.shape[1]):
            mine = s[draw == j]
            assert got["step"][i, j] == (mine[0] if mine.size else -1)
            want = x[i, j, mine[0]] if mine.size else np.full(3, np.nan)
            assert np.array_equal(got["position"][i, j], want, equal_nan=True)
        if got["hist"] is not None:
            pos = x[i, draw, s]
            assert np.array_equal(got["hist"][i], np.histogram2d(pos[:, 0], pos[:, 1], bins=BINS)[0])


def test_host_statements_on_the_reference_fixture():
    x = np.load(G14)["resim"]
    assert x.shape == (5, 6, 30, 3)
    observed = x[:, 0]
    err = RS.resimulation_error_host(x, observed)
    assert _same(err, np.nanmedian(np.nanmean((x - observed[:, None])**2, axis=3), axis=1))
    assert err.shape == (5, 30) and (err[:, 0] >= 0).all()
    got = RS.impacts_host(x, BINS)
    assert [len(notebook_impacts(x, i)[0]) for i in range(5)] == [0, 6, 0, 5, 6]
    assert got["transitions"].sum(axis=1).tolist() == [0, 6, 0, 5, 6]
    _check_impacts_against_notebook(x, got)
    assert got["hist"].dtype == np.int32 and got["hist"].sum(axis=(1, 2)).tolist() == [0, 6, 0, 5, 6]
    assert RS.impacts_host(x)["hist"] is None
    # the kernels' definition gives the same on the fixture
    assert _same(kernel_error(x, observed), err)
    mine = kernel_impacts(x, BINS)
    for k in ("step", "position", "transitions", "hist"):
        assert _same(mine[k], got[k]), k


@pytest.mark.parametrize("m", [1, 2, 3, 8, 13])
@pytest.mark.parametrize("obs_dtype", [np.float32, np.float64])
def test_crafted_columns(m, obs_dtype):
    """Odd and even non-NaN counts, an all-NaN column, +inf, duplicates, zeros, a NaN in one component only and a NaN
    in the observation: numpy's statement, the host function and the kernels' definition agree to the bit."""
    x, obs = make_case(2, m, 7, seed=100 + m, obs_dtype=obs_dtype)
    want = notebook_error(x, obs)
    assert _same(RS.resimulation_error_host(x, obs), want)
    assert _same(kernel_error(x, obs), want)
    assert np.isnan(want[0, 1]) and np.isnan(want[1, 4])            # all-NaN columns (positions; observation)
    assert not np.isnan(want[0, 3])                                 # one NaN component of the observation: count 2
    if m >= 3:
        assert np.isinf(want[0, 2])                                 # more than half of the column is +inf
    got = RS.impacts_host(x, BINS)
    _check_impacts_against_notebook(x, got)
    mine = kernel_impacts(x, BINS)
    for k in ("step", "position", "transitions", "hist"):
        assert _same(mine[k], got[k]), k


def test_error_columns_by_hand():
    """Columns small enough to state the answer: the mean skips NaN components, the median skips NaN draws."""
    obs = np.zeros((1, 4, 3))
    x = np.zeros((1, 4, 4, 3))
    x[0, :, 0] = [[1, 2, 2], [np.nan, 3, 3], [0, 0, 0], [np.nan, np.nan, np.nan]]      # values 3, 9, 0 -> 3
    x[0, :, 1] = [[1, 1, 1], [2, 2, 2], [3, 3, 3], [4, 4, 4]]                          # 1, 4, 9, 16 -> 6.5
    x[0, :, 2] = np.nan
    x[0, :, 3] = [[np.inf, 0, 0], [1, 1, 1], [1, 1, 1], [np.inf, 1, 1]]                # inf, 1, 1, inf -> inf
    want = np.array([[3.0, 6.5, np.nan, np.inf]])
    for f in (RS.resimulation_error_host, kernel_error, notebook_error):
        assert np.array_equal(f(x, obs), want, equal_nan=True), f.__name__


def test_impact_patterns_by_hand():
    z = np.array([[1, 1, 1, 1, 1],            # no transition
                  [1, -1, -1, -1, -1],        # at s = 0
                  [1, 1, 1, 1, -1],           # at s = S - 2
                  [1, -1, 1, -1, -1],         # two
                  [1, 1, np.nan, np.nan, np.nan],   # NaN from s = 2 on
                  [-1, 1, 1, 0, -1]], float)  # starts below; falls onto exactly 0
    x = np.zeros((1, 6, 5, 3))
    x[0, :, :, 2] = z
    x[0, :, :, 0] = np.arange(5)
    for got in (RS.impacts_host(x), kernel_impacts(x)):
        assert got["step"].tolist() == [[-1, 0, 3, 0, 1, 2]]
        assert got["transitions"].tolist() == [[0, 1, 1, 2, 1, 1]]
        assert np.array_equal(got["position"][0, :, 0], [np.nan, 0, 3, 0, 1, 2], equal_nan=True)
    one = RS.impacts_host(x[:, :, :1], BINS)                       # S = 1: no diff at all
    assert (one["step"] == -1).all() and not one["hist"].any() and not one["transitions"].any()


def test_histogram_rule_at_the_edges():
    """Values on an inner edge, on the first and the last edge, just outside, NaN and inf: the kernels' bin rule is
    np.histogram2d's."""
    edges = np.array([-2.0, -0.5, 0.25, 1.0, 4.0])
    vals = [-2.0, 4.0, -0.5, 0.25, 1.0, np.nextafter(4.0, np.inf), np.nextafter(-2.0, -np.inf), np.nextafter(4.0, 0),
            np.nan, np.inf, -np.inf, 0.0, 3.9]
    assert [kernel_bin(edges, v) for v in vals] == [0, 3, 1, 2, 3, -1, -1, 3, -1, -1, -1, 1, 3]
    pairs = [(a, b) for a in vals for b in vals]
    x = np.zeros((1, len(pairs), 2, 3))
    x[0, :, 0, 2], x[0, :, 1, 2] = 1.0, -1.0                        # every draw: one transition at s = 0
    x[0, :, 0, 0] = [p[0] for p in pairs]
    x[0, :, 0, 1] = [p[1] for p in pairs]
    want = np.histogram2d(x[0, :, 0, 0], x[0, :, 0, 1], bins=edges)[0]
    assert want.sum() == 8 * 8                                      # 5 of the 13 values are dropped on each axis
    for got in (RS.impacts_host(x, edges), kernel_impacts(x, edges)):
        assert np.array_equal(got["hist"][0], want) and got["hist"].dtype == np.int32
    assert want[0, 3] == 1 * 4 and want[3, 3] == 4 * 4               # x bin first; the last edge in the last bin


def test_argument_errors():
    x = torch.zeros(2, 3, 4, 3, dtype=torch.float64)
    obs = torch.zeros(2, 4, 3)
    with pytest.raises(RuntimeError, match="HIP device only"):
        RS.resimulation_error_device(x, obs)
    with pytest.raises(RuntimeError, match="HIP device only"):
        RS.impacts_device(x)
    for bad in (torch.zeros(2, 5, 3), torch.zeros(3, 4, 3), torch.zeros(2, 4, 2), torch.zeros(2, 4)):
        with pytest.raises(ValueError, match="observed"):
            RS.resimulation_error_device(x, bad)
        with pytest.raises(ValueError, match="observed"):
            RS.resimulation_error_host(x.numpy(), bad.numpy())
    with pytest.raises(ValueError, match=r"\(N, M, S, 3\)"):
        RS.resimulation_error_device(torch.zeros(2, 3, 4, dtype=torch.float64), obs)
    with pytest.raises(ValueError, match=r"\(N, M, S, 3\)"):
        RS.impacts_device(torch.zeros(2, 3, 4, 2, dtype=torch.float64))
    with pytest.raises(ValueError, match="float64"):
        RS.impacts_device(x.float())
    with pytest.raises(ValueError, match="increase strictly"):
        RS.impacts_device(x, bins=[0.0, 1.0, 1.0])
    with pytest.raises(ValueError, match="at least 2 edges"):
        RS.impacts_host(x.numpy(), bins=[0.0])


def test_summary_argument_errors():
    import types
    from bcnf_amd.utils import ParameterIndexMapping
    names = ["x0_x", "x0_y", "x0_z"]
    stack = types.SimpleNamespace(n_distinct_conditions=1)
    model = types.SimpleNamespace(parameter_index_mapping=ParameterIndexMapping(names), device="cpu",
                                  feature_network_stack=stack)
    obs = np.zeros((4, 30, 3))
    with pytest.raises(ValueError, match="Expected 1 conditions, got 0"):
        RS.resimulation_summary(model, 2, 1 / 15, {}, observed=obs, verbose=False)
    with pytest.raises(ValueError, match=r"y_hat must be \(M, N, D\)"):
        RS.resimulation_summary(model, 2, 1 / 15, {}, np.zeros((4, 3)), observed=obs, verbose=False)
    y = np.zeros((6, 4, 3), dtype=np.float32)
    for bad in (np.zeros((4, 29, 3)), np.zeros((5, 30, 3)), np.zeros((4, 30))):
        with pytest.raises(ValueError, match="observed"):
            RS.resimulation_summary(model, 2, 1 / 15, {}, y, observed=bad, verbose=False)
    with pytest.raises(ValueError, match="chunk_trajectories"):
        RS.resimulation_summary(model, 2, 1 / 15, {}, y, observed=obs, chunk_trajectories=0, verbose=False)
    with pytest.raises(ValueError, match=f"at most {RS.MAX_EDGES} edges"):
        RS.resimulation_summary(model, 2, 1 / 15, {}, y, observed=obs, bins=np.arange(RS.MAX_EDGES + 1.0),
                                verbose=False)
    big = np.zeros((RS.MAX_DRAWS + 1, 1, 3), dtype=np.float32)
    with pytest.raises(ValueError, match=f"at most {RS.MAX_DRAWS} draws"):
        RS.resimulation_summary(model, 2, 1 / 15, {}, big, observed=obs[:1], verbose=False)
    assert RS.default_chunk_trajectories(1000, 30) == RS.SLICE_BYTES // (1000 * 30 * 24) == 372
    assert RS.default_chunk_trajectories(RS.MAX_DRAWS, 10 ** 6) == 1


def test_limits_are_refused_before_any_launch():
    """Above the documented limits the Python layer raises a ValueError that names the limit, and the C entry points
    return BCNF_ERR_UNSUPPORTED without touching a pointer (NULL everywhere: nothing can have been launched)."""
    assert (RS.MAX_DRAWS, RS.MAX_EDGES) == (16384, 192) and RS.MAX_DRAWS >= 10_000 and RS.MAX_EDGES >= 128
    src = open(os.path.join(ROOT, "include", "bcnf_amd.h")).read()
    assert f"#define BCNF_RESIM_ERROR_MAX_DRAWS {RS.MAX_DRAWS}\n" in src
    assert f"#define BCNF_RESIM_HIST_MAX_EDGES {RS.MAX_EDGES}\n" in src
    x = torch.zeros(1, RS.MAX_DRAWS + 1, 1, 3, dtype=torch.float64)
    with pytest.raises(ValueError, match="at most 16384 draws"):
        RS.resimulation_error_device(x, torch.zeros(1, 1, 3))
    with pytest.raises(ValueError, match="at most 192 edges"):
        RS.impacts_device(x[:, :2], bins=np.arange(193.0))
    null = ctypes.c_void_p(0)
    assert N.call_raw("bcnf_resim_error_median", None, None, 0, 1, RS.MAX_DRAWS + 1, 1, None, null) == N.ERR_UNSUPPORTED
    assert N.call_raw("bcnf_resim_impacts", None, 1, 1, 1, ctypes.c_void_p(8), RS.MAX_EDGES + 1, None, None, None,
                      ctypes.c_void_p(8), null) == N.ERR_UNSUPPORTED
    # argument errors and the N M == 0 no-op, also before any device call
    assert N.call_raw("bcnf_resim_error_median", None, None, 0, 1, 4, 0, None, null) == N.ERR_ARG          # steps < 1
    assert N.call_raw("bcnf_resim_error_median", None, None, 0, 1, 4, 2, None, null) == N.ERR_ARG          # NULL pointers
    assert N.call_raw("bcnf_resim_error_median", None, None, 0, 0, 4, 2, None, null) == N.OK
    assert N.call_raw("bcnf_resim_error_median", None, None, 0, 3, 0, 2, None, null) == N.OK
    assert N.call_raw("bcnf_resim_impacts", None, 0, 5, 2, None, 0, None, None, None, None, null) == N.OK
    assert N.call_raw("bcnf_resim_impacts", None, 1, 1, 2, None, 0, None, None, None, None, null) == N.ERR_ARG
    assert N.call_raw("bcnf_resim_impacts", None, 1, 1, 2, ctypes.c_void_p(8), 5, None, None, None, None,
                      null) == N.ERR_ARG                                                            # edges without hist
    assert N.call_raw("bcnf_resim_impacts", None, 1, 1, 2, ctypes.c_void_p(8), 1, None, None, None,
                      ctypes.c_void_p(8), null) == N.ERR_ARG                                        # one edge


def test_cdf_residuals_formula():
    rng = np.random.Generator(np.random.PCG64(5))
    M, n, d = 200, 37, 4
    ranks = rng.integers(0, M + 1, size=(n, d))
    t, res, ci = compute_CDF_residuals(torch.from_numpy(ranks), M, t_divisions=21, sigma=2.0)
    assert t.shape == (21,) and res.shape == (d, 21) and ci.shape == (21,)
    assert np.array_equal(t, np.linspace(0, 1, 21))
    for k in range(d):
        for q, tq in enumerate(t):
            cdf = np.count_nonzero(ranks[:, k] <= tq * M) / n
            assert res[k, q] == (cdf - tq) * np.sqrt(n) / 2.0
    assert np.array_equal(ci, np.sqrt(t * (1 - t))) and np.array_equal(ci, brownian_confidence_interval(t))
    cdf = CDF(ranks, t, M)
    assert cdf.shape == (d, 21) and cdf[2, 7] == np.count_nonzero(ranks[:, 2] <= t[7] * M) / n
    assert (CDF(ranks, np.array([1.0]), M) == 1.0).all()
    t2, res2, _ = compute_CDF_residuals(ranks, M)                   # numpy ranks; the defaults
    assert t2.shape == (100,) and res2.shape == (d, 100)


def test_exports():
    names = {"resimulation_error_device", "resimulation_error_host", "impacts_device", "impacts_host",
             "resimulation_summary"}
    assert names <= set(bcnf_amd.__all__)
    for n in names:
        assert getattr(bcnf_amd, n) is getattr(RS, n)
    from bcnf_amd import calibration
    assert {"CDF", "brownian_confidence_interval", "compute_CDF_residuals", "compute_y_hat_ranks"} <= set(
        calibration.__all__)


def test_header_and_exports_agree():
    src = open(os.path.join(ROOT, "include", "bcnf_amd.h")).read()
    declared = set(re.findall(r"^(?:int|int64_t|const char\*)\s+(bcnf_\w+)\s*\(", src, flags=re.M))
    assert declared == set(N.EXPORTS) and len(N.EXPORTS) == len(set(N.EXPORTS))
    assert {"bcnf_resim_error_median", "bcnf_resim_impacts"} <= declared
    lib = N.lib()
    assert hasattr(lib, "bcnf_resim_error_median") and hasattr(lib, "bcnf_resim_impacts")
    assert "#define BCNF_AMD_ABI_VERSION 3\n" in src and N.ABI_VERSION == 3 == lib.bcnf_abi_version()
