"""CPU checks of bcnf_amd.generate: the numpy statement of the draw rule (sample_candidates_host) against the values the
reference's own sample_ballistic_parameters computed from the same draws (tests/golden/g20_generate.npz, made by
tests/golden/make_golden_generate.py), the priors' distributions, the config's error paths and the assembly of the
returned dict. Nothing here launches a kernel.

Kolmogorov-Smirnov: each prior of tests/golden/data_config.yaml, 20 000 candidates of seed 2024_03_25, one-sample test
against the scipy distribution it should follow; the statistic must stay below 1.95 / sqrt(n), the alpha = 0.001 critical
value. With about 25 tests a correct sampler fails one of them with probability about 2.5 %; seed 2024_03_25 passes them
all, so no other seed is used.
"""
import os

import numpy as np
import pytest
import scipy.stats as st

from conftest import GOLDEN, load_golden

from bcnf_amd import generate as G
from bcnf_amd.utils import ParameterIndexMapping

CONFIG = os.path.join(GOLDEN, "data_config.yaml")
SEED = 2024_03_25
N_KS = 20_000
TWO_PI = 2 * np.pi


@pytest.fixture(scope="module")
def g20():
    return load_golden("g20_generate.npz")


@pytest.fixture(scope="module")
def host():
    return G.sample_candidates_host(CONFIG, SEED, 0, N_KS)


def test_host_rule_reproduces_the_reference_bit_for_bit(g20):
    rows = g20["rows"]
    h = G.sample_candidates_host(CONFIG, int(g20["seed"]), 0, rows.shape[0])
    assert list(h.keys()) == list(G.KEYS) + ["u_distance", "u_visibility"]
    for key in G.KEYS:
        want = rows[:, G.COLUMNS[key]]
        if key == "cam_radian_array":
            assert (want[:, 0] == 0.0).all()          # cam1_radian, prepended by generate_data
            want = want[:, 1:]
        got = np.asarray(h[key], dtype=np.float64)
        assert got.shape == want.shape, key
        assert np.array_equal(got.view(np.uint64), np.ascontiguousarray(want).view(np.uint64)), key
    assert np.array_equal(h["u_distance"], rows[:, G.COL_U_DISTANCE])
    assert np.array_equal(h["u_visibility"], rows[:, G.COL_U_VISIBILITY])


def test_candidates_do_not_depend_on_the_range_asked_for(host):
    part = G.sample_candidates_host(CONFIG, SEED, 1000, 37)
    for key, value in part.items():
        assert np.array_equal(value, host[key][1000:1037]), key
    other = G.sample_candidates_host(CONFIG, SEED + 1, 0, 37)
    assert not np.array_equal(other["x0_x"], host["x0_x"][:37])
    far = G.sample_candidates_host(CONFIG, SEED, 2**32 + 5, 3)          # the candidate's high half is part of the counter
    near = G.sample_candidates_host(CONFIG, SEED, 5, 3)
    assert not np.array_equal(far["m"], near["m"]) and np.isfinite(far["m"]).all()


def _polar(x, y, std):
    """(|n|, angle) of a polar pair drawn as r = sqrt(|n|) std: |n| is half-normal, the angle uniform on [0, 2 pi)."""
    return (np.hypot(x, y) / std) ** 2, np.mod(np.arctan2(y, x), TWO_PI)


KS_CASES = {
    "x0_xy radius": lambda h: (_polar(h["x0_x"], h["x0_y"], 20)[0], st.halfnorm()),
    "x0_xy angle": lambda h: (_polar(h["x0_x"], h["x0_y"], 20)[1], st.uniform(0, TWO_PI)),
    "x0_z": lambda h: (h["x0_z"], st.uniform(0.1, 2.4)),
    "v0_xy radius": lambda h: (_polar(h["v0_x"], h["v0_y"], 15)[0], st.halfnorm()),
    "v0_xy angle": lambda h: (_polar(h["v0_x"], h["v0_y"], 15)[1], st.uniform(0, TWO_PI)),
    "v0_z": lambda h: (h["v0_z"], st.norm(7, 5)),
    "w_xy radius": lambda h: (_polar(h["w_x"], h["w_y"], 3)[0], st.halfnorm()),
    "w_xy angle": lambda h: (_polar(h["w_x"], h["w_y"], 3)[1], st.uniform(0, TWO_PI)),
    "w_z": lambda h: (h["w_z"], st.norm(0, 1)),
    "g": lambda h: (-h["g_z"], st.gamma(9.81, scale=1)),
    "rho": lambda h: (h["rho"], st.gamma(3.5, scale=0.35)),
    "r_ball": lambda h: (h["r"], st.gamma(1.75, scale=0.05)),
    "Cd": lambda h: (h["Cd"], st.gamma(2, scale=0.35)),
    "m": lambda h: (h["m"], st.gamma(2, scale=0.15)),
    "cam_radian": lambda h: (h["cam_radian_array"][:, 0], st.uniform(0, 6.283185307)),
    "cam_radius": lambda h: (h["cam_radius"], st.gamma(2.5, scale=5)),
    "cam_angle 0": lambda h: (h["cam_angles"][:, 0], st.gamma(3, scale=10)),
    "cam_angle 1": lambda h: (h["cam_angles"][:, 1], st.gamma(3, scale=10)),
    "cam_heights 0": lambda h: (h["cam_heights"][:, 0], st.uniform(0.4, 1.0)),
    "cam_heights 1": lambda h: (h["cam_heights"][:, 1], st.uniform(0.4, 1.0)),
    "u_distance": lambda h: (h["u_distance"], st.uniform(0, 1)),
    "u_visibility": lambda h: (h["u_visibility"], st.uniform(0, 1)),
}


@pytest.mark.parametrize("name", list(KS_CASES))
def test_priors_pass_kolmogorov_smirnov(host, name):
    sample, dist = KS_CASES[name](host)
    res = st.kstest(sample, dist.cdf)
    print(f"{name}: D = {res.statistic:.5f}, p = {res.pvalue:.4f}")
    assert res.statistic < 1.95 / np.sqrt(N_KS), (name, res.statistic, res.pvalue)


def test_derived_parameters_and_the_degenerate_thrust(host):
    """a has std 0 in the config, so the thrust is exactly zero; g_z = -g, A = pi r^2, b = rho A Cd."""
    for key in ("a_x", "a_y", "a_z", "g_x", "g_y"):
        assert (host[key] == 0.0).all(), key
    assert (host["g_z"] < 0).all()
    assert np.allclose(host["A"], np.pi * host["r"] ** 2, rtol=1e-15, atol=0)
    assert np.array_equal(host["b"], host["rho"] * host["A"] * host["Cd"])
    # slots are independent: no pair of the raw draws is visibly correlated (|r| < 4 / sqrt(n))
    cols = np.stack([host["x0_z"], host["v0_z"], host["w_z"], host["g_z"], host["rho"], host["r"], host["Cd"], host["m"],
                     host["cam_radius"], host["u_distance"], host["u_visibility"]])
    corr = np.corrcoef(cols) - np.eye(len(cols))
    assert np.abs(corr).max() < 4 / np.sqrt(N_KS)


def _config(**changes):
    cfg = G.load_data_config(CONFIG)
    cfg = {k: ({kk: dict(vv) if isinstance(vv, dict) else vv for kk, vv in v.items()}) for k, v in cfg.items()}
    for path, value in changes.items():
        node = cfg
        keys = path.split("__")
        for k in keys[:-1]:
            node = node[k]
        node[keys[-1]] = value
    return cfg


def test_other_distribution_values_follow_the_reference_expressions():
    """'uniform' x0_xy is sqrt(U(min, max)); a 'uniform' v0_xy is U itself; a 'gaussian' entry the reference does not
    rescale is the raw standard normal; a gamma shape below 1 takes the boost."""
    cfg = _config(x0__x0_xy={"distribution": "uniform", "min": 0, "max": 40},
                  v0__v0_xy={"distribution": "uniform", "min": 5, "max": 25},
                  a={"distribution": "gaussian", "mean": 1.0, "std": 2.0},
                  rho={"distribution": "gaussian"}, m={"distribution": "gamma", "shape": 0.5, "scale": 2.0},
                  x0__x0_z={"distribution": "gaussian", "mean": 1.5, "std": 0.33})
    h = G.sample_candidates_host(cfg, SEED, 0, N_KS)
    crit = 1.95 / np.sqrt(N_KS)
    assert st.kstest(np.hypot(h["x0_x"], h["x0_y"]) ** 2, st.uniform(0, 40).cdf).statistic < crit
    assert st.kstest(np.hypot(h["v0_x"], h["v0_y"]), st.uniform(5, 20).cdf).statistic < crit
    assert st.kstest(h["rho"], st.norm(0, 1).cdf).statistic < crit
    assert st.kstest(h["m"], st.gamma(0.5, scale=2.0).cdf).statistic < crit
    assert st.kstest(h["x0_z"], st.norm(1.5, 0.33).cdf).statistic < crit
    r_a = np.sqrt(h["a_x"] ** 2 + h["a_y"] ** 2 + h["a_z"] ** 2)            # cbrt(|n|) 2 + 1
    assert st.kstest(((r_a - 1.0) / 2.0) ** 3, st.halfnorm().cdf).statistic < crit


def test_config_errors():
    with pytest.raises(ValueError, match="Unknown distribution type: beta"):
        G.slot_tables(_config(g={"distribution": "beta"}))
    with pytest.raises(ValueError, match="Unknown distribution type"):
        G.slot_tables(_config(x0__x0_xy={"distribution": "gamma", "shape": 2, "scale": 1}))
    with pytest.raises(ValueError, match="min and max must be defined"):
        G.slot_tables(_config(cam_heights={"distribution": "uniform", "min": 0.4}))
    with pytest.raises(ValueError, match="shape and scale must be defined"):
        G.slot_tables(_config(m={"distribution": "gamma", "shape": 2}))
    for fn in (G.generate_data, G.generate_data_device):
        with pytest.raises(ValueError, match='output_type must be one of "videos", "trajectories", or "parameters"'):
            fn(CONFIG, n=1, output_type="render")
        with pytest.raises(ValueError, match="unpack"):
            fn(CONFIG, n=1, num_cams=3)
        with pytest.raises(ValueError, match="ratio"):
            fn(CONFIG, n=1, ratio=(4, 3))
        with pytest.raises(ValueError, match="Unknown distribution type"):
            fn(_config(g={"distribution": "beta"}), n=1, device="cpu")
        with pytest.raises(RuntimeError, match="HIP device only"):
            fn(CONFIG, n=1, device="cpu")
    assert G.candidate_limit(2, 30) == 2**32 // 60


def test_slot_order_and_tables():
    names = G.slot_names(2)
    assert len(names) == 25 and names[:3] == ["x0_xy", "phi", "x0_z"] and names[12:17] == ["g", "rho", "r_ball", "Cd", "m"]
    assert names[17:] == ["cam_radian", "cam_radius", "cam_angle", "cam_angle", "cam_heights", "cam_heights",
                          "u_distance", "u_visibility"]
    kind, xf, p0, p1 = G.slot_tables(G.load_data_config(CONFIG))
    assert kind.tolist()[:12] == [1, 0, 0, 1, 0, 1, 1, 0, 1, 1, 0, 0] and set(kind[12:17]) == {G.GAMMA}
    assert xf.tolist()[:12] == [G.XF_SQRT_ABS, 0, 0, G.XF_SQRT_ABS, 0, G.XF_AFFINE, G.XF_SQRT_ABS, 0, G.XF_AFFINE,
                                G.XF_CBRT_ABS, 0, 0]
    assert (p0[15], p1[15], p0[16], p1[16]) == (2.0, 0.35, 2.0, 0.15)          # Cd and m as the config states them


def test_assembled_dict_feeds_the_reference_data_handling(g20):
    """assemble() on the accepted rows: the reference's keys in its order, and what trainer_data_handler.py:75-86 does
    with the dict (condition stacking, ParameterIndexMapping.vectorize) works unchanged."""
    rows = g20["rows"][g20["accepted"]]
    traj = g20["trajectories"]
    params = G.assemble(rows)
    assert list(params.keys()) == list(G.KEYS)
    data = G.assemble(rows, traj, None, "trajectories")
    assert list(data.keys()) == list(G.KEYS) + ["trajectories"]
    assert list(G.assemble(rows, traj, np.zeros((64, 2, 30, 1, 1)), "videos").keys()) == \
        list(G.KEYS) + ["videos", "trajectories"]
    with pytest.raises(ValueError, match="output_type"):
        G.assemble(rows, output_type="gif")
    assert data["cam_radian_array"].shape == (64, 2) and data["cam_angles"].shape == (64, 2) and data["m"].shape == (64,)
    selection = ['x0_x', 'x0_y', 'x0_z', 'v0_x', 'v0_y', 'v0_z', 'g_z', 'w_x', 'w_y', 'w_z', 'b', 'm', 'a_x', 'a_y', 'a_z',
                 'r', 'A', 'Cd', 'rho']
    y = ParameterIndexMapping(selection).vectorize(data)
    assert y.shape == (64, 19) and np.array_equal(y[:, 6], rows[:, 8])
    conditions = []
    for condition_keys in [["trajectories"], ["cam_radian_array", "cam_radius", "cam_angles", "cam_heights"]]:
        values = []
        for c in condition_keys:
            value = np.array(data[c])
            if value.ndim == 1:
                value = value[:, None]
            values.append(value)
        conditions.append(np.concatenate(values, axis=1))
    assert conditions[0].shape == (64, 30, 3) and conditions[1].shape == (64, 7)


def test_accept_visibility_is_the_reference_rule():
    lit = np.array([60, 46, 45, 30, 30, 0])
    u = np.array([0.99, 0.99, 0.9, 0.49, 0.51, 0.001])
    assert G.accept_visibility(lit, 60, u).tolist() == [True, True, True, True, False, True]
