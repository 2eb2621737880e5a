"""Generate g20_generate.npz by running the REFERENCE's generate_data (psaegert/bcnf src/bcnf/simulation/sampling.py:
287-410, with its own sample_ballistic_parameters, calculate_point_of_impact, physics_ODE_simulation, record_trajectory
and accept_* filters) on CPU, fed the draws of bcnf_amd's documented rule.

Test infrastructure only, run like make_golden_render.py (nothing of the reference is copied, only inputs / outputs).
The reference checkout's src directory is the first argument, or $BCNF_REFERENCE_SRC:

    python tests/golden/make_golden_generate.py path/to/reference/src

The priors are tests/golden/data_config.yaml, a copy of the reference's configs/data/config.yaml (settings only). The
dynaconf stub returns that YAML as a dict. The reference draws from numpy's global stream; while it runs,
    np.random.uniform(lo, hi)   -> lo + (hi - lo) * generate.slot_uniform(seed, candidate, slot)
    np.random.normal(0, 1)      -> generate.slot_normal(seed, candidate, slot)
    np.random.gamma(k, theta)   -> generate.slot_gamma(seed, candidate, slot, k, theta)
replay the rule's slots in call order for candidates 0, 1, 2, ... (a candidate starts at each call of
sample_ballistic_parameters); the two conditional uniform(0, 1) calls of accept_traveled_distance and accept_visibility
are routed to their own slots by the calling function's name, and np.random.normal(loc, scale, (5000, 3)) becomes
loc + scale * render.standard_normals(seed, 0, candidate * 2 * frames + call, 5000), the camera's rule at the
candidate's frame indices. calculate_point_of_impact, the two filters and np.histogram2d are wrapped to record what they
return.

Run: generate_data(n = 64, output_type = 'trajectories', dt = 0.067, T = 2.0, do_filter = True): 30 frames x 2 cameras.

Conditions, enforced here (a violation moves to the next seed; the seed used is stored):
  * every candidate that reaches the distance filter has |distance / 50 - 0.75| > 1e-4 and |sqrt(distance / 50) - u| > 1e-4;
  * every candidate that reaches the visibility filter gets the same decision for lit - 1, lit and lit + 1 lit frames;
  * no Marsaglia-Tsang acceptance test lies within 1e-9 of equality.
Under these, a correct implementation whose trajectories differ from odeint's at the level of `poi_tol` accepts exactly
the same candidates. About 800 candidates are examined for 64 acceptances, some 90 of them with a visibility between
0 and 0.75, where one lit frame moves the sigmoid by up to 0.04: about one seed in 2000 meets the second condition, and
one run of the reference takes a minute. SEED is therefore the first seed a search with bcnf_amd's own pipeline found to
meet the conditions (none of the 6171 seeds 20_240_325 ... 20_246_495 does); the loop below still checks them on the reference's run.
poi_tol: the reference's points of impact are compared with the same march integrated by
scipy.integrate.solve_ivp (DOP853, rtol = atol = 1e-12); poi_tol = 2e-6 (tests/test_resim.py's RTOL = ATOL: the same pair
of integrators) unless the reference alone deviates by more, then 4 x that deviation.

Stored per candidate: the parameter row (bcnf_amd.generate.COLUMNS layout, with the two filter uniforms), point of
impact and distance (NaN when not computed), reject code (0 accepted, 1 runaway, 2 underground, 3 distance,
4 visibility), lit-frame count (-1 when not rendered); the accepted indices, their trajectories and the reference's
rejection counters. No videos.
"""
import os
import sys
import tempfile
from unittest import mock

import numpy as np

REF_SRC = sys.argv[1] if len(sys.argv) > 1 else os.environ.get("BCNF_REFERENCE_SRC")
OUT = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(OUT))
CONFIG = os.path.join(OUT, "data_config.yaml")
SEED = 20_247_872
N_ACC, T, DT, NC = 64, 2.0, 0.067, 2
RESIM_TOL = 2e-6


class Violation(Exception):
    pass


def _import_reference():
    if not REF_SRC or not os.path.isdir(REF_SRC):
        raise SystemExit("usage: make_golden_generate.py path/to/reference/src (or set BCNF_REFERENCE_SRC)")
    stub = tempfile.mkdtemp(prefix="bcnf_stub_")
    os.makedirs(os.path.join(stub, "dynaconf"))
    with open(os.path.join(stub, "dynaconf", "__init__.py"), "w") as f:
        f.write("import yaml\n\n\nclass Dynaconf(dict):\n    def __init__(self, settings_files=(), **k):\n"
                "        with open(settings_files[0]) as f:\n            super().__init__(yaml.safe_load(f))\n")
    sys.dont_write_bytecode = True
    sys.path[:0] = [stub, REF_SRC, ROOT]
    import matplotlib
    matplotlib.use("Agg")
    import bcnf.simulation.physics as physics  # noqa
    import bcnf.simulation.sampling as sampling  # noqa
    return sampling, physics


def run_reference(sampling, seed):
    from bcnf_amd import generate as G
    from bcnf_amd.render import standard_normals
    frames = len(np.arange(0, T, DT))
    n_slots = len(G.slot_names(NC))
    st = {"cand": -1, "slot": 0, "frame": 0, "margin": np.inf}
    rec = {"params": [], "poi": {}, "dist": {}, "code": [], "lit": {}, "accepted": [], "u": []}
    real = {"sample": sampling.sample_ballistic_parameters, "poi": sampling.calculate_point_of_impact,
            "dist": sampling.accept_traveled_distance, "vis": sampling.accept_visibility, "hist": np.histogram2d}

    def uniform(low=0.0, high=1.0, size=None):
        assert size is None
        caller = sys._getframe(1).f_code.co_name
        if caller == "accept_traveled_distance":
            s = n_slots - 2
        elif caller == "accept_visibility":
            s = n_slots - 1
        else:
            s = st["slot"]
            st["slot"] += 1
        return low + (high - low) * G.slot_uniform(seed, [st["cand"]], s)[0]

    def normal(loc=0.0, scale=1.0, size=None):
        if size is None:
            assert loc == 0 and scale == 1
            st["slot"] += 1
            return G.slot_normal(seed, [st["cand"]], st["slot"] - 1)[0]
        assert tuple(size) == (5000, 3)
        z = standard_normals(seed, 0, st["cand"] * NC * frames + st["frame"], 5000)
        st["frame"] += 1
        return loc + scale * z

    def gamma(shape, scale=1.0, size=None):
        assert size is None
        st["slot"] += 1
        val, margin = G.slot_gamma(seed, [st["cand"]], st["slot"] - 1, shape, scale, return_margin=True)
        st["margin"] = min(st["margin"], float(margin[0]))
        return val[0]

    def sample(*a, **k):
        st.update(cand=st["cand"] + 1, slot=0, frame=0)
        p = real["sample"](*a, **k)
        assert st["slot"] == n_slots - 2
        rec["params"].append({key: np.array(v, dtype=np.float64) for key, v in p.items()})
        rec["code"].append(1 if p["g_z"] + p["a_z"] > 0 else (2 if p["x0_z"] < 0 else 0))
        rec["lit"][st["cand"]] = []
        return p

    def poi(**k):
        out = real["poi"](**k)
        rec["poi"][st["cand"]] = np.array(out, dtype=np.float64)
        return out

    def dist(distance):
        ok = real["dist"](distance)
        rec["dist"][st["cand"]] = distance
        if not ok:
            rec["code"][st["cand"]] = 3
        return ok

    def vis(visibility):
        ok = real["vis"](visibility)
        if ok:
            rec["accepted"].append(st["cand"])
        else:
            rec["code"][st["cand"]] = 4
        return ok

    def hist(*a, **k):
        vals = real["hist"](*a, **k)
        rec["lit"][st["cand"]].append(int(np.sum(vals[0]) > 0))
        return vals

    with mock.patch.object(np.random, "uniform", uniform), mock.patch.object(np.random, "normal", normal), \
            mock.patch.object(np.random, "gamma", gamma), mock.patch.object(np, "histogram2d", hist), \
            mock.patch.object(sampling, "sample_ballistic_parameters", sample), \
            mock.patch.object(sampling, "calculate_point_of_impact", poi), \
            mock.patch.object(sampling, "accept_traveled_distance", dist), \
            mock.patch.object(sampling, "accept_visibility", vis):
        data = sampling.generate_data(config_file=CONFIG, n=N_ACC, output_type="trajectories", dt=DT, T=T,
                                      do_filter=True)
    return data, rec, st["margin"], frames


def march_dop853(row):
    """calculate_point_of_impact's march (physics.py:246-276) with solve_ivp DOP853 at 1e-12 in place of odeint."""
    from scipy.integrate import solve_ivp
    x0, v0, g, w = row[0:3].copy(), row[3:6].copy(), row[6:9], row[9:12]
    b, m, a, r, rho = row[12], row[13], row[14:17], row[19], row[22]

    def f(t, v):
        return g - g * rho * (4 / 3) * (np.pi * r**3) / m - (0.5 * b / m) * (
            v**2 * v / np.linalg.norm(v) - w**2 * w / np.linalg.norm(w)) + a

    t, dt = 0.0, 0.1
    while t < 120.0:
        sol = solve_ivp(f, (t, t + dt), v0, method="DOP853", rtol=1e-12, atol=1e-12)
        x1 = x0 + v0 * dt
        if x1[2] < 0:
            return x0 + v0 * (-x0[2] / v0[2])
        x0, v0 = x1, sol.y[:, -1]
        t += dt
    return np.array([999.0, 999.0, 999.0])


def main():
    sampling, _ = _import_reference()
    from bcnf_amd import generate as G
    seed = SEED
    while True:
        try:
            data, rec, margin, frames = run_reference(sampling, seed)
            ncand = len(rec["params"])
            host = G.sample_candidates_host(CONFIG, seed, 0, ncand, NC)
            rows = np.full((ncand, G.NCOL), np.nan)
            for c, p in enumerate(rec["params"]):
                for key in G.KEYS:
                    v = p[key]
                    if key == "cam_radian_array":
                        v = np.insert(v, 0, 0.0)
                    rows[c, G.COLUMNS[key]] = v
            rows[:, G.COL_U_DISTANCE], rows[:, G.COL_U_VISIBILITY] = host["u_distance"], host["u_visibility"]
            for key in G.KEYS:      # the numpy restatement against the reference's own expressions: bit for bit
                want = rows[:, G.COLUMNS[key]][:, 1:] if key == "cam_radian_array" else rows[:, G.COLUMNS[key]]
                if not np.array_equal(np.asarray(host[key]).view(np.uint64), np.ascontiguousarray(want).view(np.uint64)):
                    raise SystemExit(f"sample_candidates_host and the reference disagree on {key}")
            if not margin > 1e-9:
                raise Violation(f"a Marsaglia-Tsang test lies within {margin} of equality")
            poi = np.full((ncand, 3), np.nan)
            dist = np.full(ncand, np.nan)
            lit = np.full(ncand, -1, dtype=np.int32)
            code = np.array(rec["code"], dtype=np.int32)
            for c, d in rec["dist"].items():
                poi[c], dist[c] = rec["poi"][c], d
                ratio = d / 50
                if abs(ratio - 0.75) <= 1e-4 or abs(np.sqrt(ratio) - rows[c, G.COL_U_DISTANCE]) <= 1e-4:
                    raise Violation(f"candidate {c}: the distance decision is within 1e-4 of its threshold")
            for c, frames_lit in rec["lit"].items():
                if not frames_lit:
                    continue
                assert len(frames_lit) == NC * frames
                lit[c] = sum(frames_lit)
                u = rows[c, G.COL_U_VISIBILITY]
                votes = {bool(G.accept_visibility(k, NC * frames, u)) for k in (lit[c] - 1, lit[c], lit[c] + 1)
                         if 0 <= k <= NC * frames}
                if len(votes) != 1 or votes != {code[c] == 0}:
                    raise Violation(f"candidate {c}: the visibility decision changes within one lit frame")
            break
        except Violation as v:
            print(f"seed {seed}: {v}; next seed", flush=True)
            seed += 1
    accepted = np.array(rec["accepted"], dtype=np.int64)
    assert len(accepted) == N_ACC and accepted[-1] == ncand - 1 and (code[accepted] == 0).all()
    traj = np.array(data["trajectories"])
    assert traj.shape == (N_ACC, frames, 3)
    for key in G.KEYS:      # the returned dict is the accepted candidates' rows
        assert np.array_equal(np.array(data[key], dtype=np.float64), rows[accepted][:, G.COLUMNS[key]]), key
    # the reference's own integration error in the point of impact, against DOP853 at 1e-12
    worst = 0.0
    for c in np.nonzero(~np.isnan(dist))[0]:
        hi = march_dop853(rows[c])
        if (poi[c] == 999.0).all() or (hi == 999.0).all():
            assert np.array_equal(poi[c], hi), c
            continue
        worst = max(worst, float(np.max(np.abs(poi[c] - hi) / (1.0 + np.abs(hi)))))
    poi_tol = RESIM_TOL if worst <= RESIM_TOL else 4 * worst
    counters = np.array([(code == k).sum() for k in (1, 2, 3, 4)], dtype=np.int64)
    print(f"seed {seed}: {ncand} candidates, {N_ACC} accepted; runaway / underground / distance / visibility = "
          f"{counters.tolist()}; far points {(poi[:, 0] == 999.0).sum()}; reference deviation {worst:.3e}, "
          f"poi_tol {poi_tol:.3e}; gamma margin {margin:.3e}")
    path = os.path.join(OUT, "g20_generate.npz")
    np.savez_compressed(path, seed=np.int64(seed), T=np.float64(T), dt=np.float64(DT), rows=rows, poi=poi, distance=dist,
                        code=code, lit=lit, accepted=accepted, trajectories=traj, counters=counters,
                        poi_tol=np.float64(poi_tol), reference_deviation=np.float64(worst))
    size = os.path.getsize(path)
    print(f"{path}: {size} bytes")
    if size > 1000_000:
        raise SystemExit("g20_generate.npz is over 1 MB")


if __name__ == "__main__":
    main()
