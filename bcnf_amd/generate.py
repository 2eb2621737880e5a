"""generate_data (psaegert/bcnf src/bcnf/simulation/sampling.py:287-410) on the GPU: the reference's rejection loop over
prior draws, with its four filters (runaway, start underground, travelled distance, visibility).

The reference runs one Python iteration per candidate: sample_ballistic_parameters (sampling.py:156-284), up to 1200
odeint calls in calculate_point_of_impact (physics.py:246-276), one physics_ODE_simulation and 2 x frames camera() calls
for the visibility. Here a chunk of candidates takes four launches:

  1. bcnf_sample_candidates (csrc/bcnf_generate.hip): the draws, the parameter rows, the runaway / underground tests,
     the point of impact and the distance filter;
  2. bcnf_resimulate on the rows of the candidates still pending (the call's T, dt, break_on_impact);
  3. bcnf_render_lit: the in-view sample count of every frame of those candidates -- the camera's device code without
     its histogram and images;
  4. bcnf_render_frames_at, once at the end and only for output_type 'videos': the videos of the accepted samples.

Defining property: candidate c is a pure function of (seed, c) and the arguments, and the result is the first n accepted
candidates in candidate order from first_candidate on. It does not depend on `chunk`, on n beyond truncation, or on the
launch a candidate ran in. The draws follow a counter-based rule (the reference uses numpy's global stream, which no
kernel can follow); `sample_candidates_host` is its normative statement:

  slot s of candidate c, attempt t:  (w0, w1, w2, w3) = Philox4x32-10 with counter (c low, c high, s, t) and key
      (seed low, seed high ^ 0x60000000);  u_i = (w_i + 0.5) 2^-32
  uniform(lo, hi) = lo + (hi - lo) u0;   normal = sqrt(-2 ln u0) cos(2 pi u1)   (float64 Box-Muller)
  gamma(k, theta): Marsaglia-Tsang without the squeeze, k' = k or k + 1 below 1, d = k' - 1/3, c = 1 / sqrt(9 d); attempt
      t = 0, 1, ...: x = normal(w0, w1), v = (1 + c x)^3, accepted when v > 0 and ln u2 < x^2 / 2 + d - d v + d ln v;
      value d v theta, times u3^(1/k) first when k < 1
  slots in the call order of sample_ballistic_parameters (SLOT_NAMES), then the uniforms of accept_traveled_distance and
  accept_visibility; the transformations are the reference's expressions per `distribution` value.
  Frame (cam, t) of candidate c is frame c num_cams frames + cam frames + t of the camera's draw rule
  (render.standard_normals) with the same seed and offset 0, so candidates lie below 2^32 / (num_cams frames).

There is no CPU path: sample_candidates_host states the draws, the kernels do the work.
"""
from __future__ import annotations

import ctypes

import numpy as np
import torch
import yaml

from . import _native
from . import render as R
from .resimulation import STATUS_OK, time_grid

DEFAULT_SEED = 2024_03_25
KEY_TAG = 0x60000000               # include/bcnf_amd.h BCNF_GEN_KEY_TAG
NCOL = 30                          # include/bcnf_amd.h BCNF_GEN_NCOL
GAMMA_MAX_ATTEMPTS = 1000
UNIFORM, GAUSSIAN, GAMMA = 0, 1, 2
XF_NONE, XF_SQRT_ABS, XF_AFFINE, XF_CBRT_ABS, XF_SQRT = 0, 1, 2, 3, 4
PENDING, RUNAWAY, UNDERGROUND, DISTANCE, VISIBILITY = 0, 1, 2, 3, 4
REJECT_NAMES = {RUNAWAY: "runaway", UNDERGROUND: "start_underground", DISTANCE: "distance", VISIBILITY: "visibility"}
OUTPUT_TYPES = ("videos", "trajectories", "parameters")

# the reference's dict, in its key order (sampling.py:258-284), and the columns of a kernel row that hold each key
KEYS = ("x0_x", "x0_y", "x0_z", "v0_x", "v0_y", "v0_z", "g_x", "g_y", "g_z", "w_x", "w_y", "w_z", "b", "m", "a_x", "a_y",
        "a_z", "cam_radian_array", "r", "A", "Cd", "rho", "cam_radius", "cam_angles", "cam_heights")
COLUMNS = {"x0_x": 0, "x0_y": 1, "x0_z": 2, "v0_x": 3, "v0_y": 4, "v0_z": 5, "g_x": 6, "g_y": 7, "g_z": 8, "w_x": 9,
           "w_y": 10, "w_z": 11, "b": 12, "m": 13, "a_x": 14, "a_y": 15, "a_z": 16, "cam_radian_array": slice(17, 19),
           "r": 19, "A": 20, "Cd": 21, "rho": 22, "cam_radius": 23, "cam_angles": slice(24, 26),
           "cam_heights": slice(26, 28)}
COL_U_DISTANCE, COL_U_VISIBILITY = 28, 29
# physics_ODE_simulation's parameters (resimulation.PHYSICS_PARAMETERS order) as columns of a row
_PHYSICS_COLUMNS = (0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11, 12, 13, 22, 19, 14, 15, 16)


def slot_names(num_cams: int = 2) -> list[str]:
    """The slots of a candidate in the call order of sample_ballistic_parameters (sampling.py:162-254), then the two
    conditional uniforms of the filters."""
    return (["x0_xy", "phi", "x0_z", "v0_xy", "phi_v", "v0_z", "w_xy", "phi_w", "w_z", "a", "phi_a", "theta_a", "g", "rho",
             "r_ball", "Cd", "m"] + ["cam_radian"] * (num_cams - 1) + ["cam_radius"] + ["cam_angle"] * num_cams +
            ["cam_heights"] * num_cams + ["u_distance", "u_visibility"])


def load_data_config(config_file) -> dict:
    """The configs/data/*.yaml layout as a dict: a path is read with yaml, a dict is taken as it is."""
    if isinstance(config_file, dict):
        return config_file
    with open(config_file) as f:
        return yaml.safe_load(f)


def _raw(values: dict):
    """sample_from_config (sampling.py:107-121): (kind, p0, p1) of the raw draw, with its errors."""
    kind = values["distribution"]
    if kind == "uniform":
        if "min" not in values or "max" not in values:
            raise ValueError("min and max must be defined for uniform distribution")
        return UNIFORM, float(values["min"]), float(values["max"])
    if kind == "gaussian":
        return GAUSSIAN, 0.0, 1.0
    if kind == "gamma":
        if "shape" not in values or "scale" not in values:
            raise ValueError("shape and scale must be defined for gamma distribution")
        if not float(values["shape"]) > 0:
            raise ValueError("shape must be positive for gamma distribution")
        return GAMMA, float(values["shape"]), float(values["scale"])
    raise ValueError(f"Unknown distribution type: {kind}")


def _rescaled(values: dict, gaussian_xf: int, uniform_xf: int):
    """An entry sample_ballistic_parameters branches on: 'gaussian' is rescaled with mean / std, 'uniform' is taken (or
    square-rooted); anything else leaves the reference's variable unset."""
    kind = values["distribution"]
    if kind == "gaussian":
        return GAUSSIAN, float(values["mean"]), float(values["std"]), gaussian_xf
    if kind == "uniform":
        return _raw(values) + (uniform_xf,)
    raise ValueError(f"Unknown distribution type: {kind}")


def slot_tables(config: dict, num_cams: int = 2):
    """(kind, transform, p0, p1) per slot: what sample_ballistic_parameters does with each entry of the config, as the
    tables bcnf_sample_candidates takes. p0, p1 = min, max | mean, std | shape, scale."""
    cfg = config
    two_pi = 2 * np.pi
    angle = (UNIFORM, 0.0, two_pi, XF_NONE)
    plain = lambda v: _raw(v) + (XF_NONE,)  # noqa: E731
    slots = [_rescaled(cfg["x0"]["x0_xy"], XF_SQRT_ABS, XF_SQRT), angle, _rescaled(cfg["x0"]["x0_z"], XF_AFFINE, XF_NONE),
             _rescaled(cfg["v0"]["v0_xy"], XF_SQRT_ABS, XF_NONE), angle, _rescaled(cfg["v0"]["v0_z"], XF_AFFINE, XF_NONE),
             _rescaled(cfg["w"]["w_xy"], XF_SQRT_ABS, XF_NONE), angle, _rescaled(cfg["w"]["w_z"], XF_AFFINE, XF_NONE),
             _rescaled(cfg["a"], XF_CBRT_ABS, XF_NONE), angle, (UNIFORM, 0.0, float(np.pi), XF_NONE),
             plain(cfg["g"]), plain(cfg["rho"]), plain(cfg["r_ball"]), plain(cfg["Cd"]), plain(cfg["m"])]
    slots += [plain(cfg["cam_radian"])] * (num_cams - 1) + [plain(cfg["cam_radius"])]
    slots += [plain(cfg["cam_angle"])] * num_cams + [plain(cfg["cam_heights"])] * num_cams
    slots += [(UNIFORM, 0.0, 1.0, XF_NONE)] * 2
    kind = np.array([s[0] for s in slots], dtype=np.int32)
    p0 = np.array([s[1] for s in slots], dtype=np.float64)
    p1 = np.array([s[2] for s in slots], dtype=np.float64)
    xf = np.array([s[3] for s in slots], dtype=np.int32)
    return kind, xf, p0, p1


# ---- the draw rule in numpy (normative) ----------------------------------------------------------------------------

def _words(seed: int, cand: np.ndarray, slot: int, attempt: int):
    seed = int(seed) & (2**64 - 1)
    cand = np.asarray(cand, dtype=np.uint64)
    return R.philox4x32_10(cand & np.uint64(0xFFFFFFFF), cand >> np.uint64(32), slot, attempt, seed & 0xFFFFFFFF,
                           ((seed >> 32) ^ KEY_TAG) & 0xFFFFFFFF)


def _unit(w) -> np.ndarray:
    return (w.astype(np.float64) + 0.5) * 2.0 ** -32


def slot_uniform(seed, cand, slot) -> np.ndarray:
    """u0 of (candidate, slot), strictly inside (0, 1)."""
    return _unit(_words(seed, cand, slot, 0)[0])


def _box_muller(w0, w1) -> np.ndarray:
    return np.sqrt(-2.0 * np.log(_unit(w0))) * np.cos(R.TWO_PI * _unit(w1))


def slot_normal(seed, cand, slot) -> np.ndarray:
    w = _words(seed, cand, slot, 0)
    return _box_muller(w[0], w[1])


def slot_gamma(seed, cand, slot, shape: float, scale: float, return_margin: bool = False):
    """np.random.gamma(shape, scale)'s stand-in. With return_margin also the smallest |rhs - ln u2| over every
    acceptance test taken (how close a decision came to equality)."""
    cand = np.atleast_1d(np.asarray(cand, dtype=np.uint64))
    k = shape + 1.0 if shape < 1.0 else shape
    d = k - 1.0 / 3.0
    c = 1.0 / np.sqrt(9.0 * d)
    out = np.full(cand.shape, np.nan)
    margin = np.full(cand.shape, np.inf)
    todo = np.arange(cand.size)
    for attempt in range(GAMMA_MAX_ATTEMPTS):
        if not todo.size:
            break
        w = _words(seed, cand[todo], slot, attempt)
        x = _box_muller(w[0], w[1])
        t = 1.0 + c * x
        v = t * t * t
        pos = v > 0.0
        with np.errstate(invalid="ignore", divide="ignore"):
            rhs = 0.5 * x * x + d - d * v + d * np.log(v)
            lhs = np.log(_unit(w[2]))
            ok = pos & (lhs < rhs)
        margin[todo[pos]] = np.minimum(margin[todo[pos]], np.abs(rhs - lhs)[pos])
        val = d * v[ok]
        if shape < 1.0:
            val = val * np.power(_unit(w[3][ok]), 1.0 / shape)
        out[todo[ok]] = val * scale
        todo = todo[~ok]
    return (out, margin) if return_margin else out


def sample_candidates_host(config, seed: int, first: int, count: int, num_cams: int = 2) -> dict:
    """Candidates first .. first + count - 1 of the draw rule: the dict of sample_ballistic_parameters (its keys, its
    order; float64 arrays over the candidates, cam_radian_array (count, num_cams - 1) as drawn, cam_angles and
    cam_heights (count, num_cams)) plus 'u_distance' and 'u_visibility', the uniforms the two conditional filters
    consume. Every expression is the reference's own on the rule's draws, so the values are the reference's bit for
    bit when its np.random calls are fed these draws (tests/golden/make_golden_generate.py)."""
    config = load_data_config(config_file=config)
    kind, xf, p0, p1 = slot_tables(config, num_cams)
    cand = np.arange(int(first), int(first) + int(count), dtype=np.uint64)
    val = []
    for s in range(len(kind)):
        if kind[s] == UNIFORM:
            raw = p0[s] + (p1[s] - p0[s]) * slot_uniform(seed, cand, s)
        elif kind[s] == GAUSSIAN:
            raw = slot_normal(seed, cand, s)
        else:
            raw = slot_gamma(seed, cand, s, p0[s], p1[s])
        if xf[s] == XF_SQRT_ABS:
            raw = np.sqrt(np.abs(raw)) * p1[s] + p0[s]
        elif xf[s] == XF_AFFINE:
            raw = raw * p1[s] + p0[s]
        elif xf[s] == XF_CBRT_ABS:
            raw = np.cbrt(np.abs(raw)) * p1[s] + p0[s]
        elif xf[s] == XF_SQRT:
            raw = np.sqrt(raw)
        val.append(raw)
    r_x, phi, x0_z, r_v, phi_v, v0_z, r_w, phi_w, w_z, r_a, phi_a, theta_a, g, rho, r, Cd, m = val[:17]
    nc = num_cams
    # r**2 on a float64 SCALAR, as the reference evaluates it, is libm's pow(r, 2); an array's r**2 is r * r, which
    # differs from it in the last bit about once in 2000 draws. So the scalar expression runs per candidate.
    A = np.pi * np.array([x**2 for x in r], dtype=np.float64)
    zero = np.zeros(len(cand))
    out = {"x0_x": r_x * np.cos(phi), "x0_y": r_x * np.sin(phi), "x0_z": x0_z,
           "v0_x": r_v * np.cos(phi_v), "v0_y": r_v * np.sin(phi_v), "v0_z": v0_z,
           "g_x": zero, "g_y": zero.copy(), "g_z": -g,
           "w_x": r_w * np.cos(phi_w), "w_y": r_w * np.sin(phi_w), "w_z": w_z,
           "b": rho * A * Cd, "m": m,
           "a_x": r_a * np.sin(theta_a) * np.cos(phi_a), "a_y": r_a * np.sin(theta_a) * np.sin(phi_a),
           "a_z": r_a * np.cos(theta_a),
           "cam_radian_array": np.stack(val[17:16 + nc], 1) if nc > 1 else np.zeros((len(cand), 0)),
           "r": r, "A": A, "Cd": Cd, "rho": rho, "cam_radius": val[16 + nc],
           "cam_angles": np.stack(val[17 + nc:17 + 2 * nc], 1), "cam_heights": np.stack(val[17 + 2 * nc:17 + 3 * nc], 1),
           "u_distance": val[17 + 3 * nc], "u_visibility": val[18 + 3 * nc]}
    return out


# ---- host-side assembly --------------------------------------------------------------------------------------------

def _check_arguments(output_type, num_cams, ratio, n, first_candidate, chunk):
    if output_type not in OUTPUT_TYPES:
        raise ValueError('output_type must be one of "videos", "trajectories", or "parameters"')
    if num_cams != 2:      # render.get_cams_position: the reference's loop unpacks exactly two cameras
        raise ValueError(f"too many values to unpack (expected 2, got {num_cams})" if num_cams > 2 else
                         f"not enough values to unpack (expected 2, got {num_cams})")
    if tuple(ratio) != (R.WIDTH // 10, R.HEIGHT // 10):
        raise ValueError(f"the kernel renders {R.HEIGHT} x {R.WIDTH} frames (ratio (16, 9)); got ratio {tuple(ratio)}")
    if n < 0 or first_candidate < 0 or chunk < 1:
        raise ValueError("n and first_candidate must not be negative and chunk must be positive")


def candidate_limit(num_cams: int, frames: int) -> int:
    """Candidates lie below this: their frames' indices must stay below 2^32."""
    return 2**32 // max(1, num_cams * frames)


def accept_visibility(lit, n_frames: int, u) -> np.ndarray:
    """sampling.py:134-142 on arrays: vis = lit / n_frames (a lit frame sums to 1, an empty one to 0)."""
    vis = np.asarray(lit, dtype=np.float64) / n_frames
    return (vis > 0.75) | (1 / (1 + np.exp(-(vis - 0.5) * 10)) > np.asarray(u))


def assemble(rows, trajectories=None, videos=None, output_type: str = "parameters") -> dict:
    """The returned dict from the accepted candidates' rows (n, NCOL): the reference's keys in its order, then
    'videos' and 'trajectories' as generate_data appends them. Works on torch tensors and numpy arrays alike."""
    if output_type not in OUTPUT_TYPES:
        raise ValueError('output_type must be one of "videos", "trajectories", or "parameters"')
    data = {key: rows[:, COLUMNS[key]] for key in KEYS}
    if output_type == "videos":
        data["videos"] = videos
        data["trajectories"] = trajectories
    elif output_type == "trajectories":
        data["trajectories"] = trajectories
    return data


def _stats(codes: np.ndarray, not_ok: np.ndarray) -> dict:
    stats = {"candidates": int(codes.size)}
    stats.update({name: int((codes == code).sum()) for code, name in REJECT_NAMES.items()})
    stats["trajectory_not_ok"] = int(not_ok.sum())
    return stats


# ---- the device pipeline -------------------------------------------------------------------------------------------

def sample_candidates_device(config, seed: int, first: int, count: int, cam1_radian: float = 0.0,
                             do_filter: bool = True, rtol: float = 1e-10, atol: float = 1e-10,
                             max_attempts: int = 1_000_000, device=None):
    """One launch of bcnf_sample_candidates: (rows (count, NCOL), poi (count, 3), distance (count,), code (count,)
    int32) on the device."""
    device = _device(device)
    kind, xf, p0, p1 = slot_tables(load_data_config(config), 2)
    rows = torch.empty((count, NCOL), dtype=torch.float64, device=device)
    poi = torch.empty((count, 3), dtype=torch.float64, device=device)
    dist = torch.empty((count,), dtype=torch.float64, device=device)
    code = torch.empty((count,), dtype=torch.int32, device=device)
    if count:
        with torch.cuda.device(device):
            _native.call("bcnf_sample_candidates", kind.ctypes.data_as(ctypes.c_void_p),
                         xf.ctypes.data_as(ctypes.c_void_p), p0.ctypes.data_as(ctypes.c_void_p),
                         p1.ctypes.data_as(ctypes.c_void_p), int(seed) & (2**64 - 1), int(first), int(count),
                         float(cam1_radian), bool(do_filter), float(rtol), float(atol), int(max_attempts), rows, poi,
                         dist, code, _native.stream_handle(device))
    return rows, poi, dist, code


def _device(device):
    if device is None:
        device = torch.device("cuda", torch.cuda.current_device())
    device = torch.device(device)
    if device.type != "cuda":
        raise RuntimeError("bcnf_amd.generate_data runs on the HIP device only (no CPU path); got " + str(device))
    return device


def _simulate(rows, T, dt, break_on_impact, device):
    """bcnf_resimulate on the rows' physics columns: ((n, steps, 3) positions, (n,) status)."""
    n = rows.shape[0]
    t = time_grid(T, dt)
    steps = len(t)
    if steps == 0:
        raise IndexError("index 0 is out of bounds for axis 0 with size 0")
    x = torch.empty((n, 1, steps, 3), dtype=torch.float64, device=device)
    status = torch.empty((n, 1), dtype=torch.int32, device=device)
    if n:
        cols = (ctypes.c_int32 * len(_PHYSICS_COLUMNS))(*_PHYSICS_COLUMNS)
        tgrid = torch.from_numpy(np.ascontiguousarray(t, dtype=np.float64)).to(device)
        with torch.cuda.device(device):
            _native.call("bcnf_resimulate", rows, True, 1, n, NCOL, cols, None, tgrid, steps, float(dt),
                         bool(break_on_impact), 1e-10, 1e-10, 1_000_000, x, None, status, _native.stream_handle(device))
    return x[:, 0], status[:, 0]


def _camera_inputs(rows_host: np.ndarray, cand: np.ndarray, frames: int, ratio, fov_horizontal, device):
    """What the camera kernels take for the candidates `cand` with rows `rows_host`: the cameras exactly as
    render_device builds them from the returned dict (get_cams_position, camera_basis on the host in float64)."""
    n, nc = rows_host.shape[0], 2
    cam_pos = R.get_cams_position(rows_host[:, COLUMNS["cam_radian_array"]], rows_host[:, COLUMNS["cam_radius"]],
                                  rows_host[:, COLUMNS["cam_heights"]])
    basis = R.camera_basis(cam_pos, rows_host[:, COLUMNS["cam_angles"]])
    ph_edges, th_edges = R.bin_edges(ratio, fov_horizontal)
    dev = lambda a, dt=np.float64: torch.from_numpy(np.ascontiguousarray(a, dtype=dt)).to(device)  # noqa: E731
    cam_index = torch.arange(n * nc, dtype=torch.int32, device=device)[:, None].expand(n * nc, frames).contiguous()
    sigma = dev(rows_host[:, COLUMNS["r"]] / R.COVERAGE)[:, None, None].expand(n, nc, frames).contiguous()
    # frame (cam, t) of candidate c: c nc frames + cam frames + t, below 2^32 (candidate_limit); the kernel reads uint32
    frame_index = cand.astype(np.int64)[:, None] * (nc * frames) + np.arange(nc * frames, dtype=np.int64)[None]
    frame_index = dev(frame_index.astype(np.uint32).view(np.int32), np.int32)
    return cam_index, sigma, dev(cam_pos), dev(basis), n * nc, dev(ph_edges), dev(th_edges), frame_index


def _ball(traj):
    n, frames = traj.shape[0], traj.shape[1]
    return traj[:, None].expand(n, 2, frames, 3).contiguous()


def lit_frames_device(traj, rows_host, cand, ratio=(16, 9), fov_horizontal=70.0, seed=DEFAULT_SEED, n_samples=5000,
                      device=None):
    """n_in (n, 2, frames) int32 of the frames of candidates `cand`: one launch of bcnf_render_lit."""
    device = _device(device)
    n, frames = traj.shape[0], traj.shape[1]
    n_in = torch.empty((n, 2, frames), dtype=torch.int32, device=device)
    if n * frames:
        cam_index, sigma, cam_pos, basis, ncams, ph, th, frame_index = _camera_inputs(
            rows_host, np.asarray(cand), frames, ratio, fov_horizontal, device)
        with torch.cuda.device(device):
            _native.call("bcnf_render_lit", _ball(traj), cam_index, sigma, n * 2 * frames, cam_pos, basis, ncams, ph, th,
                         int(n_samples), int(seed) & (2**64 - 1), 0, 0, frame_index, n_in,
                         _native.stream_handle(device))
    return n_in


def _videos_device(traj, rows_host, cand, ratio, fov_horizontal, seed, device):
    n, frames = traj.shape[0], traj.shape[1]
    videos = torch.empty((n, 2, frames, R.HEIGHT, R.WIDTH), dtype=torch.float32, device=device)
    if n * frames:
        cam_index, sigma, cam_pos, basis, ncams, ph, th, frame_index = _camera_inputs(
            rows_host, np.asarray(cand), frames, ratio, fov_horizontal, device)
        with torch.cuda.device(device):
            _native.call("bcnf_render_frames_at", _ball(traj), cam_index, sigma, n * 2 * frames, cam_pos, basis, ncams,
                         ph, th, 5000, int(seed) & (2**64 - 1), 0, frame_index, videos, False, None, None,
                         _native.stream_handle(device))
    return videos


def generate_data_device(config_file, n=100, output_type="parameters", dt=1 / 30, T=4, ratio=(16, 9),
                         fov_horizontal=70.0, cam1_radian=0.0, num_cams=2, break_on_impact=True, do_filter=True,
                         verbose=False, *, seed=DEFAULT_SEED, first_candidate=0, chunk=4096, device=None,
                         return_stats=False):
    """generate_data with the dict's values as device tensors: float64 parameters ((n,), the camera arrays (n, 2)) and
    trajectories (n, len(arange(0, T, dt)), 3), float32 videos (n, 2, frames, 90, 160). With return_stats also
    {'candidates', 'runaway', 'start_underground', 'distance', 'visibility', 'trajectory_not_ok', 'accepted'}: the
    candidates examined up to the last accepted one, the reference's four rejection counters over them, the examined
    candidates whose trajectory status was not OK, and the accepted candidates' indices (int64 numpy)."""
    n, first_candidate, chunk = int(n), int(first_candidate), int(chunk)
    _check_arguments(output_type, num_cams, ratio, n, first_candidate, chunk)
    config = load_data_config(config_file)
    slot_tables(config, num_cams)                 # the config's errors, before anything runs
    device = _device(device)
    frames = len(time_grid(T, dt))
    limit = candidate_limit(num_cams, frames)
    acc_rows, acc_traj, acc_cand, codes_all, not_ok_all = [], [], [], [], []
    have, c0 = 0, first_candidate
    while have < n:
        if c0 >= limit:
            raise ValueError(f"candidate {c0} is beyond 2^32 / (num_cams * frames) = {limit}: its frames have no index "
                             f"in the camera's draw rule")
        cnt = min(chunk, limit - c0)
        rows, _, _, code = sample_candidates_device(config, seed, c0, cnt, cam1_radian, do_filter, device=device)
        code_h = code.cpu().numpy().copy()
        pending = np.nonzero(code_h == PENDING)[0]
        pend_d = torch.from_numpy(pending).to(device)
        rows_p = rows[pend_d].contiguous()
        traj, status = _simulate(rows_p, T, dt, break_on_impact, device)
        not_ok = np.zeros(cnt, dtype=bool)
        not_ok[pending] = status.cpu().numpy() != STATUS_OK
        rows_h = rows_p.cpu().numpy()
        if do_filter:
            n_in = lit_frames_device(traj, rows_h, c0 + pending, ratio, fov_horizontal, seed, device=device)
            lit = (n_in > 0).sum((1, 2)).cpu().numpy()
            ok = accept_visibility(lit, num_cams * frames, rows_h[:, COL_U_VISIBILITY])
            code_h[pending[~ok]] = VISIBILITY
        else:
            ok = np.ones(len(pending), dtype=bool)
        keep = np.nonzero(ok)[0][:n - have]
        examined = cnt if have + len(keep) < n else int(pending[keep[-1]]) + 1
        keep_d = torch.from_numpy(keep).to(device)
        acc_rows.append(rows_p[keep_d])
        acc_traj.append(traj[keep_d])
        acc_cand.append(c0 + pending[keep])
        codes_all.append(code_h[:examined])
        not_ok_all.append(not_ok[:examined])
        have += len(keep)
        c0 += cnt
        if verbose:
            print(f"generate_data: {have} / {n} accepted after {c0 - first_candidate} candidates")
    rows = torch.cat(acc_rows) if acc_rows else torch.empty((0, NCOL), dtype=torch.float64, device=device)
    traj = torch.cat(acc_traj) if acc_traj else torch.empty((0, frames, 3), dtype=torch.float64, device=device)
    cand = np.concatenate(acc_cand) if acc_cand else np.zeros(0, dtype=np.int64)
    videos = None
    if output_type == "videos":
        videos = _videos_device(traj, rows.cpu().numpy(), cand, ratio, fov_horizontal, seed, device)
    data = assemble(rows, traj, videos, output_type)
    if not return_stats:
        return data
    stats = _stats(np.concatenate(codes_all) if codes_all else np.zeros(0, dtype=np.int32),
                   np.concatenate(not_ok_all) if not_ok_all else np.zeros(0, dtype=bool))
    stats["accepted"] = cand.astype(np.int64)
    return data, stats


def generate_data(config_file, n=100, output_type="parameters", dt=1 / 30, T=4, ratio=(16, 9), fov_horizontal=70.0,
                  cam1_radian=0.0, num_cams=2, break_on_impact=True, do_filter=True, verbose=False, *,
                  seed=DEFAULT_SEED, first_candidate=0, chunk=4096, device=None, return_stats=False):
    """sampling.py:287-410 with the reference's signature and result: a dict with the reference's keys in its order
    (then 'videos' / 'trajectories' as output_type asks), every value a numpy array stacked over the n accepted
    samples = np.array(data[key]) of the reference: float64 (n,) parameters (g_x and g_y the integer zeros the
    reference stores), cam_radian_array (n, 2) with cam1_radian prepended, cam_angles / cam_heights (n, 2),
    trajectories (n, len(arange(0, T, dt)), 3) float64, videos (n, 2, frames, 90, 160) (float32: the float64 quotient
    count / n_in rounded once). Keyword-only extras: seed, first_candidate (resume a sequence), chunk (candidates per
    launch; the result does not depend on it), device, return_stats (see generate_data_device)."""
    out = generate_data_device(config_file, n, output_type, dt, T, ratio, fov_horizontal, cam1_radian, num_cams,
                               break_on_impact, do_filter, verbose, seed=seed, first_candidate=first_candidate,
                               chunk=chunk, device=device, return_stats=return_stats)
    data, stats = out if return_stats else (out, None)
    host = {key: value.cpu().numpy() for key, value in data.items()}
    for key in ("g_x", "g_y"):
        host[key] = host[key].astype(np.int64)
    return (host, stats) if return_stats else host
