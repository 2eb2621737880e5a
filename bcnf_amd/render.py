"""The camera of the videos_* configs (psaegert/bcnf src/bcnf/simulation/camera.py) on the GPU.

The reference renders a video frame by frame on the host: `camera` (camera.py:74-150) draws 5000 Gaussian points around
the ball, projects them onto the camera's two screen axes with two arctan2 calls, fills a 160 x 90 np.histogram2d,
normalises it and returns np.flipud(vals.T); `record_trajectory` (camera.py:30-71) loops that over the frames and
`generate_data` over the two cameras of a sample (sampling.py:366-368). Here ONE launch of `bcnf_render_frames`
(bcnf_amd/csrc/bcnf_render.hip) renders every frame of a batch, one workgroup per frame, fp64 geometry.

Same semantics behind the same names:
  * `camera_basis`: focus = (0, 0, cam_pos_z), cam_dir = rotate_vector(normalise(focus - cam_pos), viewing_angle),
    cam_orthogonal_z = rotate_vector(cam_dir, 90), cam_orthogonal = cross(cam_dir, cam_orthogonal_z), with
    rotate_vector through spherical coordinates (camera.py:8-27), float64 on the host, bit-identical to the reference;
  * `get_cams_position` (sampling.py:124-131) is bug-compatible: its loop unpacks the two ARRAYS, not pairs, so camera 0
    is (radiant = radiants[0], height = radiants[1]) and camera 1 is (radiant = heights[0], height = heights[1]); any
    other camera count raises the ValueError the tuple unpacking raises;
  * the histogram follows np.histogram2d: np.linspace edges in float64, half-open bins with the last edge included,
    samples outside dropped; the image is row 89 - th_bin, column ph_bin, count / (in-range count), zeros when empty.

The random stream is the kernel's own (the reference uses numpy's global np.random.normal, which no kernel can follow):
`standard_normals` is the normative statement of the draw rule -- Philox4x32-10 of (sample, frame, offset) keyed by the
seed, 32-bit words to uniforms strictly inside (0, 1), Box-Muller in float64 -- and `render_host` is the same renderer in
numpy (np.histogram2d itself): the CPU path, and the partner of the reference in tests/golden/make_golden_render.py,
where the reference's own camera() is fed these draws.
"""
from __future__ import annotations

import numpy as np
import torch

from . import _native

HEIGHT, WIDTH = 90, 160            # include/bcnf_amd.h BCNF_RENDER_HEIGHT / BCNF_RENDER_WIDTH
COVERAGE = 1.644854                # camera.py:113: "a std of 1.644854 covers 90%"
DEFAULT_SEED = 2024_03_25
_KEY_TAG = 0xC0000000              # include/bcnf_amd.h: the render draws' key (seed high half ^ tag)

_M0, _M1 = np.uint64(0xD2511F53), np.uint64(0xCD9E8D57)
_W0, _W1 = np.uint64(0x9E3779B9), np.uint64(0xBB67AE85)
_U32, _S32 = np.uint64(0xFFFFFFFF), np.uint64(32)
TWO_PI = 6.283185307179586


def philox4x32_10(c0, c1, c2, c3, k0, k1):
    """Philox4x32-10 (Salmon et al. 2011) on uint32-valued arrays of broadcastable shapes: four uint64 arrays."""
    c0, c1, c2, c3, k0, k1 = (np.asarray(v, dtype=np.uint64) & _U32 for v in (c0, c1, c2, c3, k0, k1))
    for _ in range(10):
        p0, p1 = _M0 * c0, _M1 * c2
        c0, c1, c2, c3 = (p1 >> _S32) ^ c1 ^ k0, p1 & _U32, (p0 >> _S32) ^ c3 ^ k1, p0 & _U32
        k0, k1 = (k0 + _W0) & _U32, (k1 + _W1) & _U32
    return c0, c1, c2, c3


def standard_normals(seed: int, offset: int, frame, n_samples: int) -> np.ndarray:
    """The three standard normals of samples 0 .. n_samples - 1 of frame `frame` (a frame's index is first_frame + its
    position in the call): float64 (n_samples, 3), or (..., n_samples, 3) for an array of frames.

    Sample s draws (w0, w1, w2, w3) = Philox4x32-10 with counter (s, frame, offset low half, offset high half) and key
    (seed low half, seed high half ^ 0xC0000000); u_i = (w_i + 0.5) 2^-32; z = (sqrt(-2 ln u0) cos(2 pi u1),
    sqrt(-2 ln u0) sin(2 pi u1), sqrt(-2 ln u2) cos(2 pi u3)) with 2 pi = 6.283185307179586, all in float64."""
    seed, offset = int(seed) & (2**64 - 1), int(offset) & (2**64 - 1)
    frame = np.asarray(frame, dtype=np.int64)
    if frame.size and (frame.min() < 0 or frame.max() >= 2**32):
        raise ValueError("frame indices lie in [0, 2^32)")
    s = np.arange(int(n_samples), dtype=np.uint64)
    w = philox4x32_10(s, frame.astype(np.uint64)[..., None], offset & 0xFFFFFFFF, offset >> 32, seed & 0xFFFFFFFF,
                      ((seed >> 32) ^ _KEY_TAG) & 0xFFFFFFFF)
    shape = frame.shape + (int(n_samples),)
    u = [(np.broadcast_to(v, shape).astype(np.float64) + 0.5) * 2.0 ** -32 for v in w]
    r0, r1 = np.sqrt(-2.0 * np.log(u[0])), np.sqrt(-2.0 * np.log(u[2]))
    t0, t1 = TWO_PI * u[1], TWO_PI * u[3]
    return np.stack([r0 * np.cos(t0), r0 * np.sin(t0), r1 * np.cos(t1)], axis=-1)


# ---- camera geometry (host, float64) -----------------------------------------------------------------------------

def _norm3(v):
    """np.linalg.norm of 3-vectors along the last axis, bit for bit what the reference's 1-D call gives: that call is
    sqrt(dot(v, v)) with BLAS's dot, whose fused multiply-adds round differently from the sum of squares an axis
    reduction (or einsum) computes -- one vector in seven differs in the last bit. So the same 1-D call runs per vector
    (a batch has B x ncam of them); everything else in the basis is element-wise and vectorises bit-identically."""
    flat = v.reshape(-1, v.shape[-1])
    return np.array([np.linalg.norm(row) for row in flat], dtype=np.float64).reshape(v.shape[:-1])


def rotate_vector(vector, angle_degrees=45):
    """camera.py:8-27 vectorised over leading axes: through spherical coordinates, theta -= angle."""
    vector = np.asarray(vector, dtype=np.float64)
    angle_radians = np.asarray(angle_degrees, dtype=np.float64) * np.pi / 180
    r = _norm3(vector)
    theta = np.arccos(vector[..., 2] / r)
    phi = np.arctan2(vector[..., 1], vector[..., 0])
    theta = theta - angle_radians
    return np.stack([r * np.sin(theta) * np.cos(phi), r * np.sin(theta) * np.sin(phi), r * np.cos(theta)], axis=-1)


def camera_basis(cam_pos, viewing_angle=0.0) -> np.ndarray:
    """(..., 3, 3) float64: rows cam_dir, cam_orthogonal, cam_orthogonal_z of camera.py:91-105 for cam_pos (..., 3) and
    viewing_angle (...) in degrees."""
    cam_pos = np.asarray(cam_pos, dtype=np.float64)
    viewing_angle = np.broadcast_to(np.asarray(viewing_angle, dtype=np.float64), cam_pos.shape[:-1])
    focus = np.zeros_like(cam_pos)
    focus[..., 2] = cam_pos[..., 2]
    d = focus - cam_pos
    cam_dir = rotate_vector(d / _norm3(d)[..., None], viewing_angle)
    cam_orthogonal_z = rotate_vector(cam_dir, 90)
    cam_orthogonal = np.cross(cam_dir, cam_orthogonal_z)
    return np.stack([cam_dir, cam_orthogonal, cam_orthogonal_z], axis=-2)


def get_cams_position(cam_radiants=np.array([0, 0]), cam_circle_radius=25, cam_heights=np.array([1, 1])) -> np.ndarray:
    """sampling.py:124-131, bug for bug: `for cam_radiant, cam_height in (cam_radiants, cam_heights)` unpacks the two
    arrays, so camera 0 = (radiant radiants[0], height radiants[1]) and camera 1 = (radiant heights[0], height
    heights[1]). (..., 2, 3) float64 for radiants / heights (..., 2) and a radius (...); any other camera count raises
    the unpacking's ValueError."""
    cam_radiants = np.asarray(cam_radiants, dtype=np.float64)
    cam_heights = np.asarray(cam_heights, dtype=np.float64)
    radius = np.asarray(cam_circle_radius, dtype=np.float64)
    cams = []
    for pair in (cam_radiants, cam_heights):
        n = pair.shape[-1]
        if n != 2:
            raise ValueError(f"too many values to unpack (expected 2, got {n})" if n > 2 else
                             f"not enough values to unpack (expected 2, got {n})")
        cam_radiant, cam_height = pair[..., 0], pair[..., 1]
        cams.append(np.stack(np.broadcast_arrays(-radius * np.cos(cam_radiant), radius * np.sin(cam_radiant),
                                                 cam_height), axis=-1))
    return np.stack(cams, axis=-2)


def field_of_view(ratio=(16, 9), fov_horizontal=70.0):
    """(phi, theta) half-angles in radians, camera.py:83-88."""
    aspect_ratio = ratio[0] / ratio[1]
    fov_vertical = fov_horizontal / aspect_ratio
    return (fov_horizontal / 2) * (np.pi / 180), (fov_vertical / 2) * (np.pi / 180)


def bin_edges(ratio=(16, 9), fov_horizontal=70.0):
    """The two edge tables np.histogram2d builds for bins = [10 ratio[0], 10 ratio[1]] on [[-phi, phi], [-theta, theta]]."""
    phi, theta = field_of_view(ratio, fov_horizontal)
    return np.linspace(-phi, phi, ratio[0] * 10 + 1), np.linspace(-theta, theta, ratio[1] * 10 + 1)


def _frames(positions, cam_pos, viewing_angles, radius):
    positions = np.asarray(positions, dtype=np.float64)
    cam_pos = np.asarray(cam_pos, dtype=np.float64)
    viewing_angles = np.asarray(viewing_angles, dtype=np.float64)
    radius = np.asarray(radius, dtype=np.float64)
    if positions.ndim != 3 or positions.shape[-1] != 3:
        raise ValueError(f"positions must be (B, T, 3), got {positions.shape}")
    B = positions.shape[0]
    if cam_pos.ndim != 3 or cam_pos.shape[0] != B or cam_pos.shape[-1] != 3:
        raise ValueError(f"cam_pos must be (B, ncam, 3) with B = {B}, got {cam_pos.shape}")
    if viewing_angles.shape != cam_pos.shape[:2] or radius.shape != (B,):
        raise ValueError(f"viewing_angles must be {cam_pos.shape[:2]} and radius ({B},), got {viewing_angles.shape} "
                         f"and {radius.shape}")
    return positions, cam_pos, viewing_angles, radius


def render_host(positions, cam_pos, viewing_angles, radius, ratio=(16, 9), fov_horizontal=70.0, n_samples=5000,
                seed=DEFAULT_SEED, offset=0, first_frame=0, return_counts=False, edge_margin=None):
    """render_device in numpy float64: (B, ncam, T, 10 ratio[1], 10 ratio[0]) float64 images (with return_counts also the
    int32 counts and n_in (B, ncam, T)), frame (b, cam, t) drawing standard_normals(seed, offset, first_frame +
    (b ncam + cam) T + t, n_samples) and binned by np.histogram2d itself.

    edge_margin (radians): additionally returns the list of (b, cam, t, ph, th) of every sample that lies within the
    margin of a bin edge or range edge in either angle -- the samples another correctly rounded implementation may bin
    differently."""
    positions, cam_pos, viewing_angles, radius = _frames(positions, cam_pos, viewing_angles, radius)
    B, T, ncam = positions.shape[0], positions.shape[1], cam_pos.shape[1]
    nph, nth = ratio[0] * 10, ratio[1] * 10
    phi, theta = field_of_view(ratio, fov_horizontal)
    ph_edges, th_edges = bin_edges(ratio, fov_horizontal)
    basis = camera_basis(cam_pos, viewing_angles)
    images = np.zeros((B, ncam, T, nth, nph))
    counts = np.zeros((B, ncam, T, nth, nph), dtype=np.int32)
    n_in = np.zeros((B, ncam, T), dtype=np.int32)
    near = []
    for b in range(B):
        for c in range(ncam):
            cam_dir, cam_orthogonal, cam_orthogonal_z = basis[b, c]
            for t in range(T):
                z = standard_normals(seed, offset, first_frame + (b * ncam + c) * T + t, n_samples)
                samples = positions[b, t] + (radius[b] / COVERAGE) * z
                v = samples - cam_pos[b, c]
                v = v / np.linalg.norm(v, axis=1)[:, None]
                on_dir = np.dot(v, cam_dir)
                ph = np.arctan2(np.dot(v, cam_orthogonal), on_dir)
                th = np.arctan2(np.dot(v, cam_orthogonal_z), on_dir)
                vals = np.histogram2d(ph, th, bins=[nph, nth], range=[[-phi, phi], [-theta, theta]])[0]
                total = np.sum(vals)
                if total:
                    images[b, c, t] = np.flipud((vals / total).T)
                counts[b, c, t] = np.flipud(vals.T).astype(np.int32)
                n_in[b, c, t] = int(total)
                if edge_margin is not None:
                    close = (np.abs(ph[:, None] - ph_edges[None, :]).min(1) <= edge_margin) | \
                            (np.abs(th[:, None] - th_edges[None, :]).min(1) <= edge_margin)
                    # a sample far outside the other angle's range is dropped whichever side of the edge it falls
                    relevant = (ph >= -phi - edge_margin) & (ph <= phi + edge_margin) & \
                               (th >= -theta - edge_margin) & (th <= theta + edge_margin)
                    near += [(b, c, t, float(ph[i]), float(th[i])) for i in np.nonzero(close & relevant)[0]]
    out = (images, counts, n_in) if return_counts else (images,)
    if edge_margin is not None:
        out = out + (near,)
    return out if len(out) > 1 else out[0]


def render_device(positions, cam_pos, viewing_angles, radius, ratio=(16, 9), fov_horizontal=70.0, n_samples=5000,
                  seed=DEFAULT_SEED, offset=0, first_frame=0, dtype=torch.float32, return_counts=False, device=None):
    """(B, ncam, T, 90, 160) images on the device -- the layout np.array(data['videos']) has and CNN.forward takes -- for
    ball positions (B, T, 3), camera positions (B, ncam, 3), viewing angles (B, ncam) in degrees and ball radii (B,)
    (tensors on any device, or numpy). Frame (b, cam, t) has index first_frame + (b ncam + cam) T + t in the draw rule
    (standard_normals). dtype float32 or float64; with return_counts also the int32 counts (the images' shape) and
    n_in (B, ncam, T). One launch of bcnf_render_frames; B = 0 or T = 0 returns empty tensors without one."""
    if device is None:
        device = positions.device if isinstance(positions, torch.Tensor) and positions.is_cuda else torch.device(
            "cuda", torch.cuda.current_device())
    device = torch.device(device)
    if device.type != "cuda":
        raise RuntimeError("bcnf_amd.render_device runs on the HIP device only (render_host is the CPU path); got " +
                           str(device))
    if dtype not in (torch.float32, torch.float64):
        raise ValueError(f"dtype must be torch.float32 or torch.float64, got {dtype}")
    if tuple(ratio) != (WIDTH // 10, HEIGHT // 10):
        raise ValueError(f"the kernel renders {HEIGHT} x {WIDTH} frames (ratio (16, 9)); got ratio {tuple(ratio)}")
    to_np = lambda v: v.detach().cpu().numpy() if isinstance(v, torch.Tensor) else v  # noqa: E731
    positions_t = positions if isinstance(positions, torch.Tensor) else None
    cam_np, ang_np, rad_np = to_np(cam_pos), to_np(viewing_angles), to_np(radius)
    if positions_t is None:
        pos_np, cam_np, ang_np, rad_np = _frames(positions, cam_np, ang_np, rad_np)
        positions_t = torch.from_numpy(np.ascontiguousarray(pos_np))
    else:     # the positions may be large and on the device already: only the small camera arrays visit the host
        _, cam_np, ang_np, rad_np = _frames(np.empty(tuple(positions_t.shape)), cam_np, ang_np, rad_np)
    B, T, ncam = positions_t.shape[0], positions_t.shape[1], cam_np.shape[1]
    F = B * ncam * T
    if first_frame < 0 or first_frame + F > 2**32:
        raise ValueError("frame indices lie in [0, 2^32)")
    shape = (B, ncam, T, HEIGHT, WIDTH)
    images = torch.empty(shape, dtype=dtype, device=device)
    counts = torch.empty(shape, dtype=torch.int32, device=device) if return_counts else None
    n_in = torch.empty((B, ncam, T), dtype=torch.int32, device=device) if return_counts else None
    if F:
        ph_edges, th_edges = bin_edges(ratio, fov_horizontal)
        basis = camera_basis(cam_np, ang_np)
        ball = positions_t.to(device=device, dtype=torch.float64)[:, None].expand(B, ncam, T, 3).contiguous()
        cam_index = torch.arange(B * ncam, dtype=torch.int32)[:, None].expand(B * ncam, T).contiguous().to(device)
        sigma = torch.from_numpy(rad_np / COVERAGE)[:, None, None].expand(B, ncam, T).contiguous().to(device)
        dev = lambda a: torch.from_numpy(np.ascontiguousarray(a, dtype=np.float64)).to(device)  # noqa: E731
        with torch.cuda.device(device):
            _native.call("bcnf_render_frames", ball, cam_index, sigma, F, dev(cam_np), dev(basis), B * ncam,
                         dev(ph_edges), dev(th_edges), int(n_samples), int(seed) & (2**64 - 1),
                         int(offset) & (2**64 - 1), int(first_frame), images, dtype == torch.float64, counts, n_in,
                         _native.stream_handle(device))
    if return_counts:
        return images, counts, n_in
    return images


def _render_one(trajectory, ratio, fov_horizontal, cam_pos, radius, viewing_angle, seed, offset, first_frame, device):
    """(T, H, W) float64 numpy: on the device when there is one (and the ratio is the kernel's), else render_host."""
    args = (np.asarray(trajectory, dtype=np.float64)[None], np.asarray(cam_pos, dtype=np.float64)[None, None],
            np.asarray([[viewing_angle]], dtype=np.float64), np.asarray([radius], dtype=np.float64))
    if device is None:
        device = "cuda" if torch.cuda.is_available() else "cpu"
    if torch.device(device).type == "cuda":
        return render_device(*args, ratio, fov_horizontal, seed=seed, offset=offset, first_frame=first_frame,
                             dtype=torch.float64, device=device)[0, 0].cpu().numpy()
    return render_host(*args, ratio, fov_horizontal, seed=seed, offset=offset, first_frame=first_frame)[0, 0]


def camera(ball_pos=np.array([0, 0, 1.5]), ratio=(16, 9), fov_horizontal=70.0, cam_pos=np.array([-25, 0, 1.5]),
           show_plot=False, radius=0.1143, viewing_angle=0.0, *, seed=DEFAULT_SEED, offset=0, frame=0, device=None):
    """camera.py:74-150: one (10 ratio[1], 10 ratio[0]) float64 frame. The draws are standard_normals(seed, offset,
    frame, 5000). show_plot is accepted for the signature and must be False."""
    if show_plot:
        raise NotImplementedError("bcnf_amd.camera renders the frame only (show_plot is not supported)")
    return _render_one(np.asarray(ball_pos, dtype=np.float64)[None], ratio, fov_horizontal, cam_pos, radius,
                       viewing_angle, seed, offset, frame, device)[0]


def record_trajectory(trajectory=np.array([[0, 0, 0]]), ratio=(16, 9), fov_horizontal=70.0,
                      cam_pos=np.array([-25, 0, 1.5]), make_gif=False, gif_name='trajectory', radius=0.1143,
                      viewing_angle=0.0, *, seed=DEFAULT_SEED, offset=0, first_frame=0, device=None):
    """camera.py:30-71: the (T, 10 ratio[1], 10 ratio[0]) float64 film of a trajectory (T, 3); frame t draws
    standard_normals(seed, offset, first_frame + t, 5000). make_gif defaults to False here and is not supported."""
    if make_gif:
        raise NotImplementedError("bcnf_amd.record_trajectory returns the film only (GIF output is not supported)")
    return _render_one(trajectory, ratio, fov_horizontal, cam_pos, radius, viewing_angle, seed, offset, first_frame,
                       device)


def visibility(videos, n_in=None):
    """The statistic generate_data filters on (sampling.py:370): sum over all cameras and frames / (ncam T), per sample
    (float64 (B,), on the videos' device). A non-empty frame sums to 1 and an empty one to 0, so this is the share of
    frames with n_in > 0 -- taken from n_in (B, ncam, T) when given, else from the frames themselves (a frame is lit
    iff its largest pixel is positive: count / n_in >= 1 / n_samples > 0)."""
    lit = (n_in > 0) if n_in is not None else (torch.as_tensor(videos).flatten(-2).amax(-1) > 0)
    if lit.ndim != 3:
        raise ValueError(f"videos must be (B, ncam, T, H, W) and n_in (B, ncam, T); got a lit map of {tuple(lit.shape)}")
    return lit.sum((1, 2)).to(torch.float64) / (lit.shape[1] * lit.shape[2])
