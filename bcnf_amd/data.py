"""Synthetic ballistic-trajectory batches: a vectorised restatement of the reference's
simulator so benchmarks run on realistic conditions without the offline-unavailable HF datasets.

* ODE: ballistic_ODE (src/bcnf/simulation/physics.py:7-50):
      dv/dt = g - g rho (4/3) pi r^3 / m - (0.5 b / m) (v^2 v/|v| - w^2 w/|w|) + a
  integrated with classical RK4 (16 sub-steps per frame) on the reference's time grid t = arange(0, T, dt)
  (physics.py:144),
  positions x_i = x_{i-1} + v_i dt (physics.py:150-152), no impact break (configs use break_on_impact False).
* Priors: configs/data/config.yaml (polar x0/v0/w in the xy-plane, gamma g / rho / r / Cd, m).
* y: the 19 parameters of trajectory_FC_small's `parameter_selection`, in that order.
"""
from __future__ import annotations

import numpy as np

PARAMETERS = ['x0_x', 'x0_y', 'x0_z', 'v0_x', 'v0_y', 'v0_z', 'g', 'w_x', 'w_y', 'w_z',
              'b', 'm', 'a_x', 'a_y', 'a_z', 'r', 'A', 'Cd', 'rho']


def _polar(rng, n, std):
    r = np.abs(rng.normal(0.0, std, n))
    phi = rng.uniform(0.0, 2.0 * np.pi, n)
    return r * np.cos(phi), r * np.sin(phi)


def _dvdt(v, g, w, b, m, rho, r, a):
    vn = np.linalg.norm(v, axis=1, keepdims=True)
    wn = np.linalg.norm(w, axis=1, keepdims=True)
    vn = np.where(vn == 0, 1.0, vn)
    wn = np.where(wn == 0, 1.0, wn)
    buoy = g * rho * (4.0 / 3.0) * (np.pi * r ** 3) / m
    drag = (0.5 * b / m) * (v ** 2 * v / vn - w ** 2 * w / wn)
    return g - buoy - drag + a


def simulate(n: int, seed: int = 2024_03_25, T: float = 2.0, dt: float = 0.067, substeps: int = 16):
    """Return (y (n, 19) float32, trajectories (n, len(arange(0,T,dt)), 3) float32)."""
    rng = np.random.Generator(np.random.PCG64(seed))
    x0x, x0y = _polar(rng, n, 20.0)
    x0z = rng.uniform(0.1, 2.5, n)
    v0x, v0y = _polar(rng, n, 15.0)
    v0z = rng.normal(7.0, 5.0, n)
    wx, wy = _polar(rng, n, 3.0)
    wz = rng.normal(0.0, 1.0, n)
    gz = -rng.gamma(9.81, 1.0, n)
    rho = rng.gamma(3.5, 0.35, n)
    r = rng.gamma(1.75, 0.05, n) + 1e-3
    cd = rng.gamma(2.0, 0.1, n)
    m = rng.gamma(2.0, 0.5, n) + 0.05
    A = np.pi * r ** 2
    b = 0.5 * rho * A * cd
    zeros = np.zeros(n)

    g = np.stack([zeros, zeros, gz], 1)
    w = np.stack([wx, wy, wz], 1)
    a = np.stack([zeros, zeros, zeros], 1)
    bb, mm, rr, rh = b[:, None], m[:, None], r[:, None], rho[:, None]

    t = np.arange(0.0, T, dt)
    steps = len(t)
    v = np.stack([v0x, v0y, v0z], 1)
    x = np.stack([x0x, x0y, x0z], 1)
    traj = np.empty((n, steps, 3))
    traj[:, 0] = x
    f = lambda vv: _dvdt(vv, g, w, bb, mm, rr, rh, a)  # noqa: E731
    for i in range(1, steps):
        h = (t[i] - t[i - 1]) / substeps     # odeint is adaptive; fixed RK4 needs sub-steps for
        for _ in range(substeps):            # the stiff light-and-draggy tail of the priors
            k1 = f(v)
            k2 = f(v + 0.5 * h * k1)
            k3 = f(v + 0.5 * h * k2)
            k4 = f(v + h * k3)
            v = v + (h / 6.0) * (k1 + 2 * k2 + 2 * k3 + k4)
        x = x + v * dt
        traj[:, i] = x
    y = np.stack([x0x, x0y, x0z, v0x, v0y, v0z, gz, wx, wy, wz, b, m, zeros, zeros, zeros, r, A, cd, rho], 1)
    return y.astype(np.float32), traj.astype(np.float32)


class DeviceBatches:
    """A device-resident pool of samples served as pre-shuffled batches (the Trainer's DataLoader
    shuffle without its per-sample Python collate: SURVEY §7 'Trainer overheads')."""

    def __init__(self, n_pool: int, batch: int, device, seed: int = 2024_03_25, normalize: bool = True):
        import torch
        y, traj = simulate(n_pool, seed)
        y_t = torch.from_numpy(y)
        tr_t = torch.from_numpy(traj)
        if normalize:   # standardise so the synthetic NLL stays in the reference's training regime
            y_t = (y_t - y_t.mean(0)) / (y_t.std(0) + 1e-6)
            tr_t = (tr_t - tr_t.mean((0, 1))) / (tr_t.std((0, 1)) + 1e-6)
        self.y = y_t.to(device)
        self.traj = tr_t.to(device)
        self.batch = batch
        self.n = n_pool
        self.gen = torch.Generator(device="cpu").manual_seed(seed)
        self._perm = None
        self._pos = 0
        self.device = device

    def next_indices(self):
        import torch
        if self._perm is None or self._pos + self.batch > self.n:
            self._perm = torch.randperm(self.n, generator=self.gen).to(self.device)
            self._pos = 0
        idx = self._perm[self._pos:self._pos + self.batch]
        self._pos += self.batch
        return idx


def sample_cameras(n: int, seed: int = 2024_03_25):
    """The camera parameters of n two-camera samples from the priors of configs/data/config.yaml, as generate_data
    arranges them (sampling.py:245-254, 363): cam_radian (n, 2) = [cam1 at 0, U(0, 2 pi)], cam_radius (n,) ~ Gamma(2.5,
    5), cam_angles (n, 2) ~ Gamma(3, 10) degrees, cam_heights (n, 2) ~ U(0.4, 1.4). float64."""
    rng = np.random.Generator(np.random.PCG64(seed))
    cam_radian = np.stack([np.zeros(n), rng.uniform(0.0, 6.283185307, n)], 1)
    cam_radius = rng.gamma(2.5, 5.0, n)
    cam_angles = rng.gamma(3.0, 10.0, (n, 2))
    cam_heights = rng.uniform(0.4, 1.4, (n, 2))
    return cam_radian, cam_radius, cam_angles, cam_heights


class VideoBatches:
    """A pool of simulated samples served as (y, videos, cam_tail) batches for the videos_* configs: physics parameters
    and trajectories from simulate() (T = 2.0, dt = 0.067: 30 frames), camera parameters from sample_cameras(), the two
    cameras placed by get_cams_position (the reference's, bug for bug) and every frame rendered on the device by
    bcnf_amd.render.render_device.

    videos (batch, 2, 30, 90, 160) float32; cam_tail (batch, 7) float32 = cam_radian (2), cam_radius (1), cam_angles
    (2), cam_heights (2), the order the configs' second condition concatenates them. The pool is rendered once; with
    online=True only the parameters are kept and each batch is rendered when it is served, with `offset` advanced by
    one per batch, so every batch sees fresh camera noise."""

    T, DT, N_CAMS = 2.0, 0.067, 2

    def __init__(self, n_pool: int, batch: int, device, seed: int = 2024_03_25, normalize: bool = True,
                 online: bool = False, n_samples: int = 5000, fov_horizontal: float = 70.0):
        import torch
        from .render import get_cams_position
        y, traj = simulate(n_pool, seed, T=self.T, dt=self.DT)
        cam_radian, cam_radius, cam_angles, cam_heights = sample_cameras(n_pool, seed + 1)
        self.radius = y[:, PARAMETERS.index('r')].astype(np.float64)
        self.cam_pos = get_cams_position(cam_radian, cam_radius, cam_heights)          # (n, 2, 3)
        self.cam_angles = cam_angles
        tail = np.concatenate([cam_radian, cam_radius[:, None], cam_angles, cam_heights], 1).astype(np.float32)
        y_t = torch.from_numpy(y)
        if normalize:
            y_t = (y_t - y_t.mean(0)) / (y_t.std(0) + 1e-6)
        self.device = torch.device(device)
        self.y = y_t.to(self.device)
        self.traj = torch.from_numpy(traj).to(self.device, torch.float64)
        self.cam_tail = torch.from_numpy(tail).to(self.device)
        self.batch, self.n, self.seed, self.online = batch, n_pool, seed, online
        self.n_samples, self.fov_horizontal = n_samples, fov_horizontal
        self.offset = 0
        self.gen = torch.Generator(device="cpu").manual_seed(seed)
        self._perm = None
        self._pos = 0
        self.videos = None if online else self.render(np.arange(n_pool))

    def render(self, rows):
        """float32 videos (len(rows), 2, 30, 90, 160) of pool samples `rows` at the current offset, in ONE launch: the
        sample at position k of `rows` draws with frame indices k * 60 .. k * 60 + 59."""
        import torch
        from .render import render_device
        rows = np.asarray(rows, dtype=np.int64)
        return render_device(self.traj[torch.from_numpy(rows).to(self.device)],self.cam_pos[rows], self.cam_angles[rows], self.radius[rows],
                             fov_horizontal=self.fov_horizontal, n_samples=self.n_samples, seed=self.seed,
                             offset=self.offset, device=self.device)

    def next_indices(self):
        import torch
        if self._perm is None or self._pos + self.batch > self.n:
            self._perm = torch.randperm(self.n, generator=self.gen)
            self._pos = 0
        idx = self._perm[self._pos:self._pos + self.batch]
        self._pos += self.batch
        return idx

    def next_batch(self):
        """(y (batch, 19), videos (batch, 2, 30, 90, 160), cam_tail (batch, 7)) on the device."""
        idx = self.next_indices()
        idx_d = idx.to(self.device)
        if self.online:
            videos = self.render(idx.numpy())
            self.offset += 1
        else:
            videos = self.videos[idx_d]
        return self.y[idx_d], videos, self.cam_tail[idx_d]
