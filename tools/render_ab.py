"""Time the camera kernel (bcnf_render_frames, bcnf_amd/csrc/bcnf_render.hip) on one batch of the videos_* configs'
shape beside the same renderer in numpy on the host's cores.

    python tools/render_ab.py [--iters 10] [--rounds 9] [--procs 16] [--out profiles/render_ab.txt]

Shape: B = 32 samples x 2 cameras x 30 frames (1920 frames of 90 x 160), 5000 samples per frame, float32 images;
trajectories from bcnf_amd.data.simulate (T = 2.0, dt = 0.067), cameras from the priors of configs/data/config.yaml.

    host     bcnf_amd.render.render_host (numpy float64, np.histogram2d), the 32 samples spread over `procs` worker
             processes (forked before the GPU is touched), wall time of the whole batch, once
    device   bcnf_amd.render.render_device: the whole call (host-side camera bases, uploads, the launch), wall time,
             and the kernel alone between two events, raw entry point on resident inputs

The device is spun up first; a timed region is `iters` calls ended by a synchronise (the event pair brackets `iters`
launches); `rounds` (>= 7) regions; medians and min / max. Before timing, the device's integer counts are compared
with the host's."""
import argparse
import multiprocessing
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

B, CAMS, N_SAMPLES = 32, 2, 5000


def inputs():
    from bcnf_amd.data import PARAMETERS, sample_cameras, simulate
    from bcnf_amd.render import get_cams_position
    y, traj = simulate(B, 2024_03_25, T=2.0, dt=0.067)
    cam_radian, cam_radius, cam_angles, cam_heights = sample_cameras(B, 2024_03_26)
    return (traj.astype(np.float64), get_cams_position(cam_radian, cam_radius, cam_heights), cam_angles,
            y[:, PARAMETERS.index('r')].astype(np.float64))


def _host_one(job):
    from bcnf_amd.render import render_host
    b, pos, cam, ang, rad = job
    frames = CAMS * pos.shape[1]
    return render_host(pos, cam, ang, rad, n_samples=N_SAMPLES, first_frame=b * frames, return_counts=True)


def summary(ts):
    return f"median {statistics.median(ts):9.4f}  min {min(ts):9.4f}  max {max(ts):9.4f}"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--rounds", type=int, default=9)
    ap.add_argument("--procs", type=int, default=16)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "render_ab.txt"))
    args = ap.parse_args()
    if args.rounds < 7:
        ap.error("--rounds must be at least 7")
    pos, cam, ang, rad = inputs()
    T = pos.shape[1]
    jobs = [(b, pos[b:b + 1], cam[b:b + 1], ang[b:b + 1], rad[b:b + 1]) for b in range(B)]
    with multiprocessing.get_context("fork").Pool(args.procs) as pool:      # before the GPU is initialised
        pool.map(_host_one, jobs[:args.procs])                              # workers imported and warm
        t0 = time.perf_counter()
        host = pool.map(_host_one, jobs, chunksize=1)
        t_host = (time.perf_counter() - t0) * 1e3
    counts_h = np.concatenate([h[1] for h in host])
    n_h = np.concatenate([h[2] for h in host])

    import torch
    from bcnf_amd import _native as N
    from bcnf_amd import render as R
    dev = torch.device("cuda")
    a = torch.randn(4096, 4096, device=dev)
    t_end = time.perf_counter() + 1.5                     # spin the device up
    while time.perf_counter() < t_end:
        (a @ a).sum().item()
    img, counts, n_in = R.render_device(pos, cam, ang, rad, n_samples=N_SAMPLES, return_counts=True, device=dev)
    diff = int((counts.cpu().numpy() != counts_h).sum())
    lit = int((n_in > 0).sum())

    def timed(fn):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(args.iters):
            fn()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) / args.iters * 1e3

    pos_d = torch.from_numpy(pos).to(dev)
    call = lambda: R.render_device(pos_d, cam, ang, rad, n_samples=N_SAMPLES, device=dev)  # noqa: E731
    F = B * CAMS * T
    d = lambda v: torch.from_numpy(np.ascontiguousarray(v, dtype=np.float64)).to(dev)  # noqa: E731
    ball = pos_d[:, None].expand(B, CAMS, T, 3).contiguous()
    cam_index = torch.arange(B * CAMS, dtype=torch.int32)[:, None].expand(B * CAMS, T).contiguous().to(dev)
    sigma = d(rad / R.COVERAGE)[:, None, None].expand(B, CAMS, T).contiguous()
    ph, th = R.bin_edges()
    cam_d, basis_d, ph_d, th_d = d(cam), d(R.camera_basis(cam, ang)), d(ph), d(th)
    out = torch.empty((F, 90, 160), dtype=torch.float32, device=dev)
    stream = N.stream_handle(dev)
    kernel = lambda: N.call("bcnf_render_frames", ball, cam_index, sigma, F, cam_d, basis_d, B * CAMS, ph_d, th_d,  # noqa: E731
                            N_SAMPLES, R.DEFAULT_SEED, 0, 0, out, False, None, None, stream)

    def timed_events(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        e0.record()
        for _ in range(args.iters):
            fn()
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1) / args.iters

    for _ in range(3):
        call()
        kernel()
    assert torch.equal(out.view(B, CAMS, T, 90, 160), img)
    t_call, t_kernel = [], []
    for _ in range(args.rounds):
        t_call.append(timed(call))
        t_kernel.append(timed_events(kernel))
    k = statistics.median(t_kernel)
    lines = [f"device: {torch.cuda.get_device_name(0)}; B = {B} x {CAMS} cameras x {T} frames = {F} frames of 90 x 160, "
             f"{N_SAMPLES} samples per frame ({F * N_SAMPLES / 1e6:.1f} M samples), float32 images; ms per batch, "
             f"{args.iters} calls per timed region, {args.rounds} rounds",
             f"frames with the ball in view: {lit} of {F}; device counts differing from render_host's: {diff} of "
             f"{counts_h.size} pixels",
             f"  host   render_host on {args.procs} processes (wall, once)   {t_host:10.1f}   "
             f"{F / t_host * 1e3:10.0f} frames/s",
             f"  device render_device, whole call (wall)   {summary(t_call)}   "
             f"{F / statistics.median(t_call) * 1e3:10.0f} frames/s",
             f"  device bcnf_render_frames alone (events)  {summary(t_kernel)}   {F / k * 1e3:10.0f} frames/s",
             f"  kernel vs host: x{t_host / k:.0f}; kernel vs the 13.55 ms TrainStep of videos_double_CNN_LSTM_large: "
             f"{k / 13.55:.3f} of it",
             "k_render<float>: 77 VGPRs, 106 SGPRs, 59,624 B LDS, no scratch, 512 threads, 4 waves / SIMD "
             "(hipcc -Rpass-analysis=kernel-resource-usage)"]
    text = "\n".join(lines) + "\n"
    print(text)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(text)


if __name__ == "__main__":
    main()
