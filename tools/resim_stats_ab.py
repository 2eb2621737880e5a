"""Time the notebook's analysis of the re-simulated positions on the device and on the host, in one process.

    python tools/resim_stats_ab.py [--trajectories 1024] [--draws 1000] [--rounds 7] [--host-rounds 3]
                                   [--out profiles/resim_stats_ab.txt]

Shape: bench.py's resimulation workload (resim_draws(1024, 1000), T = 2, dt = 1/15, break_on_impact), the first draw's
trajectories rounded to float32 as the observation, the notebook's edges np.linspace(-42, 42, 128).

Device: `resimulation_summary` end to end (y_hat resident, numpy results returned: wall time), the peak device memory
of that chunked path, and event pairs around `resimulate_device`, `resimulation_error_device` and `impacts_device` on
the positions of all trajectories at once. Host: what a user does without the kernels: `resimulate()` to a numpy
array, then the notebook's expressions (nanmedian of nanmean; np.where(np.diff(...)) per trajectory, the positions
there and one histogram2d per trajectory). The device is spun up first; medians with min / max; both paths' results
are compared bit for bit."""
import argparse
import os
import statistics
import sys
import time
import types
import warnings

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)
T, DT = 2.0, 1 / 15


def summary(ts):
    return f"median {statistics.median(ts):9.2f}  min {min(ts):9.2f}  max {max(ts):9.2f}"


def notebook(X_resim, X, edges):
    """The notebook's cells on the host array; returns (errors, indices, positions, hists) and the seconds of the two
    parts."""
    t0 = time.perf_counter()
    with warnings.catch_warnings():
        warnings.simplefilter("ignore", RuntimeWarning)
        X_errors = np.nanmedian(np.nanmean((X_resim - X[:, None])**2, axis=3), axis=1)
    t1 = time.perf_counter()
    indices, positions, hists = [], [], []
    for i in range(X_resim.shape[0]):
        impact_indices = np.where(np.diff((X_resim[i, :, :, -1] > 0).astype(int), axis=1) == -1)
        impact_positions = X_resim[i][impact_indices]
        indices.append(impact_indices)
        positions.append(impact_positions)
        hists.append(np.histogram2d(impact_positions[:, 0], impact_positions[:, 1], bins=[edges, edges])[0])
    t2 = time.perf_counter()
    return (X_errors, indices, positions, hists), t1 - t0, t2 - t1


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--trajectories", type=int, default=1024)
    ap.add_argument("--draws", type=int, default=1000)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--host-rounds", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "resim_stats_ab.txt"))
    args = ap.parse_args()
    import torch
    import bench
    from bcnf_amd import resimulation_stats as RS
    from bcnf_amd.resimulation import resimulate, resimulate_device
    from bcnf_amd.utils import ParameterIndexMapping
    dev = torch.device("cuda", 0)
    n, m = args.trajectories, args.draws
    yh, dd = bench.resim_draws(n, m)
    pim = ParameterIndexMapping(bench.FC_SMALL["global"]["parameter_selection"])
    model = types.SimpleNamespace(parameter_index_mapping=pim, device=dev)
    y = torch.from_numpy(yh).to(dev)
    edges = RS.DEFAULT_BINS
    observed = resimulate_device(y[:1], T, DT, dd, pim, break_on_impact=True)[:, 0].cpu().numpy().astype(np.float32)
    steps = observed.shape[1]

    a = torch.randn(4096, 4096, device=dev)
    t_end = time.perf_counter() + 1.5                     # spin the device up
    while time.perf_counter() < t_end:
        (a @ a).sum().item()
    del a

    def device_path():
        return RS.resimulation_summary(model, T, DT, dd, y, observed=observed, break_on_impact=True, bins=edges,
                                       verbose=False)

    dev_res = device_path()                               # warms the kernels
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats(dev)
    base = torch.cuda.memory_allocated(dev)
    t_dev = []
    for _ in range(args.rounds):
        t0 = time.perf_counter()
        device_path()
        t_dev.append((time.perf_counter() - t0) * 1e3)
    peak = torch.cuda.max_memory_allocated(dev)
    chunk = RS.default_chunk_trajectories(m, steps)

    # the launches alone, all trajectories at once, event pairs behind one launch already in the queue
    x = resimulate_device(y, T, DT, dd, pim, break_on_impact=True)
    obs_d = torch.from_numpy(observed).to(dev)
    st = torch.cuda.current_stream(dev)
    kernels = {"resimulate_device": lambda: resimulate_device(y, T, DT, dd, pim, break_on_impact=True),
               "resimulation_error_device": lambda: RS.resimulation_error_device(x, obs_d),
               "impacts_device (with hist)": lambda: RS.impacts_device(x, edges),
               "impacts_device (no hist)": lambda: RS.impacts_device(x)}
    k_ms = {}
    for name, fn in kernels.items():
        fn()
        ts = []
        for _ in range(args.rounds):
            fn()
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(st)
            for _ in range(4):
                fn()
            e1.record(st)
            torch.cuda.synchronize()
            ts.append(e0.elapsed_time(e1) / 4)
        k_ms[name] = ts
    pos_bytes = x.numel() * 8
    del x

    t_res, t_err, t_imp = [], [], []
    for _ in range(args.host_rounds):
        t0 = time.perf_counter()
        xh = resimulate(model, T, DT, dd, y, break_on_impact=True, verbose=False)
        t_res.append((time.perf_counter() - t0) * 1e3)
        host_res, se, si = notebook(xh, observed.astype(np.float64), edges)
        t_err.append(se * 1e3)
        t_imp.append(si * 1e3)
    t_host = [r + e + i for r, e, i in zip(t_res, t_err, t_imp)]
    X_errors, indices, positions, hists = host_res
    same = np.array_equal(dev_res["errors"], X_errors, equal_nan=True)
    for i in range(n):
        draw, s = indices[i]
        same &= int(dev_res["impact_transitions"][i].sum()) == len(draw)
        same &= np.array_equal(dev_res["impact_hist"][i], hists[i])
        which, first = np.unique(draw, return_index=True)
        same &= np.array_equal(dev_res["impact_step"][i, which], s[first])
        same &= np.array_equal(dev_res["impact_position"][i, which], positions[i][first])
    del xh

    med_d, med_h = statistics.median(t_dev), statistics.median(t_host)
    lines = [
        f"device: {torch.cuda.get_device_name(0)}; resim_draws({n}, {m}), T = {T}, dt = 1/15 ({steps} steps), "
        f"break_on_impact, edges linspace(-42, 42, 128); ms; device spun up 1.5 s; device rows {args.rounds} rounds, host "
        f"rows {args.host_rounds} rounds, after one warm call",
        f"  device  resimulation_summary end to end (slices of {chunk} trajectories)   {summary(t_dev)}",
        f"          peak device memory of the chunked path {(peak - base) / 2**20:.1f} MiB above the resident draws "
        f"({base / 2**20:.1f} MiB); one slice's positions {min(chunk, n) * m * steps * 24 / 2**20:.1f} MiB, all "
        f"positions {pos_bytes / 2**20:.1f} MiB",
    ]
    for name, ts in k_ms.items():
        lines.append(f"          launch alone, all {n} trajectories: {name:32s} {summary(ts)}")
    lines += [
        f"  host    resimulate() to numpy + the notebook's expressions                {summary(t_host)}",
        f"          resimulate() (launch + {pos_bytes / 1e6:.0f} MB copy)                             {summary(t_res)}",
        f"          nanmedian(nanmean(...))                                          {summary(t_err)}",
        f"          np.where(np.diff(...)), positions, histogram2d x {n}             {summary(t_imp)}",
        f"  host / device = {med_h / med_d:.1f}; results identical (errors, impact steps, positions, counts, "
        f"histograms): {bool(same)}",
        "k_resim_error<float>: 22 VGPRs, 45 SGPRs, no scratch, 256 threads (1024 above 32 KB), dynamic LDS 8 P x tile "
        "bytes (32 KB at M = 1000); k_resim_impacts: 44 VGPRs, 97 SGPRs, no scratch, 1024 threads, dynamic LDS 65,540 B "
        "at 128 edges (hipcc -Rpass-analysis=kernel-resource-usage)",
    ]
    text = "\n".join(lines) + "\n"
    print(text)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(text)


if __name__ == "__main__":
    main()
