"""Time generate_data on the GPU (bcnf_amd.generate.generate_data_device) and the reference's generate_data on the host.

    python tools/generate_ab.py [--trajectories 100000] [--videos 2048] [--chunk 65536] [--rounds 7]
                                [--out profiles/generate_ab.txt]
    python tools/generate_ab.py --reference path/to/reference/src [--accepted 50] [--out profiles/generate_ab.txt]

Arguments of both: configs/data/config.yaml's priors (tests/golden/data_config.yaml), T = 2.0, dt = 0.067 (30 frames x 2
cameras), do_filter, break_on_impact.

Device: the device is spun up, one call warms the kernels, then `rounds` (>= 7) calls of generate_data_device, each
ended by a synchronise, wall time; medians and min / max. The share of each launch is the sum of event pairs around
every call of the four entry points during one further run (events serialise nothing here: the pipeline is
stream-ordered and the host waits for each chunk's reject codes anyway).

Reference (--reference, CPU only, appends to --out): the reference's own generate_data, numpy's global stream seeded
with 2024_03_25, dynaconf replaced by a stub that returns the YAML as a dict, wall time for `accepted` samples, once."""
import argparse
import os
import statistics
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)
CONFIG = os.path.join(ROOT, "tests", "golden", "data_config.yaml")
T, DT = 2.0, 0.067
LAUNCHES = ("bcnf_sample_candidates", "bcnf_resimulate", "bcnf_render_lit", "bcnf_render_frames_at")


def reference(src, accepted, out):
    stub = tempfile.mkdtemp(prefix="bcnf_stub_")
    os.makedirs(os.path.join(stub, "dynaconf"))
    with open(os.path.join(stub, "dynaconf", "__init__.py"), "w") as f:
        f.write("import yaml\n\n\nclass Dynaconf(dict):\n    def __init__(self, settings_files=(), **k):\n"
                "        with open(settings_files[0]) as f:\n            super().__init__(yaml.safe_load(f))\n")
    sys.dont_write_bytecode = True
    sys.path[:0] = [stub, src]
    import matplotlib
    matplotlib.use("Agg")
    import bcnf.simulation.sampling as sampling
    np.random.seed(2024_03_25)
    calls = [0]
    real = sampling.sample_ballistic_parameters

    def counted(*a, **k):
        calls[0] += 1
        return real(*a, **k)

    sampling.sample_ballistic_parameters = counted
    lines = []
    for output_type in ("trajectories", "videos"):
        calls[0] = 0
        t0 = time.perf_counter()
        sampling.generate_data(config_file=CONFIG, n=accepted, output_type=output_type, dt=DT, T=T, do_filter=True)
        dt = time.perf_counter() - t0
        lines.append(f"  reference generate_data on one host core, output_type '{output_type}': {accepted} accepted of "
                     f"{calls[0]} candidates in {dt:.1f} s = {accepted / dt:.2f} accepted/s "
                     f"(acceptance {accepted / calls[0]:.3f})")
    text = "\n".join(lines) + "\n"
    print(text)
    with open(out, "a") as f:
        f.write(text)


def summary(ts):
    return f"median {statistics.median(ts):9.2f}  min {min(ts):9.2f}  max {max(ts):9.2f}"


def device(args):
    import torch
    from bcnf_amd import _native as N
    from bcnf_amd import generate as G
    dev = torch.device("cuda")
    a = torch.randn(4096, 4096, device=dev)
    t_end = time.perf_counter() + 1.5                     # spin the device up
    while time.perf_counter() < t_end:
        (a @ a).sum().item()

    def run(n, output_type, chunk):
        out = G.generate_data_device(CONFIG, n=n, output_type=output_type, dt=DT, T=T, chunk=chunk, device=dev,
                                     return_stats=True)
        torch.cuda.synchronize()
        return out

    def shares(n, output_type, chunk):
        events, real = [], N.call

        def call(name, *a):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            real(name, *a)
            e1.record()
            events.append((name, e0, e1))

        N.call = call
        try:
            t0 = time.perf_counter()
            run(n, output_type, chunk)
            wall = (time.perf_counter() - t0) * 1e3
        finally:
            N.call = real
        ms = {name: 0.0 for name in LAUNCHES}
        count = {name: 0 for name in LAUNCHES}
        for name, e0, e1 in events:
            ms[name] += e0.elapsed_time(e1)
            count[name] += 1
        return wall, ms, count

    lines = [f"device: {torch.cuda.get_device_name(0)}; priors of configs/data/config.yaml, T = {T}, dt = {DT} (30 frames x "
             f"2 cameras), do_filter, break_on_impact; ms per call of generate_data_device, {args.rounds} rounds after one "
             f"warm call"]
    for n, output_type, chunk in ((args.trajectories, "trajectories", args.chunk),
                                  (args.videos, "videos", min(args.chunk, 8192))):
        _, stats = run(n, output_type, chunk)
        ts = []
        for _ in range(args.rounds):
            t0 = time.perf_counter()
            run(n, output_type, chunk)
            ts.append((time.perf_counter() - t0) * 1e3)
        med = statistics.median(ts)
        wall, ms, count = shares(n, output_type, chunk)
        rejected = {k: stats[k] for k in ("runaway", "start_underground", "distance", "visibility")}
        lines += [f"  {n} accepted, output_type '{output_type}', chunk {chunk}: {summary(ts)}   "
                  f"{n / med * 1e3:12.0f} accepted/s",
                  f"    candidates examined {stats['candidates']} (acceptance {n / stats['candidates']:.3f}); rejected "
                  f"{rejected}; trajectories not OK {stats['trajectory_not_ok']}",
                  "    launches (events, one instrumented run of %.2f ms): " % wall + "; ".join(
                      f"{name} x{count[name]} {ms[name]:.2f} ms ({ms[name] / wall:.1%})" for name in LAUNCHES) +
                  f"; host and torch {wall - sum(ms.values()):.2f} ms ({(wall - sum(ms.values())) / wall:.1%})"]
    lines.append("k_candidates: 143 VGPRs, 106 SGPRs, 12,808 B LDS, no scratch, 64 threads; k_render<float, lit>: 69 VGPRs, "
                 "2,024 B LDS, no scratch, 512 threads (hipcc -Rpass-analysis=kernel-resource-usage)")
    text = "\n".join(lines) + "\n"
    print(text)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(text)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--trajectories", type=int, default=100_000)
    ap.add_argument("--videos", type=int, default=2048)
    ap.add_argument("--chunk", type=int, default=65536)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--reference", default=None)
    ap.add_argument("--accepted", type=int, default=50)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "generate_ab.txt"))
    args = ap.parse_args()
    if args.reference:
        return reference(args.reference, args.accepted, args.out)
    if args.rounds < 7:
        ap.error("--rounds must be at least 7")
    device(args)


if __name__ == "__main__":
    main()
