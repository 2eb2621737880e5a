"""A/B of the hybrid (NLL + prediction-head MSE) training step: TrainStep.fuse_hybrid False (the generic route: torch
nn.Linear + MSELoss + autograd, and in run_epoch one replay and one host sync per batch) against True (model.hybrid_loss:
the head kernels, one autograd node, multi-step graphs), in ONE process, arms interleaved.

    python tools/hybrid_step_ab.py [--steps 200] [--repeats 3] [--out profiles/hybrid_step_ab.json]

Shapes: the reference's configs/runs/hybrid/t_FC_small_hybrid (B = 256, the config's batch, and 4096) and
t_FC_large_hybrid (B = 256 and 2048). Each arm is timed as the per-step loop (step_epoch per batch, one host sync per
step) and as run_epoch; device-resident pools, the device spun up and every arm warmed (graphs captured) before any
timed region, >= `steps` timed steps per arm ended by a synchronise, `repeats` interleaved repetitions; medians and
min / max are reported. The head kernels are timed alone with HIP events and set against their algorithmic bytes
(forward 4 B K + the weights; backward 4 B K read + 8 B K for the dL/dh read-modify-write + the weights) as a fraction
of 8 TB/s HBM -- the bound they would meet if they ran at memory speed, not a claim that they do."""
import argparse
import json
import os
import statistics
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

NAMES = ['x0_x', 'x0_y', 'x0_z', 'v0_x', 'v0_y', 'v0_z', 'g_x', 'g_y', 'g_z', 'w_x', 'w_y', 'w_z', 'b', 'm',
         'a_x', 'a_y', 'a_z', 'r', 'A', 'Cd', 'rho']
SHAPES = {
    "t_FC_small_hybrid": dict(nested=[128] * 3, C=128, fc=[60, 136, 136, 136, 136, 128], batches=[256, 4096]),
    "t_FC_large_hybrid": dict(nested=[512] * 4, C=512, fc=[60, 896, 896, 896, 896, 512], batches=[256, 2048]),
}
HBM_BYTES_PER_S = 8e12
POOL_ROWS = 8192


def config(s):
    return {
        "global": {"parameter_selection": NAMES},
        "model": {"kwargs": {"size": 21, "nested_sizes": s["nested"], "n_conditions": s["C"], "n_blocks": 32,
                             "dropout": 0.5, "act_norm": True, "layer": "Linear", "activation": "GELU",
                             "random_state": 2024_03_25, "hybrid": True}},
        "feature_networks": [
            {"type": "ConcatenateCondition", "kwargs": {"input_size": None, "output_size": 60}},
            {"type": "FullyConnected", "kwargs": {"sizes": s["fc"], "dropout": 0.5}},
        ],
    }


def make_arm(s, B, steps, fuse, pools, order):
    from bcnf_amd import CondRealNVP_v2
    from bcnf_amd.train import TrainStep
    torch.manual_seed(2024_03_25)
    m = CondRealNVP_v2.from_config(config(s)).to("cuda").train()
    m.fused.set_seed(7)
    st = TrainStep(m, lr=2e-4, hybrid_weight=1.0)
    st.fuse_hybrid = fuse
    st.set_pool(*pools)
    st.set_epoch(order, B)
    st.prepare_epoch(steps)
    return st


def run_arm(st, form, steps):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    if form == "loop":
        for _ in range(steps):
            last = st.step_epoch()
    else:
        last = st.run_epoch()[-1]
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / steps * 1e3, last


def head_kernel_times(B, K, D, iters=50):
    """us per launch of the head forward and of the backward (dW + dbias + accumulating dx), HIP events around
    `iters` back-to-back launches."""
    from bcnf_amd import fused as F
    gen = torch.Generator().manual_seed(1)
    h = torch.randn(B, K, generator=gen).cuda()
    W = (torch.randn(D, K, generator=gen) / K ** 0.5).cuda()
    b = torch.zeros(D).cuda()
    y = torch.randn(B, D, generator=gen).cuda()
    work = F.head_workspace(B, K, D, h.device)
    dW, db, dh = torch.empty_like(W), torch.empty_like(b), torch.zeros_like(h)
    calls = {"forward": lambda: F.launch_head_forward(h, W, b, y, work),
             "backward": lambda: F.launch_head_backward(h, W, work, None, 1.0, D, dW, db, dh, True)}
    out = {}
    for name, fn in calls.items():
        fn()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(iters):
            fn()
        e1.record()
        torch.cuda.synchronize()
        out[name] = e0.elapsed_time(e1) * 1e3 / iters
    nbytes = {"forward": 4 * B * K + 4 * D * K, "backward": 12 * B * K + 4 * D * K}
    return {k: {"us": out[k], "algorithmic_bytes": nbytes[k],
                "fraction_of_8TBps_if_hbm_bound": nbytes[k] / (out[k] * 1e-6) / HBM_BYTES_PER_S} for k in out}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "hybrid_step_ab.json"))
    args = ap.parse_args()
    dev = torch.device("cuda")
    a = torch.randn(4096, 4096, device=dev)
    t_end = time.perf_counter() + 1.5                     # spin the device up
    while time.perf_counter() < t_end:
        (a @ a).sum().item()
    gen = torch.Generator().manual_seed(3)
    pools = (torch.randn(POOL_ROWS, 21, generator=gen).to(dev), torch.randn(POOL_ROWS, 20, 3, generator=gen).to(dev))
    rows = []
    for cname, s in SHAPES.items():
        for B in s["batches"]:
            order = torch.randint(0, POOL_ROWS, (args.steps * B,), generator=gen).to(dev)
            arms = {}
            for form in ("loop", "run_epoch"):
                for fuse in (False, True):
                    st = make_arm(s, B, args.steps, fuse, pools, order)
                    run_arm(st, form, args.steps)                 # warm: every graph captured, every shape seen
                    arms[(form, fuse)] = st
            times = {k: [] for k in arms}
            last = {}
            for _ in range(args.repeats):
                for k, st in arms.items():
                    ms, v = run_arm(st, k[0], args.steps)
                    times[k].append(ms)
                    last[k] = v
            row = {"config": cname, "batch": B, "steps_per_timing": args.steps, "repeats": args.repeats, "arms": {}}
            for (form, fuse), ts in times.items():
                med = statistics.median(ts)
                row["arms"][f"{form}/{'fused' if fuse else 'unfused'}"] = {
                    "ms_per_step_median": med, "ms_per_step_min": min(ts), "ms_per_step_max": max(ts),
                    "samples_per_s": B / med * 1e3, "last_logged": list(last[(form, fuse)])}
            row["head_kernels"] = head_kernel_times(B, s["C"], 21)
            rows.append(row)
            print(json.dumps(row), flush=True)
            del arms
            torch.cuda.empty_cache()
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump({"device": torch.cuda.get_device_name(0), "rows": rows}, f, indent=1)
    print("wrote", args.out)


if __name__ == "__main__":
    main()
