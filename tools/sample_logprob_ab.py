"""A/B of posterior draws WITH their log-density, in ONE process, routes alternated:

    timeout -k 10 600 python tools/sample_logprob_ab.py [--rounds 3] [--calls 20] [--out profiles/sample_logprob_ab.txt]

Shape: BASELINE.json configs[4] -- FC_small, 500 draws x 1024 conditions (512k rows), the model and conditions of
bench.py's sample workload. Routes:
  (A) draw(...)                          -- as before: k_hp + k_inverse_mfma<7, PERM>
  (B) draw(..., return_log_prob=True)    -- k_hp + k_inverse_mfma<7, PERM, LDJ>: the density out of the same launch
  (C) draw(...) then model.log_prob over the 512k tiled rows -- the only route before (feature network on tiled
      conditions, per-row projection, every tanh recomputed by k_forward)
plus one FC_large-shaped line (wide family, [526] * 5, C = 1360, 2 blocks) at 64 draws x 256 conditions for A and B.
Timing: 150 ms of the same calls as spin-up, then per round and route HIP events around `calls` (>= 20) back-to-back
calls ended by a synchronise; medians over the rounds, min / max alongside. z is drawn once and passed in, so every
route inverts the same rows. The first failure ends the run: nothing more is started on the device."""
import argparse
import os
import statistics
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)


def fc_large_proxy():
    from bcnf_amd import CondRealNVP_v2
    cfg = {"global": {"parameter_selection": [f"p{i}" for i in range(19)]},
           "model": {"kwargs": {"size": 19, "nested_sizes": [526] * 5, "n_conditions": 1360, "n_blocks": 2,
                                "dropout": 0.407, "act_norm": True}},
           "feature_networks": [{"type": "ConcatenateCondition", "kwargs": {"input_size": None, "output_size": 90}},
                                {"type": "FullyConnected", "kwargs": {"sizes": [90, 1360], "dropout": 0.0}}]}
    torch.manual_seed(2024_03_25)
    return CondRealNVP_v2.from_config(cfg)


def timed(fn, calls):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(calls):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / calls


def ab(model, n, cond, routes, rounds, calls, log):
    from bcnf_amd.sampling import draw
    nc = cond.shape[0]
    z = torch.randn(n * nc, model.size, device=cond.device, generator=torch.Generator(cond.device).manual_seed(1))
    tiled = cond.repeat(n, *([1] * (cond.dim() - 1))) if "C" in routes else None

    def route_c():
        y = draw(model, n, cond, z=z)
        return model.log_prob(y.view(-1, model.size), tiled)

    fns = {"A": lambda: draw(model, n, cond, z=z),
           "B": lambda: draw(model, n, cond, z=z, return_log_prob=True),
           "C": route_c}
    with torch.no_grad(), model.fused.reuse_pack():
        # the three routes agree before anything is timed
        ya, (yb, lpb) = fns["A"](), fns["B"]()
        assert torch.equal(ya, yb), "draws differ between the plain and the log-density launch"
        if "C" in routes:
            lpc = fns["C"]()
            err = float((lpb.reshape(-1) - lpc).abs().max())
            log(f"  max |log_prob(B) - log_prob(C)| = {err:.3e} over {lpc.numel()} rows")
        t_end = time.perf_counter() + 0.15                       # spin-up on the same kernels
        while time.perf_counter() < t_end:
            for r in routes:
                fns[r]()
        torch.cuda.synchronize()
        times = {r: [] for r in routes}
        for _ in range(rounds):
            for r in routes:
                times[r].append(timed(fns[r], calls))
    med = {r: statistics.median(t) for r, t in times.items()}
    for r in routes:
        log(f"  route {r}: {med[r]:.4f} ms per call (min {min(times[r]):.4f}, max {max(times[r]):.4f}; "
            f"{n * nc / med[r] / 1e3:.1f} M draws/s)")
    return med


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--calls", type=int, default=20)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "sample_logprob_ab.txt"))
    args = ap.parse_args()
    import bench
    from bcnf_amd import CondRealNVP_v2
    dev = torch.device("cuda")
    lines = []

    def log(s):
        print(s, flush=True)
        lines.append(s)

    log(f"sample_logprob_ab: {torch.cuda.get_device_name(0)}, rounds {args.rounds}, calls per timing {args.calls}")
    torch.manual_seed(2024_03_25)
    m = CondRealNVP_v2.from_config(bench.FC_SMALL).to(dev).eval()
    cond = torch.randn(1024, 30, 3, generator=torch.Generator().manual_seed(3)).to(dev)
    log("FC_small, 500 draws x 1024 conditions (configs[4]):")
    med = ab(m, 500, cond, ("A", "B", "C"), args.rounds, args.calls, log)
    log(f"  B/A = {med['B'] / med['A']:.4f}   B/C = {med['B'] / med['C']:.4f}")
    del m
    torch.cuda.empty_cache()
    w = fc_large_proxy().to(dev).eval()
    condw = torch.randn(256, 30, 3, generator=torch.Generator().manual_seed(4)).to(dev)
    log("FC_large-shaped proxy ([526] * 5, C = 1360, 2 blocks), 64 draws x 256 conditions (wide family):")
    medw = ab(w, 64, condw, ("A", "B"), args.rounds, args.calls, log)
    log(f"  B/A = {medw['B'] / medw['A']:.4f}")
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")
    print("wrote", args.out)


if __name__ == "__main__":
    main()
