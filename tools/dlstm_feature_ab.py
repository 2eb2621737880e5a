"""A/B of the DualDomainLSTM feature network's fused LSTM layer kernels (bcnf_lstm.hip) against the same modules forced
onto torch's own nn.LSTM (MIOpen's RNN path), in ONE process, arms alternating.

    python tools/dlstm_feature_ab.py [--iters 30] [--rounds 9] [--out profiles/dlstm_feature_ab.txt]

Arms (class attribute, bcnf_amd/feature_network.py): VerboseLSTM.fused -- per layer the input projection on the
library's GEMMs and ONE recurrence launch for both directions each way -- against the single-layer nn.LSTM modules.
The `fc` Linear and the pooling run the same code in both arms, the dropouts are nn.Dropout in both.

    torch   nn.LSTM modules        fused   projection GEMMs + bcnf_lstm_forward / bcnf_lstm_backward

Shapes: the reference's configs/runs/nll/t_DLSTM_large (H = 128, 4 bidirectional layers, S = 30 and 16 rfft bins ->
C = 512; flow H = [512] x 4, 32 blocks) and t_DLSTM_xsmall (H = 16, 1 bidirectional layer -> C = 32; flow [32] x 5, 32
blocks), B = 256, train mode. Three timings per arm: forward + backward of the feature network alone, once as eager
launches (host-bound: the GPU waits for Python between kernels) and once as a captured graph's replay (the device time
of the same work; skipped for both arms when one of them cannot be captured), and the whole TrainStep (captured graph
replay). The device is spun up and every arm warmed (graphs captured) before any timed region; a timed region is
`iters` iterations ended by a synchronise; the arms alternate for `rounds` (>= 7) rounds; medians and min / max are
reported. Before timing, the fused arm's h and gradients are compared with the torch arm's at the timed size (train mode
with the Dropout modules switched off, since torch's GPU LSTM has no eval-mode backward)."""
import argparse
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
B = 256
ARMS = {"torch": False, "fused": True}
def _shape(nested, hidden, layers):
    return dict(
        model={"size": 21, "nested_sizes": nested, "n_conditions": nested[0], "n_blocks": 32, "dropout": 0.5,
               "act_norm": True, "layer": "Linear", "activation": "GELU", "random_state": 2024_03_25},
        feature={"type": "DualDomainLSTM",
                 "kwargs": {"input_size": 3, "hidden_size": hidden, "num_layers": layers, "dropout": 0.5,
                            "bidirectional": True, "fc_sizes": [nested[0]], "fc_dropout": 0.5, "pooling": "mean"}},
        hybrid_weight=0.0)


SHAPES = {"t_DLSTM_large": _shape([512] * 4, 128, 4), "t_DLSTM_xsmall": _shape([32] * 5, 16, 1)}


def set_arm(arm):
    from bcnf_amd import feature_network as F
    F.VerboseLSTM.fused = ARMS[arm]


def build(s):
    from bcnf_amd import CondRealNVP_v2
    cfg = {"global": {"parameter_selection": NAMES}, "model": {"kwargs": dict(s["model"])},
           "feature_networks": [{"type": "ConcatenateCondition", "kwargs": {"input_size": None, "output_size": 3}},
                                s["feature"]]}
    torch.manual_seed(2024_03_25)
    return CondRealNVP_v2.from_config(cfg).to("cuda")


def feature_pass(net, traj, gh):
    for p in net.parameters():
        p.grad = None
    h = net(traj)
    h.backward(gh)
    return h


def capture_feature(net, traj, gh):
    """forward + backward of the feature network as one HIP graph (warmed up on a side stream first)."""
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        for _ in range(3):
            feature_pass(net, traj, gh)
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        feature_pass(net, traj, gh)
    return graph


def timed(fn, iters):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(iters):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / iters * 1e3


def agreement(net, traj, gh):
    """max |fused - torch| of h, relative to max |h|, and over all parameter gradients, relative to the largest
    gradient entry."""
    drops = [m for m in net.modules() if isinstance(m, torch.nn.Dropout)]
    for m in drops:
        m.eval()
    res = {}
    for arm in ("torch", "fused"):
        set_arm(arm)
        h = feature_pass(net, traj, gh)
        res[arm] = [h.detach().clone()] + [p.grad.clone() for p in net.parameters()]
    for m in drops:
        m.train()
    diff = [float((a - b).abs().max()) for a, b in zip(res["fused"], res["torch"])]
    scale = [float(b.abs().max()) for b in res["torch"]]
    return diff[0] / scale[0], max(diff[1:]) / max(scale[1:])


def summary(ts):
    return f"median {statistics.median(ts):8.4f}  min {min(ts):8.4f}  max {max(ts):8.4f}"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=30)
    ap.add_argument("--rounds", type=int, default=9)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "dlstm_feature_ab.txt"))
    args = ap.parse_args()
    if args.rounds < 7:
        ap.error("--rounds must be at least 7")
    from bcnf_amd.train import TrainStep
    dev = torch.device("cuda")
    a = torch.randn(4096, 4096, device=dev)
    t_end = time.perf_counter() + 1.5                     # spin the device up
    while time.perf_counter() < t_end:
        (a @ a).sum().item()
    gen = torch.Generator().manual_seed(3)
    y = torch.randn(B, 21, generator=gen).to(dev)
    traj = (5.0 * torch.randn(B, 30, 3, generator=gen)).to(dev)
    lines = [f"device: {torch.cuda.get_device_name(0)}; B = {B}, train mode; ms per iteration, {args.iters} iterations "
             f"per timed region, {args.rounds} alternating rounds"]
    for name, s in SHAPES.items():
        model = build(s).train()
        net = model.feature_network_stack
        gh = torch.randn(B, s["model"]["n_conditions"], generator=gen).to(dev)
        dh, dg = agreement(net, traj, gh)
        lines.append(f"\n{name}: fused vs torch arm at this size (dropouts off): max rel |dh| {dh:.2e}, "
                     f"gradients {dg:.2e}")
        steps, graphs = {}, {}
        for arm in ARMS:                                  # one model + captured TrainStep per arm
            set_arm(arm)
            try:
                graphs[arm] = capture_feature(net, traj, gh)
            except RuntimeError as e:                     # an arm that cannot be captured: no graph timing at all
                graphs[arm] = None
                lines.append(f"  arm {arm}: the feature pass could not be captured ({str(e).splitlines()[0][:120]})")
                torch.cuda.synchronize()
            st = TrainStep(build(s).train(), lr=2e-4, hybrid_weight=s["hybrid_weight"])
            st.step(y, traj)                              # warm-up steps + capture + first replay
            steps[arm] = st
            for _ in range(3):
                feature_pass(net, traj, gh)
        t_feat = {arm: [] for arm in ARMS}
        t_graph = {arm: [] for arm in ARMS}
        t_step = {arm: [] for arm in ARMS}
        for _ in range(args.rounds):
            for arm in ARMS:
                set_arm(arm)
                t_feat[arm].append(timed(lambda: feature_pass(net, traj, gh), args.iters))
            for arm in ARMS:
                if all(g is not None for g in graphs.values()):
                    t_graph[arm].append(timed(graphs[arm].replay, args.iters))
            for arm in ARMS:
                t_step[arm].append(timed(lambda: steps[arm].step_async(y, traj), args.iters))
        for what, ts in (("feature network forward + backward (eager launches)", t_feat),
                         ("feature network forward + backward (graph replay)", t_graph),
                         ("TrainStep (graph replay)", t_step)):
            if not ts["torch"]:
                continue
            lines.append(f"  {what}")
            base = statistics.median(ts["torch"])
            for arm in ARMS:
                lines.append(f"    {arm:6s} {summary(ts[arm])}   x{base / statistics.median(ts[arm]):.3f} vs torch")
        del steps, graphs, model
        torch.cuda.empty_cache()
    set_arm("fused")
    text = "\n".join(lines) + "\n"
    print(text)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(text)


if __name__ == "__main__":
    main()
