"""A/B of the CNN feature network's fused convolution-block kernels (bcnf_conv.hip) against the same module forced
onto torch's own Conv2d / ReLU / Dropout / MaxPool2d (MIOpen), in ONE process, arms alternating.

    python tools/cnn_feature_ab.py [--iters 10] [--rounds 9] [--out profiles/cnn_feature_ab.txt]

Arms (class attribute, bcnf_amd/cnn.py): CNN.fused -- each Conv2d -> ReLU -> Dropout -> MaxPool2d group as ONE launch
each way -- against the torch modules. `final_layer` runs the same code in both arms.

    torch   the nn modules         fused   bcnf_conv_block_forward / bcnf_conv_block_backward

Shapes: the CNNs of the reference's configs/runs/dev/videos_CNN_LSTM_large (channels 1 -> 8 -> 16 -> 32, kernels
8 / 5 / 3, dropout 0.5) and videos_double_CNN_LSTM_large (1 -> 5 -> 10 -> 15, kernels 3 / 3 / 5, dropout 0.25), both
output_size_lin = 1000 on 90 x 160 frames, B = 32 videos of 2 cameras x 30 frames (1920 images), train mode; the flow
is the configs' ([526] x 5, 26 blocks) on [ConcatenateCondition, CNN, LSTM(1000 -> 212 x 2 layers, bidirectional,
-> 1360, pool_dim=1)] without the camera-parameter tail, since TrainStep takes one condition. Three timings per arm:
forward + backward of the CNN alone, once as eager launches and once as a captured graph's replay (skipped for both
arms when one of them cannot be captured), and the whole TrainStep (captured graph replay). The device is spun up and
every arm warmed (graphs captured) before any timed region; a timed region is `iters` iterations ended by a
synchronise; the arms alternate for `rounds` (>= 7) rounds; medians and min / max are reported. Before timing, the
fused arm's output and gradients are compared with the torch arm's at the timed size, Dropout modules switched off."""
import argparse
import os
import statistics
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

NAMES = ['x0_x', 'x0_y', 'x0_z', 'v0_x', 'v0_y', 'v0_z', 'g', 'w_x', 'w_y', 'w_z', 'b', 'm', 'a_x', 'a_y', 'a_z', 'r',
         'A', 'Cd', 'rho']
B, CAMS, FRAMES, IMAGE = 32, 2, 30, [90, 160]
ARMS = {"torch": False, "fused": True}


def _shape(channels, kernels, dropout):
    return {"type": "CNN", "kwargs": {"hidden_channels": channels, "kernel_sizes": kernels, "strides": [1, 1, 1],
                                      "dropout_prob": dropout, "image_input_size": IMAGE, "output_size_lin": 1000,
                                      "output_size": 1000}}


SHAPES = {"videos_CNN_LSTM_large": _shape([8, 16, 32], [8, 5, 3], 0.5),
          "videos_double_CNN_LSTM_large": _shape([5, 10, 15], [3, 3, 5], 0.25)}


def set_arm(arm):
    from bcnf_amd import cnn
    cnn.CNN.fused = ARMS[arm]


def build(feature):
    from bcnf_amd import CondRealNVP_v2
    cfg = {"global": {"parameter_selection": NAMES},
           "model": {"kwargs": {"size": 19, "nested_sizes": [526] * 5, "n_conditions": 1360, "n_blocks": 26,
                                "dropout": 0.407, "act_norm": True}},
           "feature_networks": [{"type": "ConcatenateCondition", "kwargs": {"input_size": None, "output_size": IMAGE}},
                                feature,
                                {"type": "LSTM", "kwargs": {"input_size": 1000, "hidden_size": 212,
                                                            "output_size": 1360, "num_layers": 2, "dropout": 0.111,
                                                            "bidirectional": True, "pooling": "mean",
                                                            "pool_dim": 1}}]}
    torch.manual_seed(2024_03_25)
    return CondRealNVP_v2.from_config(cfg).to("cuda")


def feature_pass(net, videos, gh):
    for p in net.parameters():
        p.grad = None
    h = net(videos)
    h.backward(gh)
    return h


def capture_feature(net, videos, gh):
    """forward + backward of the CNN as one HIP graph (warmed up on a side stream first)."""
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        for _ in range(3):
            feature_pass(net, videos, gh)
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        feature_pass(net, videos, gh)
    return graph


def timed(fn, iters):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(iters):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / iters * 1e3


def agreement(net, videos, gh):
    """max |fused - torch| of the output, relative to its largest entry, and over all parameter gradients, relative
    to the largest gradient entry."""
    drops = [m for m in net.modules() if isinstance(m, torch.nn.Dropout)]
    for m in drops:
        m.eval()
    res = {}
    for arm in ("torch", "fused"):
        set_arm(arm)
        h = feature_pass(net, videos, gh)
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
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--rounds", type=int, default=9)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "cnn_feature_ab.txt"))
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
    y = torch.randn(B, 19, generator=gen).to(dev)
    videos = torch.rand(B, CAMS, FRAMES, *IMAGE, generator=gen).to(dev)
    lines = [f"device: {torch.cuda.get_device_name(0)}; B = {B} x {CAMS} cameras x {FRAMES} frames of "
             f"{IMAGE[0]} x {IMAGE[1]}, train mode; ms per iteration, {args.iters} iterations per timed region, "
             f"{args.rounds} alternating rounds"]
    for name, feature in SHAPES.items():
        model = build(feature).train()
        net = model.feature_network_stack.feature_networks[1]
        gh = torch.randn(B, FRAMES, 1000, generator=gen).to(dev)
        dh, dg = agreement(net, videos, gh)
        lines.append(f"\n{name}: fused vs torch arm at this size (dropouts off): max rel |dh| {dh:.2e}, "
                     f"gradients {dg:.2e}")
        steps, graphs = {}, {}
        for arm in ARMS:                                  # one model + captured TrainStep per arm
            set_arm(arm)
            try:
                graphs[arm] = capture_feature(net, videos, gh)
            except RuntimeError as e:                     # an arm that cannot be captured: no graph timing at all
                graphs[arm] = None
                lines.append(f"  arm {arm}: the CNN pass could not be captured ({str(e).splitlines()[0][:120]})")
                torch.cuda.synchronize()
            st = TrainStep(build(feature).train(), lr=2e-4)
            st.step(y, videos)                            # warm-up steps + capture + first replay
            steps[arm] = st
            for _ in range(3):
                feature_pass(net, videos, gh)
        t_feat = {arm: [] for arm in ARMS}
        t_graph = {arm: [] for arm in ARMS}
        t_step = {arm: [] for arm in ARMS}
        for _ in range(args.rounds):
            for arm in ARMS:
                set_arm(arm)
                t_feat[arm].append(timed(lambda: feature_pass(net, videos, gh), args.iters))
            for arm in ARMS:
                if all(g is not None for g in graphs.values()):
                    t_graph[arm].append(timed(graphs[arm].replay, args.iters))
            for arm in ARMS:
                t_step[arm].append(timed(lambda: steps[arm].step_async(y, videos), args.iters))
        for what, ts in (("CNN forward + backward (eager launches)", t_feat),
                         ("CNN forward + backward (graph replay)", t_graph),
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
