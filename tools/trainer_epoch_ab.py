"""A/B of one training epoch (train + validate) of bcnf_amd.trainer.Trainer's device loop against the literal loop a
user writes without it, in ONE process, arms alternating.

    python tools/trainer_epoch_ab.py [--rounds 9] [--out profiles/trainer_epoch_ab.txt]

Shapes: the reference's configs/runs/hybrid/t_FC_small_hybrid (hybrid_weight 1) and configs/runs/nll/t_FC_small
(hybrid_weight 0): D = 21, nested [128] x 3, 32 blocks, C = 128, FullyConnected [60, 136 x 4, 128], dropout 0.5,
n = 5000 samples, validation_split 0.2 -> 4001 training samples (15 batches of 256 and one of 161) and 999 validation
samples (3 batches of 256 and one of 231).

    trainer   TrainStep.set_epoch + run_epoch (multi-step graphs, one host sync) + step_indexed for the ragged batch,
              then ValidationPass.run (multi-batch graphs + the ragged batch, bcnf_validation_stats, one host sync)
    literal   per batch: TrainStep.step_indexed (captured step, one host sync each; the ragged batch eager), then per
              validation batch: eager model.forward under no_grad, torch reductions (inn_nll_loss, MSELoss, z.mean(0),
              z.std(0)) and three .item() -- Trainer._validate_batch as written

Both arms own a model (same initial weights) and draw the same epoch orders. Protocol (tools/dlstm_feature_ab.py): the
device is spun up, both arms run warm-up epochs (every graph captured) before any timed region; a timed region is one
epoch ended by its own host syncs; the arms alternate for `rounds` (>= 7) rounds; medians with min .. max are
reported, for the epoch and for its two halves. Also reported: the statistics kernel alone (a captured graph of 64
launches, per launch) and the cost of one TrainStep.set_lr recapture (the epoch after set_lr against the median
epoch)."""
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
N, SPLIT, BATCH = 5000, 0.2, 256
SHAPES = {"t_FC_small_hybrid": 1.0, "t_FC_small": 0.0}


def build(hybrid):
    from bcnf_amd import CondRealNVP_v2
    cfg = {"global": {"parameter_selection": NAMES},
           "model": {"kwargs": {"size": 21, "nested_sizes": [128] * 3, "n_conditions": 128, "n_blocks": 32,
                                "dropout": 0.5, "act_norm": True, "hybrid": hybrid, "random_state": 2024_03_25}},
           "feature_networks": [{"type": "ConcatenateCondition", "kwargs": {"input_size": None, "output_size": 60}},
                                {"type": "FullyConnected",
                                 "kwargs": {"sizes": [60, 136, 136, 136, 136, 128], "dropout": 0.5}}]}
    torch.manual_seed(2024_03_25)
    m = CondRealNVP_v2.from_config(cfg).to("cuda")
    m.fused.set_seed(5)
    return m


class TrainerArm:
    def __init__(self, model, y, cond, n_train, w):
        from bcnf_amd.train import TrainStep
        from bcnf_amd.validate import ValidationPass
        self.model, self.nw = model, n_train // BATCH
        self.ts = TrainStep(model, lr=2e-4, hybrid_weight=w)
        self.ts.set_pool(y[:n_train].contiguous(), cond[:n_train].contiguous())
        self.vp = ValidationPass(model, hybrid_weight=w)
        self.vp.set_pool(y[n_train:].contiguous(), cond[n_train:].contiguous(), BATCH)

    def train(self, order):
        self.model.train()
        self.ts.set_epoch(order[:self.nw * BATCH], BATCH)
        out = self.ts.run_epoch()
        if order.numel() > self.nw * BATCH:
            out.append(self.ts.step_indexed(order[self.nw * BATCH:]))
        return out

    def validate(self):
        return self.vp.run()[:3]


class LiteralArm:
    def __init__(self, model, y, cond, n_train, w):
        from bcnf_amd.train import TrainStep
        self.model, self.w = model, w
        self.ts = TrainStep(model, lr=2e-4, hybrid_weight=w)
        self.ts.set_pool(y[:n_train].contiguous(), cond[:n_train].contiguous())
        self.yv, self.cv = y[n_train:].contiguous(), cond[n_train:].contiguous()
        self.mse = torch.nn.MSELoss()

    def train(self, order):
        self.model.train()
        return [self.ts.step_indexed(order[lo:lo + BATCH]) for lo in range(0, order.numel(), BATCH)]

    def validate(self):
        from bcnf_amd.utils import inn_nll_loss
        m, w = self.model, self.w
        m.eval()
        sums, nb = [0.0, 0.0, 0.0], 0
        with torch.no_grad():
            for lo in range(0, self.yv.shape[0], BATCH):
                y, c = self.yv[lo:lo + BATCH], self.cv[lo:lo + BATCH]
                z, h = m.forward(y, c, log_det_J=True, return_features=True)
                mse = self.mse(m.prediction_head(h), y) if w > 0 else torch.tensor(0.0)
                nll = inn_nll_loss(z, m.log_det_J)
                loss = (nll + mse.to(nll.device) * w) / (1 + w)
                for i, v in enumerate((loss.item(), nll.item(), mse.item())):
                    sums[i] += v
                self.z_mean, self.z_std = z.mean(dim=0), z.std(dim=0)
                nb += 1
        m.train()
        return tuple(s / nb for s in sums)


def timed_epoch(arm, order):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    arm.train(order)
    t1 = time.perf_counter()
    arm.validate()
    torch.cuda.synchronize()
    t2 = time.perf_counter()
    return (t2 - t0) * 1e3, (t1 - t0) * 1e3, (t2 - t1) * 1e3


def summary(ts):
    return f"median {statistics.median(ts):8.3f}  min {min(ts):8.3f}  max {max(ts):8.3f}"


def stats_kernel_us(D, hybrid):
    from bcnf_amd.validate import validation_stats
    gen = torch.Generator().manual_seed(1)
    z, ldj = torch.randn(BATCH, D, generator=gen).cuda(), torch.randn(BATCH, generator=gen).cuda()
    pred, y = (torch.randn(BATCH, D, generator=gen).cuda() for _ in range(2)) if hybrid else (None, None)
    row = torch.zeros((1, 4 + 2 * D), device="cuda")
    acc = torch.zeros(3, dtype=torch.float64, device="cuda")
    validation_stats(z, ldj, pred, y, 1.0 if hybrid else 0.0, row=row, epoch_sum=acc)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        for _ in range(64):
            validation_stats(z, ldj, pred, y, 1.0 if hybrid else 0.0, row=row, epoch_sum=acc)
    ts = []
    for _ in range(12):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        g.replay()
        torch.cuda.synchronize()
        ts.append((time.perf_counter() - t0) * 1e6 / 64)
    return ts[2:]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=9)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "trainer_epoch_ab.txt"))
    args = ap.parse_args()
    rounds = max(7, args.rounds)
    from bcnf_amd.trainer import split_sizes
    n_train, n_val = split_sizes(N, SPLIT)
    lines = [f"trainer_epoch_ab: one epoch = {n_train} training samples ({-(-n_train // BATCH)} batches of {BATCH}) + "
             f"{n_val} validation samples ({-(-n_val // BATCH)} batches); {rounds} rounds, arms alternating; ms",
             f"device: {torch.cuda.get_device_name(0)}"]
    x = torch.randn(4096, 4096, device="cuda")
    t_end = time.perf_counter() + 1.5                      # spin the device up
    while time.perf_counter() < t_end:
        (x @ x).sum().item()
    del x
    gen = torch.Generator().manual_seed(7)
    y = torch.randn(N, 21, generator=gen).cuda()
    cond = (2.0 * torch.randn(N, 20, 3, generator=gen)).cuda()
    og = torch.Generator().manual_seed(11)
    for shape, w in SHAPES.items():
        arms = {"literal": LiteralArm(build(w > 0), y, cond, n_train, w),
                "trainer": TrainerArm(build(w > 0), y, cond, n_train, w)}
        for _ in range(3):                                  # warm-up: every graph captured, allocators settled
            order = torch.randperm(n_train, generator=og).cuda()
            vals = {k: (a.train(order), a.validate()) for k, a in arms.items()}
        agree = max(abs(a - b) for a, b in zip(vals["literal"][1], vals["trainer"][1]))
        same = vals["literal"][0] == vals["trainer"][0]
        ts = {k: [] for k in arms}
        for r in range(rounds):
            order = torch.randperm(n_train, generator=og).cuda()
            for k in (("literal", "trainer") if r % 2 == 0 else ("trainer", "literal")):
                ts[k].append(timed_epoch(arms[k], order))
        lines.append(f"\n{shape} (hybrid_weight {w}): training triples of the arms bit-equal: {same}; "
                     f"validation triples agree to {agree:.2e}")
        for part, name in enumerate(("epoch", "  train", "  validate")):
            base = statistics.median([t[part] for t in ts["literal"]])
            for k in ("literal", "trainer"):
                col = [t[part] for t in ts[k]]
                lines.append(f"  {name:10s} {k:8s} {summary(col)}   x{base / statistics.median(col):.3f} vs literal")
        # one set_lr recapture: the epoch after it against the steady epoch
        a = arms["trainer"]
        order = torch.randperm(n_train, generator=og).cuda()
        a.ts.set_lr(1e-4)
        t_re = timed_epoch(a, order)
        steady = statistics.median([t[0] for t in ts["trainer"]])
        lines.append(f"  epoch after set_lr (recapture of the step graphs): {t_re[0]:8.3f} ms = steady {steady:.3f} + "
                     f"{t_re[0] - steady:.3f}")
        ks = stats_kernel_us(21, w > 0)
        lines.append(f"  bcnf_validation_stats alone (B = {BATCH}, D = 21, {'with' if w > 0 else 'no'} pred / y; graph of "
                     f"64 launches, us per launch): {summary(ks)}")
        del arms
    text = "\n".join(lines) + "\n"
    print(text)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(text)


if __name__ == "__main__":
    main()
