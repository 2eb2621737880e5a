"""GPU tests of bcnf_amd.trainer.Trainer and TrainStep.set_lr: a run of Trainer.train against the literal loop
(tests/trainer_ref.py: one eager TrainStep step per batch with the lr edited through param_groups, _validate_batch in
torch ops) on the recorded model, data and batch orders of tests/golden/g21_trainer.npz, with dropout 0.5.

Training values, final parameters and Adam state are compared bit for bit (the captured epoch equals the eager
per-batch loop, tests/test_gpu_train.py, and ValidationPass draws no masks); validation values at 1e-5, the project's
forward gate: they come from two different reductions (the fp64 statistics kernel against torch's fp32 ones)."""
import numpy as np
import pytest
import torch

from conftest import close, load_golden
from trainer_ref import (BATCH, NAMES, bits_equal, golden_data, golden_model, literal_loop, model_config,
                         train_config)

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def g21():
    return load_golden("g21_trainer.npz")


def _order_fn(g):
    orders = g["orders"]
    return lambda epoch, n_train: torch.from_numpy(orders[epoch % len(orders)][:n_train].copy())


def _wide_model(seed=77):
    from bcnf_amd import CondRealNVP_v2
    from bcnf_amd.wide import WideStack
    torch.manual_seed(3)
    m = CondRealNVP_v2.from_config(model_config(dropout=0.5, D=21, nested=(32,) * 3, C=32, n_blocks=4))
    assert isinstance(m.fused, WideStack)
    m.to("cuda")
    m.fused.set_seed(seed)
    return m


def _pair(g, case):
    """Two identical models (same weights, same dropout seed) and the data of the case."""
    y, cond = golden_data(g)
    if case == "wide":
        a, b = _wide_model(), _wide_model()
        b.load_state_dict(a.state_dict())
        gen = torch.Generator().manual_seed(11)
        y = torch.randn(200, 21, generator=gen).cuda()
        return a, b, y, cond, 0.0
    run = "ii" if case == "hybrid" else "i"
    return golden_model(g, run, dropout=0.5), golden_model(g, run, dropout=0.5), y, cond, float(g[f"{run}/w"])


def _adam_state(ts):
    out = []
    for p in ts.params:
        st = ts.opt.state[p]
        out += [st["exp_avg"], st["exp_avg_sq"], st["step"].float()]
    return out


@pytest.mark.parametrize("case", ["small", "hybrid", "wide"])
def test_trainer_equals_the_literal_loop(g21, case):
    from bcnf_amd import ParameterIndexMapping, Trainer
    ma, mb, y, cond, w = _pair(g21, case)
    # lr 5e-3 with a scheduler that halves after every epoch that does not improve by 1e9: the lr changes after
    # epochs 1, 2 and 3, so every later epoch runs on recaptured graphs
    cfg = train_config(4, 5e-3, dict(patience=0, factor=0.5, threshold=1e9, threshold_mode="abs"))
    tr = Trainer(cfg, ParameterIndexMapping(NAMES[:y.shape[1]]), hybrid_weight=w, data=(y, cond),
                 order_fn=_order_fn(g21))
    assert tr.train(ma) is ma
    h = tr.meta_scheduler
    hl, trains, vals, ts_l = literal_loop(mb, cfg, y, cond, _order_fn(g21), w)
    ph, pl = h.parameter_history, hl.parameter_history
    assert ph["stop_reason"] == pl["stop_reason"] == "max_epochs"
    assert list(ph) == list(pl)
    for k in ("train_loss", "train_loss_nll", "train_loss_mse", "lr", "distance_to_last_best_val_loss"):
        assert ph[k] == pl[k], k                                        # bit-equal training triples, same lr sequence
    assert [v for _, v in ph["lr"]] == [5e-3, 5e-3, 5e-3, 2.5e-3, 1.25e-3]   # first entry twice; halved after epoch 1, 2
    for k in ("val_loss", "val_loss_nll", "val_loss_mse", "z_mean_mean", "z_mean_std", "z_std_mean", "z_std_std",
              "log_det_J"):
        ok, err = close([v for _, v in ph[k]], [v for _, v in pl[k]])
        print(f"{case} {k}: err {err:.3e}")
        assert ok, (k, err)
    if w == 0.0:
        assert all(v == 0.0 for _, v in ph["val_loss_mse"]) and ph["val_loss"] == ph["val_loss_nll"]
    for (n, pa), (_, pb) in zip(ma.named_parameters(), mb.named_parameters()):
        assert bits_equal(pa, pb), n
    for i, (sa, sb) in enumerate(zip(_adam_state(tr.train_step), _adam_state(ts_l))):
        assert bits_equal(sa, sb), i
    assert ma.training and torch.equal(ma.fused.rng_state(), mb.fused.rng_state())
    assert (h.best_val_epoch, ph["stop_reason"]) == (hl.best_val_epoch, pl["stop_reason"])


def test_set_lr_reaches_the_captured_step(g21):
    """Three epochs of two batches; the lr halves after the second. The captured TrainStep with set_lr equals the eager
    one bit for bit; a captured one whose lr is edited through param_groups alone keeps stepping at the old rate."""
    from bcnf_amd.train import TrainStep
    y, cond = golden_data(g21)
    models = [golden_model(g21, "i", dropout=0.5) for _ in range(3)]
    steps = [TrainStep(models[0], lr=1e-2, capture=False), TrainStep(models[1], lr=1e-2),
             TrainStep(models[2], lr=1e-2)]
    for ts in steps:
        ts.set_pool(y[:121].contiguous(), cond[:121].contiguous())
    logged = [[], [], []]
    for epoch in range(3):
        order = torch.from_numpy(g21["orders"][epoch][:96]).cuda()
        for i, ts in enumerate(steps):
            ts.model.train()
            ts.set_epoch(order, BATCH)
            logged[i] += ts.run_epoch()
        if epoch == 1:
            steps[0].set_lr(5e-3)
            steps[1].set_lr(5e-3)
            assert steps[1]._cap is None
            steps[2].opt.param_groups[0]["lr"] = 5e-3
    assert logged[0] == logged[1]
    for (n, pa), (_, pb), (_, pc) in zip(*(m.named_parameters() for m in models)):
        assert bits_equal(pa, pb), n
    for sa, sb in zip(_adam_state(steps[0]), _adam_state(steps[1])):
        assert bits_equal(sa, sb)
    assert torch.equal(models[0].fused.rng_state(), models[1].fused.rng_state())
    assert steps[1].opt.param_groups[0]["lr"] == 5e-3
    assert logged[2][:5] == logged[0][:5] and logged[2] != logged[0]     # the first step at the new rate shows next
    assert not bits_equal(models[2].fused.flat_param, models[0].fused.flat_param)


def test_divergence_leaves_the_reference_state(g21):
    """An absurd lr from epoch 11 on (start_epoch: the reference checks `epoch > 10`): TrainingDivergedError, with the
    parameters and Adam state of the literal loop raising after the same batch."""
    from bcnf_amd import ParameterIndexMapping, Trainer
    from bcnf_amd.errors import TrainingDivergedError
    ma, mb, y, cond, w = _pair(g21, "small")
    cfg = train_config(13, 1e3)
    tr = Trainer(cfg, ParameterIndexMapping(NAMES[:19]), data=(y, cond), order_fn=_order_fn(g21))
    with pytest.raises(TrainingDivergedError, match="Loss exploded"):
        tr.train(ma, start_epoch=11)
    with pytest.raises(TrainingDivergedError, match="Loss exploded"):
        literal_loop(mb, cfg, y, cond, _order_fn(g21), w, start_epoch=11)
    for (n, pa), (_, pb) in zip(ma.named_parameters(), mb.named_parameters()):
        assert bits_equal(pa, pb), n
    assert "stop_reason" not in tr.meta_scheduler.parameter_history


def test_trainer_generates_its_data_on_the_device(g21):
    """data=None: generate_data_device with config["data"], y vectorised in the mapping's order, the condition from
    config["global"]["conditions"][0]; one epoch runs on it."""
    import os

    from conftest import GOLDEN
    from bcnf_amd import ParameterIndexMapping, Trainer
    from bcnf_amd.generate import generate_data_device
    names = ["x0_x", "x0_y", "x0_z", "v0_x", "v0_y", "v0_z", "g_x", "g_y", "g_z", "w_x", "w_y", "w_z", "b", "m", "a_x",
             "a_y", "a_z", "r", "A"]
    cfg = train_config(1, 2e-4)
    cfg["training"]["batch_size"] = 8
    cfg["data"] = {"config_file": os.path.join(GOLDEN, "data_config.yaml"), "n_samples": 24,
                   "output_type": "trajectories", "dt": 1 / 15, "T": 2, "verbose": False, "break_on_impact": True,
                   "do_filter": True}
    tr = Trainer(cfg, ParameterIndexMapping(names))
    y, cond = tr.data
    assert y.is_cuda and y.dtype == torch.float32 and tuple(y.shape) == (24, 19) and tuple(cond.shape) == (24, 30, 3)
    data = generate_data_device(cfg["data"]["config_file"], n=24, output_type="trajectories", dt=1 / 15, T=2)
    assert torch.equal(y[:, 17], data["r"].float()) and torch.equal(y[:, 6], data["g_x"].float())
    assert torch.equal(cond, data["trajectories"].float())
    m = golden_model(g21, "i", dropout=0.5)
    tr.train(m)
    ph = tr.meta_scheduler.parameter_history
    assert ph["stop_reason"] == "max_epochs" and len(ph["train_loss"]) == 2
    assert np.isfinite(ph["train_loss"][-1][1]) and np.isfinite(ph["val_loss"][-1][1])


def test_timeout_stops_after_one_epoch(g21):
    from bcnf_amd import ParameterIndexMapping, Trainer
    ma = golden_model(g21, "i", dropout=0.5)
    y, cond = golden_data(g21)
    logged = []
    tr = Trainer(train_config(50, 2e-4, timeout=0), ParameterIndexMapping(NAMES[:19]), data=(y, cond),
                 order_fn=_order_fn(g21), log_fn=lambda d, step: logged.append(step))
    tr.train(ma)
    ph = tr.meta_scheduler.parameter_history
    assert ph["stop_reason"] == "timeout" and len(ph["val_loss"]) == 2 and logged == [0] * 14
    assert np.isfinite(ph["val_loss"][-1][1])
