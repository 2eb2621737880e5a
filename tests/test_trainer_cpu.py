"""CPU tests of the training loop's host side (bcnf_amd/trainer.py, bcnf_amd/validate.py) against the reference's
recorded runs (tests/golden/g21_trainer.npz, made by tests/golden/make_golden_trainer.py from Trainer._train):
the epoch-end logic fed the recorded per-epoch values reproduces the reference's parameter history, lr sequence, best
epoch / loss and stop reason with exact float equality; the split and order rules; validation_stats_host against the
torch expressions of Trainer._validate_batch; the argument errors. No GPU."""
import numpy as np
import pytest
import torch

from conftest import load_golden

KEYS = ["train_loss", "train_loss_mse", "train_loss_nll", "val_loss", "val_loss_mse", "val_loss_nll", "lr",
        "distance_to_last_best_val_loss", "time", "z_mean_mean", "z_mean_std", "z_std_mean", "z_std_std", "log_det_J"]


@pytest.fixture(scope="module")
def g21():
    return load_golden("g21_trainer.npz")


def _replay(g, run):
    """Drive epoch_end with the reference's recorded per-epoch values and a real Adam + ReduceLROnPlateau."""
    from bcnf_amd.trainer import TrainerParameterHistoryHandler, epoch_end
    hist = {k: g[f"{run}/hist/{k}"] for k in KEYS}
    n_epochs = int(g[f"{run}/n_epochs"])
    p = torch.nn.Parameter(torch.zeros(1))
    opt = torch.optim.Adam([p], lr=float(g[f"{run}/lr0"]))
    sched = torch.optim.lr_scheduler.ReduceLROnPlateau(opt, patience=1, factor=0.5, threshold_mode="abs")
    logged = []
    h = TrainerParameterHistoryHandler(val_loss_window_size=2, val_loss_patience=4, val_loss_tolerance_mode="abs",
                                       val_loss_tolerance=0.1, fold=-1, log_fn=lambda d, step: logged.append((d, step)))
    stop = None
    for epoch in range(n_epochs):
        h.update_epoch(epoch)
        e = epoch + 1            # entry 0 is the duplicated first value
        v = {k: float(hist[k][e, 1]) for k in KEYS}
        stop = epoch_end(h, epoch, (v["train_loss"], v["train_loss_nll"], v["train_loss_mse"]),
                         (v["val_loss"], v["val_loss_nll"], v["val_loss_mse"]),
                         (v["z_mean_mean"], v["z_mean_std"], v["z_std_mean"], v["z_std_std"], v["log_det_J"]),
                         opt, sched, None, 0.0)
        if stop is not None:
            break
    else:
        h.parameter_history["stop_reason"] = "max_epochs"
    return h, hist, logged


@pytest.mark.parametrize("run", ["i", "ii"])
def test_epoch_end_reproduces_the_reference_history(g21, run):
    h, hist, logged = _replay(g21, run)
    ph = h.parameter_history
    assert ph["stop_reason"] == str(g21[f"{run}/stop_reason"])
    assert [k for k in ph if k != "stop_reason"] == KEYS              # the 14 keys, in the reference's order
    for k in KEYS:
        got = np.array(ph[k], dtype=np.float64)
        assert got.shape == hist[k].shape, k                            # first entry duplicated: epochs + 1 entries
        assert got[0].tolist() == got[1].tolist(), k
        assert np.array_equal(got[:, 0], hist[k][:, 0]), k
        if k != "time":
            assert np.array_equal(got[:, 1], hist[k][:, 1]), k          # exact float equality, lr sequence included
    assert h.best_val_epoch == int(g21[f"{run}/best_val_epoch"])
    assert h.best_val_loss == float(g21[f"{run}/best_val_loss"])
    assert len(logged) == 14 * int(g21[f"{run}/n_epochs_run"])
    d, step = logged[0]
    assert step == 0 and d == {"epoch": 1, "train_loss_fold_-1": float(hist["train_loss"][1, 1])}


def test_golden_run_i_is_discriminating(g21):
    lrs = g21["i/hist/lr"][:, 1]
    assert lrs.min() < lrs[0] and str(g21["i/stop_reason"]) == "val_loss_plateau"
    assert str(g21["ii/stop_reason"]) == "max_epochs" and int(g21["ii/n_epochs_run"]) == 3


def test_handler_quirks():
    from bcnf_amd.trainer import TrainerParameterHistoryHandler as H
    with pytest.raises(ValueError, match="rel.*abs"):
        H(2, 1, "relative")
    h = H(val_loss_window_size=3, val_loss_patience=None)
    for i, v in enumerate([3.0, 1.0, 2.0, 6.0]):
        h.update_epoch(i)
        h.update_rolling_validation_loss(v)
        h.update_best_loss()
    assert h.val_loss_rolling_avg == (1.0 + 2.0 + 6.0) / 3
    assert h.best_val_loss == float("inf") and h.best_val_epoch == 0     # no patience: the best never moves
    r = H(val_loss_window_size=1, val_loss_patience=2, val_loss_tolerance_mode="rel", val_loss_tolerance=0.5)
    for i, v in enumerate([8.0, 5.0, 3.9]):
        r.update_epoch(i)
        r.update_rolling_validation_loss(v)
        r.update_best_loss()
    assert (r.best_val_loss, r.best_val_epoch) == (3.9, 2)               # 5.0 is not < 8.0 * 0.5; 3.9 is
    r.log("x", 1.5)
    assert r.parameter_history["x"] == [(3, 1.5), (3, 1.5)]


def test_epoch_end_timeout_and_patience_order():
    from bcnf_amd.trainer import TrainerParameterHistoryHandler, epoch_end
    opt = torch.optim.Adam([torch.nn.Parameter(torch.zeros(1))], lr=1e-3)
    h = TrainerParameterHistoryHandler(2, 5)
    h.update_epoch(0)
    assert epoch_end(h, 0, (1.0, 1.0, 0.0), (1.0, 1.0, 0.0), (0.0,) * 5, opt, None, 0, start_time=-1.0) == "timeout"
    assert h.parameter_history["stop_reason"] == "timeout"
    # the distance is logged before update_best_loss: an epoch that sets a new best still stops on the old distance
    h = TrainerParameterHistoryHandler(1, 1)
    for epoch, v in enumerate([5.0, 1.0]):
        h.update_epoch(epoch)
        stop = epoch_end(h, epoch, (v, v, 0.0), (v, v, 0.0), (0.0,) * 5, opt, None, None, 0.0)
    assert stop == "val_loss_plateau" and h.best_val_epoch == 1


@pytest.mark.parametrize("n,ratio,want", [(200, 0.4, (121, 79)), (5000, 0.2, (4001, 999)), (10, 0.5, (6, 4))])
def test_split_rule(n, ratio, want):
    from bcnf_amd.trainer import split_sizes
    assert split_sizes(n, ratio) == want
    train_size = int(1 - ratio * n)                      # trainer_data_handler.py:195-203
    idx = list(range(n))
    assert (len(idx[:train_size]), len(idx[train_size:])) == want


def test_default_order_is_reproducible():
    from bcnf_amd.trainer import DEFAULT_RANDOM_STATE, default_order_fn
    a, b, c = default_order_fn(5), default_order_fn(5), default_order_fn(None)
    oa, ob = [a(e, 121) for e in range(3)], [b(e, 121) for e in range(3)]
    assert all(torch.equal(x, y) for x, y in zip(oa, ob))
    assert not torch.equal(oa[0], oa[1])                                  # one generator: epochs differ
    assert sorted(oa[0].tolist()) == list(range(121))
    g = torch.Generator().manual_seed(DEFAULT_RANDOM_STATE)
    assert torch.equal(c(0, 50), torch.randperm(50, generator=g))


@pytest.mark.parametrize("B,D,w", [(1, 3, 0.0), (2, 19, 1.0), (48, 19, 0.0), (31, 21, 0.1), (300, 5, 1.0)])
def test_validation_stats_host_matches_validate_batch(B, D, w):
    """The torch expressions of Trainer._validate_batch (trainer.py:293-303) in float64, and in fp32 at the fp32
    expressions' own accuracy."""
    from bcnf_amd.utils import inn_nll_loss
    from bcnf_amd.validate import validation_stats_host
    gen = torch.Generator().manual_seed(B * 100 + D)
    z = torch.randn(B, D, generator=gen, dtype=torch.float64) * 1.5 + 0.3
    ldj = torch.randn(B, generator=gen, dtype=torch.float64) * 4 - 7
    pred = torch.randn(B, D, generator=gen, dtype=torch.float64)
    y = torch.randn(B, D, generator=gen, dtype=torch.float64)
    hybrid = w > 0
    loss, nll, mse, ldj_mean, z_mean, z_std = validation_stats_host(
        z.numpy(), ldj.numpy(), pred.numpy() if hybrid else None, y.numpy() if hybrid else None, w)
    nll_t = inn_nll_loss(z, ldj)
    mse_t = torch.nn.MSELoss()(pred, y) if hybrid else torch.tensor(0.0, dtype=torch.float64)
    assert nll == pytest.approx(nll_t.item(), rel=1e-13, abs=1e-13)
    assert mse == pytest.approx(mse_t.item(), rel=1e-13)
    assert ldj_mean == pytest.approx(ldj.mean().item(), rel=1e-13)
    np.testing.assert_allclose(z_mean, z.mean(0).numpy(), rtol=1e-12, atol=1e-14)
    if B == 1:
        assert np.isnan(z_std).all() and torch.isnan(z.std(0)).all()
    else:
        np.testing.assert_allclose(z_std, z.std(0).numpy(), rtol=1e-12)
    # loss: the fp32 expression on the rounded nll and mse
    n32, m32, w32 = np.float32(nll), np.float32(mse), np.float32(w)
    assert loss == float((n32 + m32 * w32) / (np.float32(1) + w32))
    if not hybrid:
        assert loss == float(n32) and mse == 0.0
    # ... which is what the reference's fp32 tensors give, to fp32 accuracy
    ref = (nll_t.float() + mse_t.float() * w) / (1 + w)
    assert loss == pytest.approx(ref.item(), rel=4e-7)


def _two_condition_model():
    from bcnf_amd import CondRealNVP_v2
    cfg = {"global": {"parameter_selection": [str(i) for i in range(19)]},
           "model": {"kwargs": {"size": 19, "nested_sizes": [16] * 2, "n_conditions": 80, "n_blocks": 2}},
           "feature_networks": [{"type": "ConcatenateCondition", "kwargs": {"input_size": None, "output_size": 60}},
                                {"type": "ConcatenateCondition", "kwargs": {"input_size": 60, "output_size": 90}},
                                {"type": "FullyConnected", "kwargs": {"sizes": [90, 80]}}]}
    return CondRealNVP_v2.from_config(cfg)


def _train_config():
    return {"global": {"conditions": [["trajectories"]]},
            "training": {"val_loss_window_size": 2, "val_loss_patience": 4, "val_loss_tolerance_mode": "abs",
                         "val_loss_tolerance": 0.1, "n_epochs": 1, "validation_split": 0.4, "batch_size": 4,
                         "timeout": None},
            "optimizer": {"type": "Adam", "kwargs": {"lr": 1e-3}},
            "lr_scheduler": {"type": "ReduceLROnPlateau", "kwargs": {}}}


def test_argument_errors(monkeypatch):
    import bcnf_amd
    from bcnf_amd import Trainer, ValidationPass
    assert {"Trainer", "TrainerParameterHistoryHandler", "ValidationPass"} <= set(bcnf_amd.__all__)
    two = _two_condition_model()
    with pytest.raises(NotImplementedError, match="TrainStep's one-condition limit"):
        ValidationPass(two)
    data = (torch.zeros(10, 19), torch.zeros(10, 30, 3))
    mapping = bcnf_amd.ParameterIndexMapping([str(i) for i in range(19)])
    with pytest.raises(NotImplementedError, match="TrainStep's one-condition limit"):
        Trainer(_train_config(), mapping, data=data).train(two)
    cfg = _train_config()
    cfg["global"]["conditions"] = [["trajectories"], ["cams"]]
    with pytest.raises(NotImplementedError, match="TrainStep's one-condition limit"):
        Trainer(cfg, mapping, data=data)
    from bcnf_amd import CondRealNVP_v2
    one = CondRealNVP_v2.from_config({
        "global": {"parameter_selection": [str(i) for i in range(19)]},
        "model": {"kwargs": {"size": 19, "nested_sizes": [16] * 2, "n_conditions": 80, "n_blocks": 2}},
        "feature_networks": [{"type": "ConcatenateCondition", "kwargs": {"input_size": None, "output_size": 90}},
                             {"type": "FullyConnected", "kwargs": {"sizes": [90, 80]}}]})
    with pytest.raises(RuntimeError, match="needs set_pool"):
        ValidationPass(one).run()
    with pytest.raises(ValueError, match="hybrid=True"):
        ValidationPass(one, hybrid_weight=1.0)
    monkeypatch.setattr(torch.distributed, "is_initialized", lambda: True)
    monkeypatch.setattr(torch.distributed, "get_world_size", lambda *a, **k: 2)
    with pytest.raises(NotImplementedError, match="world size > 1"):
        Trainer(_train_config(), mapping, data=data)
