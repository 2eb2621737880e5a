"""GPU tests of the validation pass: the bcnf_validation_stats kernel against its numpy float64 restatement
(bcnf_amd.validate.validation_stats_host), and ValidationPass on the reference's recorded model and data
(tests/golden/g21_trainer.npz).

Kernel gates, from fp64 accumulation plus ONE rounding to fp32 (the kernel and the oracle both sum in fp64; their
orders differ, which is ~1e-16 relative to the summed absolute terms and far below an fp32 ulp):
  z_mean, z_std          within 2 fp32 ulps of the oracle's value;
  nll, mse, mean(ldj)    within 2^-22 S, S the mean of the summed absolute terms (nll: mean_b(0.5 sum z^2 + |ldj|));
  loss                   bit-equal to the fp32 expression on the returned nll and mse.
ValidationPass gates: 1e-5, the project's forward gate (conftest.close)."""
import numpy as np
import pytest
import torch

from conftest import close, load_golden
from trainer_ref import BATCH, bits_equal, golden_data, golden_model, validate_torch

pytestmark = pytest.mark.gpu

DEV = "cuda"
SHAPES = [(1, 1), (2, 19), (63, 21), (64, 32), (65, 5), (257, 19), (4099, 21)]


@pytest.fixture(scope="module")
def g21():
    return load_golden("g21_trainer.npz")


def _inputs(B, D, seed, z_shift=0.0, z_scale=1.0, ldj_scale=3.0):
    gen = torch.Generator().manual_seed(seed)
    z = (z_shift + z_scale * torch.randn(B, D, generator=gen)).float()
    ldj = (ldj_scale * torch.randn(B, generator=gen)).float()
    pred = torch.randn(B, D, generator=gen)
    y = torch.randn(B, D, generator=gen)
    return z, ldj, pred, y


def _kernel(z, ldj, pred, y, w, epoch_sum=None):
    from bcnf_amd.validate import validation_stats
    row = validation_stats(z.to(DEV), ldj.to(DEV), None if pred is None else pred.to(DEV),
                           None if y is None else y.to(DEV), w, epoch_sum=epoch_sum)
    torch.cuda.synchronize()
    return row[0].cpu().numpy()


def _ulps(got, ref):
    ref32 = np.asarray(ref, dtype=np.float64).astype(np.float32)
    return np.abs(got.astype(np.float64) - np.asarray(ref, dtype=np.float64)) / np.spacing(np.abs(ref32)).astype(
        np.float64)


def _check(z, ldj, pred, y, w):
    from bcnf_amd.validate import validation_stats_host
    B, D = z.shape
    row = _kernel(z, ldj, pred, y, w)
    assert row.shape == (4 + 2 * D,)
    zn, ln = z.numpy(), ldj.numpy()
    _, nll, mse, ldj_mean, z_mean, z_std = validation_stats_host(
        zn, ln, None if pred is None else pred.numpy(), None if y is None else y.numpy(), w)
    z64, l64 = zn.astype(np.float64), ln.astype(np.float64)
    eps = 2.0 ** -22
    s_nll = (0.5 * (z64 * z64).sum() + np.abs(l64).sum()) / B
    print(f"B={B} D={D} w={w}: nll err {abs(float(row[1]) - nll):.3e} (limit {eps * s_nll:.3e}), "
          f"ldj err {abs(float(row[3]) - ldj_mean):.3e} (limit {eps * np.abs(l64).mean():.3e}), "
          f"mean ulps {_ulps(row[4:4 + D], z_mean).max():.2f}")
    assert abs(float(row[1]) - nll) <= eps * s_nll
    assert abs(float(row[3]) - ldj_mean) <= eps * np.abs(l64).mean()
    if pred is None:
        assert row[2] == 0.0
    else:
        assert abs(float(row[2]) - mse) <= eps * mse          # every term is non-negative: S = mse
    assert _ulps(row[4:4 + D], z_mean).max() <= 2.0
    if B == 1:
        assert np.isnan(row[4 + D:]).all() and np.isnan(z_std).all()
    else:
        su = _ulps(row[4 + D:], z_std).max()
        print(f"  std ulps {su:.2f}")
        assert su <= 2.0
    wf = np.float32(w)
    assert row[0] == (row[1] + row[2] * wf) / (np.float32(1.0) + wf)      # fp32, on the returned nll and mse
    if w == 0.0:
        assert row[0] == row[1]
    return row


@pytest.mark.parametrize("hybrid", [False, True])
@pytest.mark.parametrize("B,D", SHAPES)
def test_kernel_matches_host_oracle(B, D, hybrid):
    z, ldj, pred, y = _inputs(B, D, 1000 * B + D)
    _check(z, ldj, pred if hybrid else None, y if hybrid else None, 0.7 if hybrid else 0.0)


def test_kernel_survives_cancellation():
    """z = 1e3 + 1e-2 randn: sum(z^2) / B - mean^2 in fp32 has no correct digit of the deviation (1e6 against 1e-4)."""
    z, ldj, pred, y = _inputs(257, 19, 5, z_shift=1e3, z_scale=1e-2)
    row = _check(z, ldj, pred, y, 1.0)
    std = row[4 + 19:]
    assert (std > 5e-3).all() and (std < 2e-2).all()


def test_kernel_large_log_det():
    z, ldj, pred, y = _inputs(300, 21, 6, ldj_scale=1e4)
    _check(z, ldj + 1e4, None, None, 0.0)


def test_kernel_is_deterministic_and_accumulates_in_order():
    rows, acc = [], torch.zeros(3, dtype=torch.float64, device=DEV)
    for i, (B, D) in enumerate([(257, 19), (65, 19), (4099, 19), (31, 19)]):
        z, ldj, pred, y = _inputs(B, D, 40 + i)
        a = _kernel(z, ldj, pred, y, 1.0, epoch_sum=acc)
        b = _kernel(z, ldj, pred, y, 1.0)
        assert a.tobytes() == b.tobytes()                  # same inputs, same bits
        rows.append(a)
    want = np.zeros(3, dtype=np.float64)
    for r in rows:                                         # the Trainer's `val_loss += loss.item()`, batch by batch
        want += r[:3].astype(np.float64)
    assert acc.cpu().numpy().tobytes() == want.tobytes()


def test_cursor_selects_the_row_and_advances():
    from bcnf_amd.validate import validation_stats
    z, ldj, _, _ = _inputs(50, 7, 9)
    cursor = torch.tensor([1], dtype=torch.int64, device=DEV)
    rows = torch.full((3, 4 + 14), -5.0, device=DEV)
    validation_stats(z.to(DEV), ldj.to(DEV), row=rows, cursor=cursor, n_batches=3)
    validation_stats(z.to(DEV), ldj.to(DEV), row=rows, cursor=cursor, n_batches=3)
    torch.cuda.synchronize()
    assert int(cursor) == 0                                # 1 -> 2 -> 0 (modulo 3)
    assert (rows[0] == -5.0).all() and torch.equal(rows[1], rows[2])
    assert rows[1].cpu().numpy().tobytes() == _kernel(z, ldj, None, None, 0.0).tobytes()


def test_bad_arguments_launch_nothing():
    from bcnf_amd import _native as N
    z, ldj, pred, y = (t.to(DEV) for t in _inputs(8, 33, 3))
    row = torch.full((4 + 66,), -5.0, device=DEV)
    st = N.stream_handle(row.device)
    assert N.call_raw("bcnf_validation_stats", z, ldj, None, None, 8, 33, 0.0, row, None, None, 1, st) \
        == N.ERR_UNSUPPORTED
    assert N.call_raw("bcnf_validation_stats", z, ldj, None, None, 8, 0, 0.0, row, None, None, 1, st) == N.ERR_ARG
    assert N.call_raw("bcnf_validation_stats", z, ldj, None, None, 0, 19, 0.0, row, None, None, 1, st) == N.ERR_ARG
    assert N.call_raw("bcnf_validation_stats", z, ldj, pred, None, 8, 19, 1.0, row, None, None, 1, st) == N.ERR_ARG
    assert N.call_raw("bcnf_validation_stats", z, ldj, None, None, 8, 19, -1.0, row, None, None, 1, st) == N.ERR_ARG
    assert N.call_raw("bcnf_validation_stats", z, None, None, None, 8, 19, 0.0, row, None, None, 1, st) == N.ERR_ARG
    torch.cuda.synchronize()
    assert (row == -5.0).all()


# ------------------------------------------------------------------------------------------ ValidationPass
def _val_pool(g):
    y, cond = golden_data(g)
    return y[121:].contiguous(), cond[121:].contiguous()


@pytest.mark.parametrize("run", ["i", "ii"])
def test_validation_pass_matches_the_reference(g21, run):
    """The reference's _validate_batch loop at the initial weights (val0/*): 79 samples = one whole batch of 48 and a
    ragged one of 31. Captured equals eager bit for bit; the model's mode and dropout RNG are untouched."""
    from bcnf_amd.validate import ValidationPass
    w = float(g21[f"{run}/w"])
    m = golden_model(g21, run, dropout=0.5)
    m.train()
    rng = m.fused.rng_state().clone()
    yv, cv = _val_pool(g21)
    out = {}
    for capture in (True, False):
        vp = ValidationPass(m, hybrid_weight=w, capture=capture)
        vp.set_pool(yv, cv, BATCH)
        first = vp.run()
        again = vp.run()                                    # a replay (captured) of the same epoch
        assert first[:3] == again[:3] and torch.equal(first[3], again[3]) and torch.equal(first[4], again[4])
        out[capture] = (again, vp.rows.clone())
        assert m.training and torch.equal(m.fused.rng_state(), rng)
    (loss, nll, mse, z_mean, z_std, ldj), rows = out[True]
    for name, got, key in (("loss", loss, "loss"), ("nll", nll, "nll"), ("mse", mse, "mse"), ("ldj", ldj, "ldj_mean"),
                           ("z_mean", z_mean.cpu(), "z_mean"), ("z_std", z_std.cpu(), "z_std")):
        ok, err = close(got, g21[f"{run}/val0/{key}"])
        print(f"run {run} {name}: err {err:.3e}")
        assert ok, (name, err)
    (loss_e, nll_e, mse_e, zm_e, zs_e, ldj_e), rows_e = out[False]
    assert (loss, nll, mse, ldj) == (loss_e, nll_e, mse_e, ldj_e)
    assert bits_equal(rows, rows_e) and bits_equal(z_mean, zm_e) and bits_equal(z_std, zs_e)
    if w == 0.0:
        assert loss == nll and mse == 0.0


def test_validation_pass_multi_batch_graphs(g21):
    """11 whole batches (graphs of 8, 2 and 1) and a ragged one against the torch-op loop."""
    from bcnf_amd.validate import ValidationPass
    m = golden_model(g21, "ii")
    y, cond = golden_data(g21)
    yv, cv = y[:185].contiguous(), cond[:185].contiguous()          # 11 x 16 + 9
    vp = ValidationPass(m, hybrid_weight=1.0)
    vp.set_pool(yv, cv, 16)
    loss, nll, mse, z_mean, z_std, ldj = vp.run()
    assert sorted(vp._graphs) == [1, 2, 8]
    (rl, rn, rm), rzm, rzs, rldj = validate_torch(m, yv, cv, 16, 1.0)
    for name, got, ref in (("loss", loss, rl), ("nll", nll, rn), ("mse", mse, rm), ("ldj", ldj, rldj),
                           ("z_mean", z_mean.cpu(), rzm.cpu()), ("z_std", z_std.cpu(), rzs.cpu())):
        ok, err = close(got, ref)
        assert ok, (name, err)


def test_validation_pass_sees_new_weights(g21):
    """run(), one training epoch, run(): the second pass reads the updated parameters (captured graphs included)."""
    from bcnf_amd.train import TrainStep
    from bcnf_amd.validate import ValidationPass
    m = golden_model(g21, "i", dropout=0.5)
    y, cond = golden_data(g21)
    yv, cv = _val_pool(g21)
    vp = ValidationPass(m)
    vp.set_pool(yv, cv, BATCH)
    before = vp.run()
    ts = TrainStep(m, lr=1e-2)
    ts.set_pool(y[:121].contiguous(), cond[:121].contiguous())
    ts.set_epoch(torch.from_numpy(g21["orders"][0][:96]).cuda(), BATCH)
    m.train()
    ts.run_epoch()
    after = vp.run()
    assert m.training
    (rl, rn, rm), rzm, rzs, rldj = validate_torch(m, yv, cv, BATCH, 0.0)
    assert abs(after[0] - before[0]) > 1e-3                          # the weights did move
    for name, got, ref in (("loss", after[0], rl), ("nll", after[1], rn), ("ldj", after[5], rldj),
                           ("z_mean", after[3].cpu(), rzm.cpu()), ("z_std", after[4].cpu(), rzs.cpu())):
        ok, err = close(got, ref)
        assert ok, (name, err)
