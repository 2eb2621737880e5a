"""GPU calibration ranks (bcnf_amd/calibration.py, bcnf_eval.hip) vs the reference's compute_y_hat_ranks semantics
(eval/calibration.py:20-48: ranks = sum over draws of [y_hat < y], draws from sample(outer=True))."""
import pytest
import torch

from conftest import FC_SMALL_CFG, golden_sd
from oracle import cnf_oracle as O

pytestmark = pytest.mark.gpu


def _model(g1):
    from bcnf_amd import CondRealNVP_v2
    torch.manual_seed(0)
    m = CondRealNVP_v2.from_config(FC_SMALL_CFG)
    m.load_state_dict(golden_sd(g1))
    return m.to("cuda").eval()


def test_rank_count_kernel_exact():
    from bcnf_amd.calibration import rank_count_
    g = torch.Generator().manual_seed(1)
    y_hat = torch.randn(1000, 33, 19, generator=g)
    y = torch.randn(33, 19, generator=g)
    y_hat[7, 3, 4] = y[3, 4]                  # ties do not count (strict <), as in the reference
    ref = (torch.cat([y_hat, y.unsqueeze(0)]) < y.unsqueeze(0)).sum(0)
    counts = torch.zeros(33, 19, dtype=torch.int32, device="cuda")
    rank_count_(counts, y_hat[:600].cuda(), y.cuda())      # chunked accumulation
    rank_count_(counts, y_hat[600:].cuda(), y.cuda())
    assert torch.equal(counts.cpu().long(), ref)


def _guarded_counts(n_rows, dim, seed):
    """(buffer, (n_rows, dim) view, its starting values): nonzero int32 counts inside canaries -- the call accumulates."""
    from gpu_guard import guarded1
    start = torch.randint(1, 1000, (n_rows * dim,), generator=torch.Generator().manual_seed(seed), dtype=torch.int32)
    buf, view = guarded1(n_rows * dim, start, dtype=torch.int32)
    return buf, view.view(n_rows, dim), start.view(n_rows, dim)


# S_PER_WG = 64 draws per workgroup: one draw, the full group, one past it, two groups and one; 256 lanes per
# workgroup along N * D: 255, 256 and 257 elements
@pytest.mark.parametrize("n_rows,dim", [(15, 17), (16, 16), (257, 1)])
@pytest.mark.parametrize("M", [1, 64, 65, 129])
def test_rank_count_at_the_workgroup_edges(M, n_rows, dim):
    from bcnf_amd.calibration import rank_count_
    from gpu_guard import canaries_alive1
    g = torch.Generator().manual_seed(1000 * M + n_rows)
    y_hat = torch.randn(M, n_rows, dim, generator=g)
    y = torch.randn(n_rows, dim, generator=g)
    y_hat[M // 2, n_rows - 1, dim - 1] = y[n_rows - 1, dim - 1]           # a tie in the last element
    ref = (y_hat.double() < y.double().unsqueeze(0)).sum(0)
    buf, counts, start = _guarded_counts(n_rows, dim, M)
    rank_count_(counts, y_hat.cuda(), y.cuda())
    torch.cuda.synchronize()
    assert canaries_alive1(buf, n_rows * dim)
    assert torch.equal(counts.cpu().long(), start.long() + ref)
    assert int(ref.max()) <= M and (M == 1 or int(ref.max()) > 0)


def test_rank_count_of_non_finite_and_signed_zero_values():
    """Strict IEEE <: a NaN on either side counts nothing, the infinities order as numbers, -0.0 is not below +0.0,
    a tie does not count."""
    from bcnf_amd.calibration import rank_count_
    from gpu_guard import canaries_alive1
    M, n_rows, dim = 65, 3, 9
    nan, inf = float("nan"), float("inf")
    g = torch.Generator().manual_seed(5)
    y_hat = torch.randn(M, n_rows, dim, generator=g)
    y = torch.randn(n_rows, dim, generator=g)
    expect = (y_hat.double() < y.double().unsqueeze(0)).sum(0)
    #                      column: draws                          y          count
    planted = [(lambda s: nan,                               0.25, 0),       # every draw NaN
               (lambda s: nan if s % 2 else -1.0,            0.25, 33),      # the odd draws NaN
               (lambda s: float(s),                          nan, 0),        # y NaN
               (lambda s: -inf,                              0.0, M),
               (lambda s: inf,                               0.0, 0),
               (lambda s: float(s),                          inf, M),
               (lambda s: inf if s < 64 else nan,            inf, 0),        # inf < inf is false
               (lambda s: -inf if s < 64 else 0.0,           -inf, 0),
               (lambda s: -0.0,                              0.0, 0),        # -0.0 < +0.0 is false
               ]
    for col, (draw, ref, count) in enumerate(planted):
        y_hat[:, 1, col] = torch.tensor([draw(s) for s in range(M)])
        y[1, col] = ref
        expect[1, col] = count
    y_hat[:, 2, 0], y[2, 0], expect[2, 0] = 0.0, -0.0, 0                  # +0.0 < -0.0 is false
    y_hat[:, 2, 1], y[2, 1], expect[2, 1] = y[2, 2], y[2, 2], 0           # M exact ties
    y_hat[:64, 2, 3], y_hat[64, 2, 3], y[2, 3], expect[2, 3] = 1.0, 0.5, 1.0, 1     # ties, and one draw below
    assert torch.equal((y_hat < y.unsqueeze(0)).sum(0), expect)           # torch's float32 < says the same
    buf, counts, start = _guarded_counts(n_rows, dim, 9)
    rank_count_(counts, y_hat.cuda(), y.cuda())
    torch.cuda.synchronize()
    assert canaries_alive1(buf, n_rows * dim)
    assert torch.equal(counts.cpu().long(), start.long() + expect)


def test_rank_count_empty_and_refused_calls():
    """n_draws = 0 and n_rows = 0 are OK and count nothing; dim = 0 is refused; more than 65535 groups of 64 draws is
    the library's unsupported status, returned before any launch. counts stays as it was throughout."""
    from bcnf_amd import _native as N
    from gpu_guard import canaries_alive1
    buf, counts, start = _guarded_counts(4, 5, 3)
    y_hat = torch.full((2 * 4 * 5,), -1.0, device="cuda")                  # would count everywhere
    y = torch.zeros(4 * 5, device="cuda")
    st = N.stream_handle(y.device)
    assert N.call_raw("bcnf_rank_count", y_hat, y, 0, 4, 5, counts, st) == N.OK
    assert N.call_raw("bcnf_rank_count", y_hat, y, 2, 0, 5, counts, st) == N.OK
    assert N.call_raw("bcnf_rank_count", y_hat, y, 2, 4, 0, counts, st) == N.ERR_ARG
    assert N.call_raw("bcnf_rank_count", y_hat, y, -1, 4, 5, counts, st) == N.ERR_ARG
    assert N.call_raw("bcnf_rank_count", y_hat, y, 2, -1, 5, counts, st) == N.ERR_ARG
    assert N.call_raw("bcnf_rank_count", None, y, 2, 4, 5, counts, st) == N.ERR_ARG
    assert N.call_raw("bcnf_rank_count", y_hat, y, 2, 4, 5, None, st) == N.ERR_ARG
    assert N.call_raw("bcnf_rank_count", y_hat, y, 64 * 65535 + 1, 1, 1, counts, st) == N.ERR_UNSUPPORTED
    torch.cuda.synchronize()
    assert canaries_alive1(buf, 20) and torch.equal(counts.cpu(), start)
    # the same buffers do count
    assert N.call_raw("bcnf_rank_count", y_hat, y, 2, 4, 5, counts, st) == N.OK
    torch.cuda.synchronize()
    assert torch.equal(counts.cpu(), start + 2) and canaries_alive1(buf, 20)


def test_compute_y_hat_ranks_reference_stream(g1):
    from bcnf_amd.calibration import compute_y_hat_ranks
    m = _model(g1)
    sd = golden_sd(g1)
    g = torch.Generator().manual_seed(2)
    traj = torch.randn(21, 30, 3, generator=g)
    y = torch.randn(21, 19, generator=g)
    torch.manual_seed(77)
    got = compute_y_hat_ranks(m, y, traj, M_samples=300, batch_size=8, sample_batch_size=64, device="cuda")
    torch.manual_seed(77)
    y_hat = O.sample(sd, O.FC_SMALL_SPEC, 300, traj, outer=True, batch_size=8, sample_batch_size=64)
    ref = (y_hat < y.unsqueeze(0)).sum(0)
    assert got.dtype == torch.int64 and got.device.type == "cpu" and got.shape == (21, 19)
    # the draws agree to ~1e-6; only a draw within that distance of y could flip one comparison
    assert (got - ref).abs().max().item() <= 1 and (got != ref).float().mean().item() < 1e-2


def test_compute_y_hat_ranks_device_stream(g1):
    from bcnf_amd.calibration import compute_y_hat_ranks
    m = _model(g1)
    g = torch.Generator().manual_seed(3)
    traj = torch.randn(40, 30, 3, generator=g)
    y = torch.randn(40, 19, generator=g)
    runs = []
    for _ in range(2):
        gen = torch.Generator(device="cuda").manual_seed(5)
        runs.append(compute_y_hat_ranks(m, y, traj, M_samples=1200, device="cuda", z_stream="device", generator=gen,
                                        chunk_draws=500))
    a, b = runs
    assert a.shape == (40, 19) and int(a.min()) >= 0 and int(a.max()) <= 1200
    assert torch.equal(a, b)                    # seeded device stream: reproducible
    # calibrated-in-distribution sanity: y drawn from the model itself ranks uniformly -> mean rank ~ M / 2
    with torch.no_grad():
        z = torch.randn(40, 19, generator=g).cuda()
        y_model = m.inverse(z, traj.cuda())
    gen = torch.Generator(device="cuda").manual_seed(6)
    r = compute_y_hat_ranks(m, y_model, traj, M_samples=1200, device="cuda", z_stream="device", generator=gen)
    assert abs(r.double().mean().item() / 1200 - 0.5) < 0.05
