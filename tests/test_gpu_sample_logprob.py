"""Posterior draws with their log-density out of the fused inverse (k_inverse_mfma<.., LDJ>, k_wlink<INV, .., LDJ>;
bcnf_stack_inverse_logdet / bcnf_wide_inverse_logdet; inverse(log_det_J=True), sample / draw(return_log_prob=True),
posterior_mode).

Truth: the fp64 oracle, never the new code -- y64 = model_inverse(z), ldj64 = model_forward(y64)[1], log_prob64 =
O.log_prob(z, ldj64). The reference's own error ref_err is the same two calls in fp32 against the fp64 value. Gate
(the round-trip gate of tests/test_gpu_parity.py:66-73 plus conftest.close):
    |got - truth| <= 2 ref_err + 1e-5 |truth| + 1e-5 max(1, max|truth|).
Every gated case also asserts ldj64.std() >= 100 * gate, so the per-sample variation from the couplings is far above
what the gate lets through: a wrong sign, a dropped block or a dropped feature fails.

Rows N in {1, 37, 300}: one lane group, less than one 128-row workgroup, three workgroups with a ragged tail. The
reference values are computed once per case on 300 rows; a row's result does not depend on its position (checked
here bit for bit), so the N = 1 and N = 37 calls are gated against the first rows of it."""
import copy
import functools

import pytest
import torch

from conftest import FC_SMALL_CFG, close, golden_sd, large_proxy_sd, load_golden
from dropout_ref import apply_gain
from oracle import cnf_oracle as O

pytestmark = pytest.mark.gpu
DEV = "cuda"
NC = 7                                   # conditions behind cond_index

# name -> (model kwargs, family). (a) PERM; (b) Da = Db = 16: non-PERM; (c) no ActNorm; (d) one block: no Q, no ActNorm;
# (f) .. (l): the NH = 1, 4, 5, 6, 8 arms of k_inverse_mfma (tests/small_arms.py)
CASES = {
    "a_perm": (dict(size=19, nested_sizes=[16] * 3, n_blocks=4, n_conditions=80, act_norm=True), "FusedStack"),
    "b_nonperm": (dict(size=32, nested_sizes=[16] * 2, n_blocks=3, n_conditions=24, act_norm=True), "FusedStack"),
    "c_no_actnorm": (dict(size=7, nested_sizes=[16] * 2, n_blocks=3, n_conditions=8, act_norm=False), "FusedStack"),
    "d_one_block": (dict(size=19, nested_sizes=[16] * 3, n_blocks=1, n_conditions=80, act_norm=True), "FusedStack"),
    "e_g1": (None, "FusedStack"),       # the reference's trained-shape weights, full depth (32 blocks, [16] * 7)
    # NH = 4, 5, 6 (12 / 12 the last PERM layout, 13 / 12 the first non-PERM, 10 / 10), C = 17, KC, KC + 1; (g) has a
    # hidden layer of width 1
    "f_nh4_d24": (dict(size=24, nested_sizes=[16] * 4, n_blocks=3, n_conditions=17, act_norm=True), "FusedStack"),
    "g_nh5_d25": (dict(size=25, nested_sizes=[16, 7, 16, 1, 11], n_blocks=4, n_conditions=128, act_norm=True),
                  "FusedStack"),
    "h_nh6_d20": (dict(size=20, nested_sizes=[16] * 6, n_blocks=5, n_conditions=129, act_norm=True), "FusedStack"),
    # (i) NH = 1: the empty hidden-bias section of the matrix-core record (PMB); (j) NH = 8 at Da = 2, Db = 1 without
    # ActNorm; (l) NH = 8 at D = 22: PMB = 3792 of the 4096 floats of a ring slot
    "i_nh1_d23": (dict(size=23, nested_sizes=[16], n_blocks=3, n_conditions=1, act_norm=True), "FusedStack"),
    "j_nh8_d3": (dict(size=3, nested_sizes=[5] * 8, n_blocks=2, n_conditions=16, act_norm=False), "FusedStack"),
    "l_nh8_d22": (dict(size=22, nested_sizes=[16] * 8, n_blocks=2, n_conditions=128, act_norm=True), "FusedStack"),
    "w48": (dict(size=19, nested_sizes=[48] * 2, n_blocks=3, n_conditions=80, act_norm=True), "WideStack"),
    "w20_one_hidden": (dict(size=19, nested_sizes=[20], n_blocks=3, n_conditions=4, act_norm=True), "WideStack"),
    "w24_c13": (dict(size=19, nested_sizes=[24] * 2, n_blocks=2, n_conditions=13, act_norm=True), "WideStack"),
    "w526_fc_large": (dict(size=19, nested_sizes=[526] * 5, n_blocks=2, n_conditions=1360, act_norm=True),
                      "WideStack"),
}
# dropout_ref.apply_gain's factor on the coupling weights, after large_proxy_sd (absent: 1)
GAIN = {"g_nh5_d25": 2.0, "h_nh6_d20": 2.0, "j_nh8_d3": 2.0, "l_nh8_d22": 2.0}
ROWS = {name: ((64,) if name == "w526_fc_large" else (1, 37, 300)) for name in CASES}
SMALL = [n for n, (_, fam) in CASES.items() if fam == "FusedStack"]
WIDE = [n for n, (_, fam) in CASES.items() if fam == "WideStack"]


@functools.lru_cache(maxsize=None)
def _case(name):
    """(model on the GPU in eval mode, fp32 state dict, oracle spec, conditions (NC, 30, 3), and the reference on the
    case's largest row count). Built once per case and left unchanged."""
    from bcnf_amd import CondRealNVP_v2
    kw, fam = CASES[name]
    torch.manual_seed(11)
    if kw is None:
        g1 = load_golden("g1_fc_small.npz")
        m = CondRealNVP_v2.from_config(copy.deepcopy(FC_SMALL_CFG))
        sd = golden_sd(g1)
        spec = O.FC_SMALL_SPEC
        # conditions of physical magnitude (the reference ODE simulator's trajectories, |x| up to 85 m: what the model
        # is conditioned on in use). With the fixture's own unit-scale traj rows the conditions barely move ldj: its
        # std over the rows is 0.038 against a gate of 4.3e-4 (|ldj64| ~ 20.6 sets the gate), short of the 100 x the
        # condition on the inputs asks; across these trajectories it is 0.074 (fp64 oracle, not the kernels).
        cond = torch.from_numpy(load_golden("g9_ballistic.npz")["traj"][:NC].copy()).float()
    else:
        C = kw["n_conditions"]
        cfg = {"global": {"parameter_selection": [f"p{i}" for i in range(kw["size"])]},
               "model": {"kwargs": dict(kw, dropout=0.0)},
               "feature_networks": [
                   {"type": "ConcatenateCondition", "kwargs": {"input_size": None, "output_size": 90}},
                   {"type": "FullyConnected", "kwargs": {"sizes": [90, C], "dropout": 0.0}}]}
        m = CondRealNVP_v2.from_config(cfg)
        sd = {k: torch.from_numpy(v) for k, v in large_proxy_sd(m, 2024_03_25 + len(name)).items()}
        if name in GAIN:
            apply_gain(sd, GAIN[name])
        spec = O.StackSpec(size=kw["size"], nested_sizes=kw["nested_sizes"], n_blocks=kw["n_blocks"], n_conditions=C,
                           act_norm=kw["act_norm"], feature_sizes=[90, C])
        cond = torch.randn(NC, 30, 3, generator=torch.Generator().manual_seed(5))
    assert type(m.fused).__name__ == fam
    m.load_state_dict(sd)
    m.to(DEV).eval()
    n = max(ROWS[name])
    z = torch.randn(n, spec.size, generator=torch.Generator().manual_seed(7))
    idx = torch.arange(n) % NC
    ref = _reference(sd, spec, z, cond, idx)
    return m, sd, spec, cond, z, idx, ref


def _reference(sd, spec, z, cond, idx):
    """fp64 truth and the reference's own fp32 values of (y, ldj, log_prob) for latent rows z with conditions
    cond[idx]."""
    out = {}
    for tag, cast in (("64", torch.Tensor.double), ("32", torch.Tensor.float)):
        s = {k: cast(v) for k, v in sd.items()}
        h = O.feature_forward(s, spec, cast(cond))[idx]
        with torch.no_grad():
            y = O.model_inverse(s, spec, cast(z), h)
            ldj = O.model_forward(s, spec, y, h)[1]
        out["y" + tag], out["ldj" + tag], out["lp" + tag] = y, ldj, O.log_prob(cast(z), ldj)
    return out


def _tol(truth, ref32):
    ref_err = float((ref32.double() - truth).abs().max())
    return 2.0 * ref_err + 1e-5 * truth.abs() + 1e-5 * max(1.0, float(truth.abs().max())), ref_err


def _guard(what, ref):
    """The condition on the inputs: the couplings' per-sample variation is >= 100 x what the gate lets through."""
    tol_l, _ = _tol(ref["ldj64"], ref["ldj32"])
    std = float(ref["ldj64"].std())
    assert std >= 100.0 * float(tol_l.max()), (what, "inputs: ldj64.std() < 100 * gate", std, float(tol_l.max()))


def _gate(what, got, ref, rows=None):
    """Gate ldj and log_prob of `rows` of the reference; print each figure before asserting. The caller ends with
    _guard(ref), after every row count has been gated."""
    sl = slice(None) if rows is None else rows
    ldj, lp = got
    tol_l, re_l = _tol(ref["ldj64"], ref["ldj32"])
    tol_p, re_p = _tol(ref["lp64"], ref["lp32"])
    err_l = (ldj.detach().cpu().double() - ref["ldj64"][sl]).abs()
    err_p = (lp.detach().cpu().double() - ref["lp64"][sl]).abs()
    std = float(ref["ldj64"].std()) if ref["ldj64"].numel() > 1 else float("nan")
    print(f"{what}: ldj err {float(err_l.max()):.3e} (ref_err {re_l:.3e}, gate {float(tol_l.max()):.3e}, "
          f"ldj64 std {std:.3e}); log_prob err {float(err_p.max()):.3e} (ref_err {re_p:.3e}, "
          f"gate {float(tol_p.max()):.3e})")
    assert bool((err_l <= tol_l[sl]).all()), (what, "ldj", float(err_l.max()))
    assert bool((err_p <= tol_p[sl]).all()), (what, "log_prob", float(err_p.max()))


def _gate_lp(what, lp, ref):
    """Gate log_prob alone (sample / draw return no ldj), with the same condition on the inputs."""
    tol_p, re_p = _tol(ref["lp64"], ref["lp32"])
    err = (lp.detach().cpu().double() - ref["lp64"]).abs()
    std = float(ref["ldj64"].std())
    print(f"{what}: log_prob err {float(err.max()):.3e} (ref_err {re_p:.3e}, gate {float(tol_p.max()):.3e}, "
          f"ldj64 std {std:.3e})")
    assert bool((err <= tol_p).all()), (what, "log_prob", float(err.max()))
    _guard(what, ref)


def _inverse(m, z, h, idx, want_ldj=True):
    from bcnf_amd.fused import stack_inverse
    with torch.no_grad():
        return stack_inverse(m.fused, z.to(DEV), h, cond_index=None if idx is None else idx.to(DEV),
                             want_ldj=want_ldj)


def _features(m, cond):
    with torch.no_grad():
        return m.feature_network_stack(cond.to(DEV)).contiguous()


# ------------------------------------------------------------------------------------------ values vs the fp64 oracle
@pytest.mark.parametrize("name", SMALL + WIDE)
def test_ldj_and_log_prob_match_the_fp64_oracle(name):
    """Every row count with cond_index, and 37 rows without it, against the gate; then the condition on the inputs.

    The figures of every case are printed before they are asserted (pytest -s)."""
    m, sd, spec, cond, z, idx, ref = _case(name)
    h = _features(m, cond)
    for n in ROWS[name]:
        y, ldj, lp = _inverse(m, z[:n], h, idx[:n])
        assert ldj.shape == (n,) and lp.shape == (n,) and y.shape == (n, spec.size)
        _gate(f"{name} N={n} cond_index", (ldj, lp), ref, slice(0, n))
        ok, err = close(y.cpu(), ref["y32"][:n])
        assert ok, (name, n, "y", err)
        # the flag changes nothing about y
        assert torch.equal(y, _inverse(m, z[:n], h, idx[:n], want_ldj=False))
    # without cond_index: the tiled feature rows (37 rows; the FC_large-shaped proxy runs at its 64)
    n = 37 if 37 in ROWS[name] else ROWS[name][0]
    y, ldj, lp = _inverse(m, z[:n], h[idx[:n].to(DEV)].contiguous(), None)
    _gate(f"{name} N={n} tiled", (ldj, lp), ref, slice(0, n))
    assert torch.equal(y, _inverse(m, z[:n], h[idx[:n].to(DEV)].contiguous(), None, want_ldj=False))
    _guard(name, ref)


POSITION_CASES = ["a_perm", "b_nonperm", "e_g1", "w48", "w24_c13", "g_nh5_d25", "h_nh6_d20"]


@pytest.mark.parametrize("name", POSITION_CASES)
def test_rows_do_not_depend_on_their_position(name):
    m, sd, spec, cond, z, idx, ref = _case(name)
    h = _features(m, cond)
    full = _inverse(m, z, h, idx)
    rev = _inverse(m, z.flip(0), h, idx.flip(0))
    for a, b in zip(full, rev):
        assert torch.equal(a, b.flip(0))
    rows = torch.arange(131, 168)                                # 37 rows across a workgroup boundary of the 300
    sub = _inverse(m, z[rows], h, idx[rows])
    for a, b in zip(full, sub):
        assert torch.equal(a[rows.to(DEV)], b)


@pytest.mark.parametrize("name", ["a_perm", "b_nonperm", "w48"])
def test_model_inverse_sets_log_det_J_and_agrees_with_the_forward_kernels(name):
    m, sd, spec, cond, z, idx, ref = _case(name)
    n = 37
    c = cond[idx[:n]].to(DEV)
    with torch.no_grad():
        y_plain = m.inverse(z[:n].to(DEV), c)
        y = m.inverse(z[:n].to(DEV), c, log_det_J=True)
        ldj = m.log_det_J.clone()
        assert ldj.shape == (n,) and torch.equal(y, y_plain)
        _, _, lp = _inverse(m, z[:n], _features(m, cond), idx[:n])
        lp_fwd = m.log_prob(y, c)                               # the existing forward kernels at the draw
        ldj_fwd = m.log_det_J.clone()
    ok, err = close(lp.cpu(), lp_fwd.cpu())
    assert ok, (name, "log_prob vs model.log_prob", err)
    ok, err = close(ldj.cpu(), ldj_fwd.cpu())
    assert ok, (name, "ldj vs forward", err)


# ------------------------------------------------------------------------------------------ sample / draw
def _sample_reference(sd, spec, cond, seed, n, batch_size, sample_batch_size, outer):
    """The z stream of CondRealNVP_v2.sample (cnf.py:510-588: per condition chunk, per sample chunk, one CPU randn)
    replayed, then the fp64 / fp32 reference per chunk, assembled like the samples."""
    torch.manual_seed(seed)
    m_sizes = [s for s in [sample_batch_size] * (n // sample_batch_size) + [n % sample_batch_size] if s]
    cols = []
    for b in range(0, len(cond), batch_size):
        c = cond[b:b + batch_size]
        nc = c.shape[0]
        parts = []
        for ms in m_sizes:
            if outer:
                z = torch.randn(ms * nc, spec.size)
                r = _reference(sd, spec, z, c, torch.arange(ms * nc) % nc)
                parts.append({k: v.view(ms, nc, *v.shape[1:]) for k, v in r.items()})
            else:
                z = torch.randn(ms, spec.size)
                parts.append(_reference(sd, spec, z, c, torch.arange(ms)))
        cols.append({k: torch.cat([p[k] for p in parts], dim=0) for k in parts[0]})
    return {k: torch.cat([c[k] for c in cols], dim=1 if outer else 0) for k in cols[0]}


@pytest.mark.parametrize("name", ["a_perm", "w48"])
def test_sample_returns_log_prob(name):
    m, sd, spec, cond, z, idx, _ = _case(name)
    kw = dict(outer=True, batch_size=3, sample_batch_size=16)
    torch.manual_seed(123)
    plain = m.sample(50, cond, **kw)
    torch.manual_seed(123)
    s, lp = m.sample(50, cond, return_log_prob=True, **kw)
    assert s.shape == (50, NC, 19) and lp.shape == (50, NC) and s.device.type == "cpu" and lp.device.type == "cpu"
    assert torch.equal(s, plain)
    ref = _sample_reference(sd, spec, cond, 123, 50, 3, 16, True)
    torch.manual_seed(123)          # the replayed z stream is sample()'s (the oracle tiles the conditions before the
    ok, err = close(ref["y32"], O.sample(sd, spec, 50, cond, **kw))         # feature GEMM: same values, not bits)
    assert ok, err
    ok, err = close(s, ref["y32"])
    assert ok, err
    _gate_lp(f"{name} sample outer", lp.reshape(-1), {k: v.reshape(-1, *v.shape[2:]) for k, v in ref.items()})


def test_sample_non_outer_and_1d_condition():
    m, sd, spec, cond, z, idx, _ = _case("a_perm")
    torch.manual_seed(77)
    plain = m.sample(NC, cond)
    torch.manual_seed(77)
    s, lp = m.sample(NC, cond, return_log_prob=True)
    assert s.shape == (NC, 19) and lp.shape == (NC,) and torch.equal(s, plain)
    _gate_lp("sample non-outer", lp, _sample_reference(sd, spec, cond, 77, NC, 100, 100, False))
    # a 1-D condition: n draws of the one condition
    c1 = cond[2].reshape(-1)
    torch.manual_seed(78)
    plain = m.sample(5, c1)
    torch.manual_seed(78)
    s, lp = m.sample(5, c1, return_log_prob=True)
    assert s.shape == (5, 19) and lp.shape == (5,) and torch.equal(s, plain)
    torch.manual_seed(78)
    z1 = torch.randn(5, 19)
    _gate_lp("sample 1-D condition", lp, _reference(sd, spec, z1, cond[2:3], torch.zeros(5, dtype=torch.int64)))


@pytest.mark.parametrize("name", ["a_perm", "w48"])
def test_draw_returns_log_prob_and_posterior_mode_picks_the_best(name):
    from bcnf_amd import posterior_mode
    from bcnf_amd.sampling import draw
    m, sd, spec, _, _, _, _ = _case(name)
    gen = torch.Generator().manual_seed(9)
    n, N = 20, 9
    cond = torch.randn(N, 30, 3, generator=gen)
    z = torch.randn(n * N, spec.size, generator=gen)
    plain = draw(m, n, cond.to(DEV), z=z.to(DEV))
    y, lp = draw(m, n, cond.to(DEV), z=z.to(DEV), return_log_prob=True)
    assert y.shape == (n, N, spec.size) and lp.shape == (n, N) and torch.equal(y, plain)
    ref = _reference(sd, spec, z, cond, torch.arange(n * N) % N)
    _gate_lp(f"{name} draw", lp.reshape(-1), ref)
    ym, lpm = posterior_mode(m, n, cond.to(DEV), z=z.to(DEV))
    best = lp.argmax(dim=0)
    assert ym.shape == (N, spec.size) and lpm.shape == (N,)
    assert torch.equal(lpm, lp[best, torch.arange(N, device=DEV)])
    assert torch.equal(ym, y[best, torch.arange(N, device=DEV)])
    # tempered proposal (sigma != 1): log_prob is still the model's density at the draw, z the scaled latent
    y2, lp2 = draw(m, n, cond.to(DEV), z=z.to(DEV), sigma=0.5, return_log_prob=True)
    _gate_lp(f"{name} draw sigma=0.5", lp2.reshape(-1), _reference(sd, spec, 0.5 * z, cond, torch.arange(n * N) % N))


# ------------------------------------------------------------------------------------------ AnyGLU (layerwise)
GLU_ONE_WAY = {"global": FC_SMALL_CFG["global"],
               "model": {"kwargs": {"size": 19, "nested_sizes": [24, 24, 24], "n_conditions": 12, "n_blocks": 3,
                                    "dropout": 0.407, "act_norm": True, "two_way": False, "layer": "AnyGLU",
                                    "layer_kwargs": {"activation": "Sigmoid"}, "activation": "GELU",
                                    "random_state": 2024_03_25}},
               "feature_networks": [{"type": "ConcatenateCondition", "kwargs": {"input_size": None,
                                                                               "output_size": 12}}]}


def test_anyglu_layerwise_log_prob_matches_its_own_forward():
    """tests/test_gpu_variants.py's AnyGLU coupling (Sigmoid gate), one-way: the layerwise inverse accumulates the same
    sum with torch ops; it must agree with the model's forward log-det at the draws."""
    from bcnf_amd import CondRealNVP_v2, log_prob_from_latent
    from bcnf_amd.sampling import draw
    m = CondRealNVP_v2.from_config(copy.deepcopy(GLU_ONE_WAY))
    assert type(m.fused).__name__ == "_LayerwiseStack"
    with torch.no_grad():
        for k, p in m.named_parameters():
            if k.endswith(".scale"):
                p.copy_(0.7 + 0.6 * torch.rand_like(p))
    m.to(DEV).eval()
    gen = torch.Generator().manual_seed(3)
    n, N = 6, 5
    cond = torch.randn(N, 12, generator=gen).to(DEV)
    z = torch.randn(n * N, 19, generator=gen).to(DEV)
    y, lp = draw(m, n, cond, z=z, return_log_prob=True)
    assert y.shape == (n, N, 19) and lp.shape == (n, N) and torch.equal(y, draw(m, n, cond, z=z))
    with torch.no_grad():
        m.forward(y.reshape(-1, 19), cond.repeat(n, 1), log_det_J=True)
        ldj_fwd = m.log_det_J.clone()
        y2 = m.inverse(z, cond.repeat(n, 1), log_det_J=True)
    # the couplings' per-sample variation is >= 100 x what conftest.close lets through below
    assert float(ldj_fwd.std()) >= 100 * (1e-5 * float(ldj_fwd.abs().max()) + 1e-5 * max(1.0, float(ldj_fwd.abs().max())))
    ok, err = close(m.log_det_J.cpu(), ldj_fwd.cpu())
    assert ok, ("ldj", err)
    ok, err = close(lp.reshape(-1).cpu(), log_prob_from_latent(z, ldj_fwd).cpu())
    assert ok, ("log_prob", err)
    assert torch.equal(y2, y.reshape(-1, 19))
