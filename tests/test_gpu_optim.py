"""GPU tests of the kernels that run on every training step, driven through the C ABI directly: the optimizer
(k_adam<1>, k_adam<2>, k_sumsq, k_clip, k_sum_partials), the bookkeeping and guard kernels (k_advance,
k_guard_global, the last-workgroup bookkeeping of k_adam, the guard[HALTED] no-op of every kernel) and the batch
gather (k_gather2 / gather2_rows).

The reference is tests/optim_ref.py: float64 restatements of torch's Adam and clip_grad_norm_, pinned to torch's own
float64 results by tests/test_optim_ref_cpu.py. Adam is held to max(1, 2 x the error of torch's fp32 CPU Adam on the
same inputs) in the project's tolerance units (optim_ref.units); everything the code claims to be bit-exact is
compared bit for bit. Every tensor, partials buffer, norm, log and gather destination sits between NaN canaries.

Sum of squares, the bound used below (u = 2^-24, every term non-negative, so an addition's rounding error is at
most u of the running sum and k roundings cost at most k u to first order): a thread's chain is EPT * G fused
multiply-adds (the square is exact inside the fma: one rounding each), the workgroup tree 8 levels, so one partial
is within (4 G + 8) u of its float64 value, and so is the float64 sum of the partials. k_clip then sums at most
ceil(nparts / 256) partials per thread and 8 tree levels: nparts <= 2048 gives (4 G + 8 + 8 + 8) u <= 32 u on the
sum, half of it plus one rounding of the square root on the norm, 17 u = 1.01e-6: capped at the project's 1e-6.
Pre-reduced (nparts > 2048), k_sum_partials adds 3 roundings per 16-byte quad and one per accumulate, 8 for its
accumulators, ceil(tail / 1024) for the tail (unaligned: ceil(nparts / 1024) for the scalar loop, counted on top),
6 shuffle levels and 16 wave sums; k_clip's single read adds nothing but its 8 (exact) tree levels are counted:
(4 G + 8) + (4 + 8 + 3 + 6 + 16) + 8 <= 61 u on the sum, 31.5 u = 1.9e-6 on the norm, below the project's 1e-5.
"""
import ctypes
import functools
import math

import numpy as np
import pytest
import torch

import optim_ref as R
from gpu_guard import DEV, GUARD, canaries_alive, canaries_alive1, guarded, guarded1

pytestmark = pytest.mark.gpu

U = 2.0 ** -24
OK, ERR_ARG, ERR_UNSUPPORTED = 0, 1, 2
HALTED, DIVERGED_ONLY = [0, 0, 1, 0], [1, 1, 0, 0]


@pytest.fixture(scope="module")
def N():
    from bcnf_amd import _native
    _native.lib()
    return _native


def stream(N):
    return N.stream_handle(torch.device(DEV, torch.cuda.current_device()))


def sync():
    torch.cuda.synchronize()


def groups(total):
    return 2 if total >= 1 << 22 else 1


def workgroups(total):
    return max(1, -(-total // (R.CHUNK * groups(total))))


def sum_bound(total):
    """Relative bound on the float64 sum of the partials, and on the norm k_clip reports (module docstring)."""
    part = (4 * groups(total) + 8) * U
    if workgroups(total) <= 2048:
        return part, min(0.5 * (part + 16 * U) + U, 1e-6)
    return part, min(0.5 * (part + (4 + 8 + 3 + 6 + 16 + 8) * U) + U, 1e-5)


def bits(t):
    return t.contiguous().view(torch.int32) if t.dtype == torch.float32 else t


def same_bits(a, b):
    return a.shape == b.shape and torch.equal(bits(a), bits(b))


def ptr_array(ptrs):
    arr = (ctypes.c_void_p * max(1, len(ptrs)))()
    for i, q in enumerate(ptrs):
        arr[i] = q or None
    return arr


class Arr:
    """One of p / g / m / v of a tensor list: every tensor in its own 256-byte aligned slot of one NaN-filled buffer,
    `offs[t]` floats into the slot, GUARD NaNs at least between neighbours. A zero-length tensor has a (non-NULL)
    address of its own."""

    def __init__(self, sizes, offs, flat):
        self.sizes, self.pos, cur = list(sizes), [], GUARD
        for n, o in zip(sizes, offs):
            self.pos.append(cur + o)
            cur += -(-(o + n) // 64) * 64 + GUARD
        host = np.full(cur, np.nan, dtype=np.float32)
        outside = np.ones(cur, dtype=bool)
        k = 0
        for s, n in zip(self.pos, sizes):
            host[s:s + n] = flat[k:k + n]
            outside[s:s + n] = False
            k += n
        self.buf = torch.from_numpy(host).to(DEV)
        self.outside = torch.from_numpy(outside).to(DEV)
        assert self.buf.data_ptr() % 256 == 0

    def ptrs(self):
        return [self.buf.data_ptr() + 4 * s for s in self.pos]

    def flat(self):
        return torch.cat([self.buf[s:s + n] for s, n in zip(self.pos, self.sizes)])

    def set(self, flat):
        src = torch.from_numpy(np.array(flat)).to(DEV)       # a copy: the cached inputs are read-only
        k = 0
        for s, n in zip(self.pos, self.sizes):
            self.buf[s:s + n] = src[k:k + n]
            k += n

    def alive(self):
        return bool(torch.isnan(self.buf[self.outside]).all()) and bool(torch.isfinite(self.buf[~self.outside]).all())


class TSet:
    """A tensor list on the device with its step count (in a guarded buffer). sizes: element counts; offsets: per
    tensor (p, g, m, v) float offsets from the 16-byte grid; lo, hi: the slice of the list's concatenated inputs."""

    def __init__(self, sizes, offsets=None, step0=0, lo=0, hi=None, total=None):
        total = sum(sizes) if total is None else total
        hi = total if hi is None else hi
        assert sum(sizes) == hi - lo
        offsets = offsets or [(0, 0, 0, 0)] * len(sizes)
        p, m, v = (a[lo:hi] for a in R.state_inputs(total))
        g = R.grad_inputs(total, 0)[lo:hi]
        self.sizes, self.total, self.lo, self.hi, self.n_all = list(sizes), hi - lo, lo, hi, total
        self.p, self.g, self.m, self.v = (Arr(sizes, [o[i] for o in offsets], a)
                                          for i, a in enumerate((p, g, m, v)))
        self.step_buf, self.step = guarded1(1, [float(step0)])

    @classmethod
    def of(cls, name, step0=0):
        return cls(R.LISTS[name], R.VIEW_OFFSETS if name == "views" else None, step0)

    def grads(self, launch):
        self.g.set(R.grad_inputs(self.n_all, launch)[self.lo:self.hi])

    def arrays(self, which="pgmv"):
        return [getattr(self, c) for c in which]

    def snapshot(self):
        return [a.buf.clone() for a in self.arrays()] + [self.step_buf.clone()]

    def unchanged(self, snap):
        return all(same_bits(a, b) for a, b in zip(self.snapshot(), snap))

    def alive(self):
        return all(a.alive() for a in self.arrays()) and canaries_alive1(self.step_buf, 1)


def hyper(wd=0.0, betas=R.BETAS[0]):
    return (R.LR, betas[0], betas[1], R.EPS, wd)


def partials(N, total, offset=0):
    """(buffer, view, workgroups): a NaN-filled partials buffer of exactly bcnf_grad_partials(total) floats."""
    n = int(N.call_raw("bcnf_grad_partials", total))
    assert n == workgroups(total) + 1
    buf, view = guarded1(n, offset=offset)
    return buf, view, n - 1


def adam(N, S, hyp, part=None, advance=1, guard=None, n=None, null=()):
    ptrs = [[0 if t in null else q for t, q in enumerate(a.ptrs())] for a in S.arrays()]
    return N.call_raw("bcnf_adam_step", len(S.sizes) if n is None else n, *(ptr_array(q) for q in ptrs),
                      N.i64_array(S.sizes), S.step, *hyp, part, advance, guard, stream(N))


def bookkeep(N, S, hyp, cursor, modulo, logv, logh, done, guard=None, n=None):
    return N.call_raw("bcnf_adam_step_bookkeep", len(S.sizes) if n is None else n,
                      *(ptr_array(a.ptrs()) for a in S.arrays()), N.i64_array(S.sizes), S.step, *hyp, cursor, modulo,
                      logv, logh, done, guard, stream(N))


def sumsq(N, S, part, n=None, null=()):
    ptrs = [0 if t in null else q for t, q in enumerate(S.g.ptrs())]
    return N.call_raw("bcnf_grad_sumsq", len(S.sizes) if n is None else n, ptr_array(ptrs), N.i64_array(S.sizes),
                      part, stream(N))


def clip(N, S, part, max_norm, norm=None, step=None, cursor=None, modulo=0, logv=None, logh=None, guard=None, n=None,
         null=()):
    ptrs = [0 if t in null else q for t, q in enumerate(S.g.ptrs())]
    return N.call_raw("bcnf_clip_grad_norm", len(S.sizes) if n is None else n, ptr_array(ptrs), N.i64_array(S.sizes),
                      part, max_norm, norm, step, cursor, modulo, logv, logh, guard, stream(N))


def i32(values):
    return torch.tensor(values, dtype=torch.int32, device=DEV)


# ------------------------------------------------------------------------------------------ 1. fp64 accuracy
@pytest.mark.parametrize("name,wd,betas,step0", R.adam_cases())
def test_adam_against_float64(N, name, wd, betas, step0):
    """p, exp_avg, exp_avg_sq after one launch and after three (fresh gradients each) against adam64, within
    max(1, 2 x torch fp32 CPU Adam's error on the same inputs) units. Launches 1 and 3 advance the step count
    themselves, launch 2 leaves it to the clip that follows: it is step0 + launches after each."""
    S = TSet.of(name, step0)
    ref = R.reference(S.total, wd, betas, step0)
    ref_err = R.torch_fp32_errors(S.total, wd, betas, step0)
    pb, pv, nwg = partials(N, S.total)
    for k in range(3):
        S.grads(k)
        assert adam(N, S, hyper(wd, betas), pv, advance=int(k != 1)) == OK
        if k == 1:
            assert clip(N, S, pv, 1.0, step=S.step) == OK
        sync()
        assert S.step.item() == step0 + k + 1
        if k == 1:
            continue
        for what, arr, want in zip("pmv", S.arrays("pmv"), ref[k]):
            err = R.units(arr.flat().cpu().numpy(), want, what)
            bound = max(1.0, 2.0 * ref_err[(k + 1, what)])
            print(f"{name} wd={wd} betas={betas} step0={step0} launches={k + 1} {what}: kernel {err:.3f} "
                  f"torch-fp32 {ref_err[(k + 1, what)]:.3f} bound {bound:.3f}")
            assert err <= bound, (what, k + 1, err, bound)
    assert S.alive() and canaries_alive1(pb, nwg + 1, written=False)
    assert bool(torch.isfinite(pv[:nwg]).all())
    assert bool(torch.isnan(pv[nwg])) == (nwg <= 2048)      # the pre-reduce slot: only a pre-reducing clip writes it


# --------------------------------------------------------------------------------- 2. layout invariance
@pytest.mark.parametrize("name", ["seams", "views"])
def test_adam_is_layout_invariant(N, name):
    """The list's elements as the given tensors (seams, views off the 16-byte grid: element path) and as one aligned
    tensor (vector path): identical p, m, v and partials, adam_elem rounding alike on both paths."""
    hyp = hyper(0.01, R.BETAS[1])
    A, B = TSet.of(name, 7), TSet([sum(R.LISTS[name])], step0=7)
    pa, pb = partials(N, A.total)[1], partials(N, B.total)[1]
    for k in range(2):
        A.grads(k), B.grads(k)
        assert adam(N, A, hyp, pa) == OK and adam(N, B, hyp, pb) == OK
    sync()
    for a, b in zip(A.arrays("pmv"), B.arrays("pmv")):
        assert same_bits(a.flat(), b.flat())
    assert same_bits(pa[:-1], pb[:-1]) and A.alive() and B.alive()


def test_adam_two_groups_equal_one_group(N):
    """g2_ragged as given (two groups per thread; its last workgroup has a 3-element group 0 and an empty group 1)
    and as two calls below 2^22 elements (one group per thread), same step count: identical p, m, v."""
    sizes, hyp = R.LISTS["g2_ragged"], hyper(0.01, R.BETAS[0])
    total, h = sum(sizes), 2_100_001
    A = TSet.of("g2_ragged", 7)
    B1, B2 = TSet([h], step0=7, lo=0, hi=h, total=total), TSet([total - h], step0=7, lo=h, hi=total, total=total)
    assert groups(A.total) == 2 and groups(B1.total) == groups(B2.total) == 1
    for S in (A, B1, B2):
        assert adam(N, S, hyp, None, advance=0) == OK
    sync()
    for c in "pmv":
        got = getattr(A, c).flat()
        want = torch.cat([getattr(B1, c).flat(), getattr(B2, c).flat()])
        assert same_bits(got, want), (c, int((bits(got) != bits(want)).sum()))
    assert A.step.item() == B1.step.item() == 7.0 and A.alive() and B1.alive() and B2.alive()


# --------------------------------------------------------------------------------------- 3. partials and clip
@functools.lru_cache(maxsize=None)
def clip_reference(total, max_norm):
    g = R.grad_inputs(total, 0)
    norm, coef, (clipped,) = R.clip64([g], max_norm)
    return R.sumsq64([g]), norm, coef, clipped


@functools.lru_cache(maxsize=None)
def partials64(total):
    """float64 sum of squares of each workgroup's G * CHUNK elements (the last one ragged)."""
    per = R.CHUNK * groups(total)
    sq = np.zeros(workgroups(total) * per)
    sq[:total] = R.grad_inputs(total, 0).astype(np.float64) ** 2
    return sq.reshape(-1, per).sum(1)


@pytest.mark.parametrize("max_norm", [1.0, 1e30])
@pytest.mark.parametrize("name", list(R.LISTS))
def test_partials_and_clip_against_float64(N, name, max_norm):
    """bcnf_adam_step's partials == bcnf_grad_sumsq's bit for bit; their float64 sum and the clip's norm against
    sumsq64 / clip64 within the bounds of the module docstring; every gradient against g64 coef64 (rtol 1e-6, pre-
    reduced lists 1e-5), bit-identical at coef = 1; two runs give the same bits."""
    ss64, norm64, coef64, clipped64 = clip_reference(sum(R.LISTS[name]), max_norm)
    runs = []
    for _ in range(2):
        S = TSet.of(name)
        g0 = S.g.flat().clone()
        ab, av, nwg = partials(N, S.total)
        sb, sv, _ = partials(N, S.total)
        nb, nv = guarded1(1)
        assert adam(N, S, hyper(), av) == OK and sumsq(N, S, sv) == OK
        sync()
        assert same_bits(av[:nwg], sv[:nwg]) and bool(torch.isnan(sv[nwg]))
        assert canaries_alive1(ab, nwg + 1, written=False)
        part_bound, norm_bound = sum_bound(S.total)
        each = sv[:nwg].double().cpu().numpy()
        assert np.all(np.abs(each - partials64(S.total)) <= part_bound * partials64(S.total))   # the ragged last too
        ss = float(each.sum())
        assert abs(ss - ss64) <= part_bound * ss64, (ss, ss64)
        assert clip(N, S, sv, max_norm, nv) == OK
        sync()
        got = S.g.flat()
        if not runs:
            print(f"{name} max_norm={max_norm}: sum rel err {abs(ss - ss64) / ss64:.3e} (bound {part_bound:.3e}), "
                  f"norm rel err {abs(nv.item() - norm64) / norm64:.3e} (bound {norm_bound:.3e})")
        assert abs(nv.item() - norm64) <= norm_bound * norm64, (nv.item(), norm64)
        if max_norm == 1e30:
            assert coef64 == 1.0 and same_bits(got, g0)
        else:
            rtol = 1e-6 if nwg <= 2048 else 1e-5
            d = (got.cpu().double().numpy() - clipped64)
            assert np.all(np.abs(d) <= rtol * np.abs(clipped64)), float(np.max(np.abs(d)))
        assert bool(torch.isnan(sv[nwg])) == (nwg <= 2048)
        assert S.alive() and canaries_alive1(sb, nwg + 1, written=False) and canaries_alive1(nb, 1)
        runs.append((got.clone(), nv.clone(), sv.clone(), S.p.flat()))
    assert all(same_bits(a, b) for a, b in zip(*runs))


def test_clip_over_unaligned_partials(N):
    """prereduce_g1 with its partials one float off the 16-byte grid: k_sum_partials' scalar loop gives the norm
    within the same bound, and writes nothing around the buffer."""
    S = TSet.of("prereduce_g1")
    _, norm64, _, _ = clip_reference(S.total, 1.0)
    sb, sv, nwg = partials(N, S.total, offset=1)
    assert nwg == 2051 and sv.data_ptr() % 16 == 4
    nb, nv = guarded1(1)
    assert sumsq(N, S, sv) == OK and clip(N, S, sv, 1.0, nv) == OK
    sync()
    print(f"unaligned partials: norm rel err {abs(nv.item() - norm64) / norm64:.3e}")
    assert abs(nv.item() - norm64) <= (sum_bound(S.total)[1] + 1.5 * U) * norm64    # + ceil(2051 / 1024) = 3 roundings
    assert canaries_alive1(sb, nwg + 1, offset=1) and canaries_alive1(nb, 1) and S.alive()


# ----------------------------------------------------------------------------------------- refusals, tensor count
def test_tensor_count_refusals_write_nothing(N):
    """48 tensors run (test_adam_against_float64[max_tensors]); 49 and 0 are BCNF_ERR_ARG from every entry point, with
    nothing written."""
    S = TSet.of("max_tensors")
    pb, pv, _ = partials(N, S.total)
    nb, nv = guarded1(1)
    db, done = guarded1(1, [0], dtype=torch.int32)
    snap = S.snapshot()
    for n in (0, 49):
        T49 = _with_count(S, n)
        assert adam(N, T49, hyper(), pv, n=n) == ERR_ARG
        assert bookkeep(N, T49, hyper(), None, 0, None, None, done, n=n) == ERR_ARG
        assert sumsq(N, T49, pv, n=n) == ERR_ARG
        assert clip(N, T49, pv, 1.0, nv, n=n) == ERR_ARG
    sync()
    assert S.unchanged(snap) and bool(torch.isnan(pv).all()) and bool(torch.isnan(nv).all()) and done.item() == 0
    assert canaries_alive1(pb, pv.numel(), written=False) and canaries_alive1(db, 1)


class _with_count:
    """S's arrays with the pointer and size lists cut or padded (with the first tensor's) to n entries, so that a
    call that wrongly accepted n tensors would still see valid pointers."""

    def __init__(self, S, n):
        self.step = S.step
        self.sizes = (S.sizes + S.sizes)[:max(n, 1)]
        self._arrs = [_Ptrs((a.ptrs() + a.ptrs())[:max(n, 1)]) for a in S.arrays()]
        self.g = self._arrs[1]

    def arrays(self, which="pgmv"):
        return [self._arrs["pgmv".index(c)] for c in which]


class _Ptrs:
    def __init__(self, ptrs):
        self._ptrs = ptrs

    def ptrs(self):
        return self._ptrs


# -------------------------------------------------------------------------------------- 4. bookkeeping equivalence
def log_values(k):
    return torch.tensor([k + 0.5, -(k + 0.25), 100.0 * k + 0.125], dtype=torch.float32, device=DEV)


@pytest.mark.parametrize("modulo", [1, 2, 5])
@pytest.mark.parametrize("name", ["one_wg_1024", "seams", "prereduce_g1"])
def test_bookkeep_equals_adam_plus_clip(N, name, modulo):
    """Three bcnf_adam_step_bookkeep launches (done_counter untouched in between) == three x (bcnf_adam_step without
    the step advance + bcnf_clip_grad_norm with step, cursor and log), from equal states, the cursor starting at
    modulo - 1: p, m, v, step, cursor and log_history bit for bit; done_counter 0 after every launch; the row of the
    cursor before the launch holds that launch's values, every other row stays NaN; the cursor wraps to 0."""
    hyp, step0 = hyper(0.01), 7
    out = []
    for fused in (True, False):
        S = TSet.of(name, step0)
        cb, cur = guarded1(1, [modulo - 1], dtype=torch.int64)
        hb, hist = guarded(modulo, 3)
        db, done = guarded1(1, [0], dtype=torch.int32)
        pb, pv, nwg = partials(N, S.total)
        want_hist = torch.full((modulo, 3), float("nan"))
        want_cur = modulo - 1
        for k in range(3):
            S.grads(k)
            lv = log_values(k)
            if fused:
                assert bookkeep(N, S, hyp, cur, modulo, lv, hist, done) == OK
            else:
                assert adam(N, S, hyp, pv, advance=0) == OK
                assert clip(N, S, pv, 1.0, None, S.step, cur, modulo, lv, hist) == OK
            sync()
            want_hist[want_cur] = lv.cpu()
            want_cur = (want_cur + 1) % modulo
            assert done.item() == 0 and cur.item() == want_cur and S.step.item() == step0 + k + 1
            assert same_bits(hist.cpu(), want_hist)
        assert cur.item() == (modulo - 1 + 3) % modulo
        assert S.alive() and canaries_alive1(cb, 1) and canaries_alive1(db, 1)
        assert bool(torch.isnan(hb[:GUARD]).all()) and bool(torch.isnan(hb[GUARD + 3 * modulo:]).all())
        out.append([a.flat() for a in S.arrays("pmv")] + [S.step.clone(), cur.clone(), hist.clone()])
    assert all(same_bits(a, b) for a, b in zip(*out))


@pytest.mark.parametrize("fused", [True, False])
def test_bookkeeping_nullable_operands_and_refusals(N, fused):
    """cursor NULL: row 0 is written; log NULL: the history is untouched; a cursor with cursor_modulo < 1, and a NULL
    done_counter, are BCNF_ERR_ARG with nothing written."""
    S = TSet.of("seams", 3)
    hb, hist = guarded(2, 3)
    db, done = guarded1(1, [0], dtype=torch.int32)
    cb, cur = guarded1(1, [1], dtype=torch.int64)
    pb, pv, nwg = partials(N, S.total)
    assert sumsq(N, S, pv) == OK
    sync()
    lv = log_values(4)

    def run(cursor, modulo, logv, logh, counter=done):
        if fused:
            return bookkeep(N, S, hyper(), cursor, modulo, logv, logh, counter)
        return clip(N, S, pv, 1e30, None, S.step, cursor, modulo, logv, logh)

    snap, hsnap = S.snapshot(), hb.clone()
    for modulo in (0, -1):
        assert run(cur, modulo, lv, hist) == ERR_ARG
    if fused:
        assert run(cur, 2, lv, hist, counter=None) == ERR_ARG
    sync()
    assert S.unchanged(snap) and same_bits(hb, hsnap) and cur.item() == 1 and done.item() == 0
    assert run(None, 0, lv, hist) == OK                       # no cursor: row 0, and its modulo is not looked at
    sync()
    assert torch.equal(hist[0], lv) and bool(torch.isnan(hist[1]).all()) and cur.item() == 1 and S.step.item() == 4
    hsnap = hb.clone()
    for logv, logh in ((None, hist), (log_values(5), None), (None, None)):
        assert run(cur, 2, logv, logh) == OK
    sync()
    assert same_bits(hb, hsnap) and cur.item() == 0 and S.step.item() == 7 and done.item() == 0
    assert S.alive() and canaries_alive1(cb, 1) and canaries_alive1(db, 1)


@pytest.mark.parametrize("modulo", [1, 2, 5])
def test_advance_counters(N, modulo):
    """bcnf_advance_counters: step only, cursor only (from modulo - 1: wraps to 0, then counts up), both, both NULL
    (a no-op that returns OK); n_batches < 1 with a cursor is refused and changes nothing."""
    sb, step = guarded1(1, [41.0])
    cb, cur = guarded1(1, [modulo - 1], dtype=torch.int64)
    st = stream(N)
    assert N.call_raw("bcnf_advance_counters", step, None, 0, st) == OK
    sync()
    assert step.item() == 42.0 and cur.item() == modulo - 1
    want = modulo - 1
    for _ in range(modulo + 1):
        assert N.call_raw("bcnf_advance_counters", None, cur, modulo, st) == OK
        sync()
        want = (want + 1) % modulo
        assert cur.item() == want and step.item() == 42.0
    assert N.call_raw("bcnf_advance_counters", step, cur, modulo, st) == OK
    sync()
    assert step.item() == 43.0 and cur.item() == (want + 1) % modulo
    before = cur.item()
    assert N.call_raw("bcnf_advance_counters", None, None, 0, st) == OK
    for bad in (0, -3):
        assert N.call_raw("bcnf_advance_counters", step, cur, bad, st) == ERR_ARG
    sync()
    assert step.item() == 43.0 and cur.item() == before
    assert canaries_alive1(sb, 1) and canaries_alive1(cb, 1)


# ---------------------------------------------------------------------------------------------------- 5. guard
@pytest.mark.parametrize("name", ["seams", "prereduce_g1"])
def test_halted_step_changes_nothing(N, name):
    """guard = [0, 0, 1, 0]: bcnf_adam_step (both advance_step values), bcnf_adam_step_bookkeep and
    bcnf_clip_grad_norm (direct and pre-reduced) leave p, g, m, v, step, cursor, the NaN-filled partials (pre-reduce
    slot included), total_norm, log_history and done_counter bitwise unchanged."""
    S = TSet.of(name, 7)
    guard = i32(HALTED)
    pb, pv, nwg = partials(N, S.total)
    nb, nv = guarded1(1)
    hb, hist = guarded(2, 3)
    cb, cur = guarded1(1, [1], dtype=torch.int64)
    db, done = guarded1(1, [0], dtype=torch.int32)
    lv = log_values(1)
    snap = S.snapshot()
    assert adam(N, S, hyper(0.01), pv, advance=1, guard=guard) == OK
    assert adam(N, S, hyper(0.01), pv, advance=0, guard=guard) == OK
    assert bookkeep(N, S, hyper(0.01), cur, 2, lv, hist, done, guard=guard) == OK
    assert clip(N, S, pv, 1.0, nv, S.step, cur, 2, lv, hist, guard=guard) == OK
    sync()
    assert S.unchanged(snap) and S.step.item() == 7.0 and cur.item() == 1 and done.item() == 0
    assert bool(torch.isnan(pb).all()) and bool(torch.isnan(nb).all()) and bool(torch.isnan(hb).all())
    assert canaries_alive1(cb, 1) and canaries_alive1(db, 1) and torch.equal(guard, i32(HALTED))


@pytest.mark.parametrize("name", ["seams", "prereduce_g1"])
def test_diverged_but_not_halted_step_runs_as_without_guard(N, name):
    out = []
    for g in (None, DIVERGED_ONLY):
        S = TSet.of(name, 7)
        guard = None if g is None else i32(g)
        pb, pv, nwg = partials(N, S.total)
        nb, nv = guarded1(1)
        assert adam(N, S, hyper(0.01), pv, advance=0, guard=guard) == OK
        assert clip(N, S, pv, 1.0, nv, S.step, guard=guard) == OK
        sync()
        assert S.step.item() == 8.0 and (guard is None or torch.equal(guard, i32(g)))
        out.append([a.flat() for a in S.arrays()] + [nv.clone(), pv.clone()])
    assert all(same_bits(a, b) for a, b in zip(*out))


LOSSES = [0.0, 1e5, float(np.nextafter(np.float32(1e5), np.float32(np.inf))), float("nan"), float("inf"),
          float("-inf"), -1e30]


@pytest.mark.parametrize("guard0", [[0, 0, 0, 1], [0, 0, 0, 0], [0, 0, 1, 1], [1, 0, 0, 1], [1, 1, 0, 1]])
@pytest.mark.parametrize("loss", LOSSES)
def test_guard_check_global(N, loss, guard0):
    """DIVERGED is raised exactly for loss > 1e5 or NaN (1e5 itself is not, the next fp32 is) with CHECK_GLOBAL on
    and the step not halted; no other guard word ever changes, and the values are only read."""
    gb, guard = guarded1(4, guard0, dtype=torch.int32)
    vb, vals = guarded1(3, [loss, 2e5, float("nan")])
    assert N.call_raw("bcnf_guard_check_global", vals, guard, stream(N)) == OK
    sync()
    raised = guard0[3] == 1 and guard0[2] == 0 and (math.isnan(loss) or np.float32(loss) > np.float32(1e5))
    want = list(guard0)
    want[1] = 1 if raised else guard0[1]
    assert guard.tolist() == want and canaries_alive1(gb, 4)
    assert same_bits(vals, torch.tensor([loss, 2e5, float("nan")], device=DEV))
    assert canaries_alive1(vb, 3, written=False)


def test_guard_check_global_refuses_null(N):
    guard, vals = i32([0, 0, 0, 1]), torch.full((3,), 2e5, device=DEV)
    assert N.call_raw("bcnf_guard_check_global", None, guard, stream(N)) == ERR_ARG
    assert N.call_raw("bcnf_guard_check_global", vals, None, stream(N)) == ERR_ARG
    sync()
    assert guard.tolist() == [0, 0, 0, 1]


# -------------------------------------------------------------------------------------------------- 6. gathers
def gather_inputs(n, c0, c1, seed):
    gen = torch.Generator().manual_seed(seed)
    rows = n + 37
    s0 = torch.randn(rows, c0, generator=gen).to(DEV)
    s1 = torch.randn(rows, c1, generator=gen).to(DEV)
    idx = torch.randint(0, rows, (n,), generator=gen)
    idx[n // 2:] = idx[:n - n // 2].flip(0)                  # repeats, out of order
    if n:
        idx[0] = rows - 1
    return s0, s1, idx.to(DEV)


@pytest.mark.parametrize("c0,c1", [(1, 1), (3, 90), (19, 1), (7, 8)])
@pytest.mark.parametrize("n", [1, 2, 511, 512, 513, 1025, 4099])
def test_gather_rows2(N, n, c0, c1):
    """dst0 == src0[idx], dst1 == src1[idx] exactly, at the 512-workgroup plan edge and with several rows per
    workgroup; nothing outside the destinations is written."""
    s0, s1, idx = gather_inputs(n, c0, c1, 1000 * n + c0)
    b0, d0 = guarded(n, c0)
    b1, d1 = guarded(n, c1)
    assert N.call_raw("bcnf_gather_rows2", idx, n, s0, c0, d0, s1, c1, d1, stream(N)) == OK
    sync()
    assert torch.equal(d0, s0[idx]) and torch.equal(d1, s1[idx])
    assert canaries_alive(b0, n, c0) and canaries_alive(b1, n, c1)


def test_gather_rows2_refusals(N):
    s0, s1, idx = gather_inputs(8, 7, 8, 1)
    b0, d0 = guarded(8, 7)
    b1, d1 = guarded(8, 8)
    st = stream(N)
    g = functools.partial(N.call_raw, "bcnf_gather_rows2")
    assert g(idx, 0, s0, 7, d0, s1, 8, d1, st) == OK
    assert g(None, 0, None, 7, None, None, 8, None, st) == OK           # n = 0: nothing is looked at
    assert g(idx, -1, s0, 7, d0, s1, 8, d1, st) == ERR_ARG
    assert g(idx, 8, s0, 0, d0, s1, 8, d1, st) == ERR_ARG
    assert g(idx, 8, s0, 7, d0, s1, -2, d1, st) == ERR_ARG
    for k in range(5):
        ops = [idx, s0, d0, s1, d1]
        ops[k] = None
        assert g(ops[0], 8, ops[1], 7, ops[2], ops[3], 8, ops[4], st) == ERR_ARG
    # 32-bit index math: n (cols0 + cols1) >= 2^31 returns before any launch (status only; dummy buffers)
    assert g(idx, 1 << 27, s0, 8, d0, s1, 8, d1, st) == ERR_UNSUPPORTED
    sync()
    assert bool(torch.isnan(b0).all()) and bool(torch.isnan(b1).all())


@pytest.mark.parametrize("batch", [1, 48, 513])
def test_gather_batch(N, batch):
    """Batch cursor[0] of an epoch order of 5 batches, for every cursor 0..4; the gather does not advance it."""
    c0, c1 = 19, 90
    s0, s1, order = gather_inputs(5 * batch, c0, c1, batch)
    for c in range(5):
        cb, cur = guarded1(1, [c], dtype=torch.int64)
        b0, d0 = guarded(batch, c0)
        b1, d1 = guarded(batch, c1)
        assert N.call_raw("bcnf_gather_batch", order, cur, batch, s0, c0, d0, s1, c1, d1, stream(N)) == OK
        sync()
        rows = order[c * batch:(c + 1) * batch]
        assert torch.equal(d0, s0[rows]) and torch.equal(d1, s1[rows]) and cur.item() == c
        assert canaries_alive(b0, batch, c0) and canaries_alive(b1, batch, c1) and canaries_alive1(cb, 1)
    st = stream(N)
    g = functools.partial(N.call_raw, "bcnf_gather_batch")
    b0, d0 = guarded(batch, c0)
    b1, d1 = guarded(batch, c1)
    cur = torch.zeros(1, dtype=torch.int64, device=DEV)
    assert g(order, cur, 0, s0, c0, d0, s1, c1, d1, st) == ERR_ARG
    assert g(order, cur, -1, s0, c0, d0, s1, c1, d1, st) == ERR_ARG
    assert g(order, None, batch, s0, c0, d0, s1, c1, d1, st) == ERR_ARG
    assert g(None, cur, batch, s0, c0, d0, s1, c1, d1, st) == ERR_ARG
    sync()
    assert bool(torch.isnan(b0).all()) and bool(torch.isnan(b1).all())


# ----------------------------------------------------------------------------------------------- 7. empty sets
@pytest.mark.parametrize("sizes", [[0], [0, 0, 0]])
def test_empty_set(N, sizes):
    """Every numel 0, NULL tensor pointers: the four entry points return OK, partial 0 and total_norm are 0, and the
    step, cursor and log bookkeeping happen as usual. No address into a tensor can be formed: there is none."""
    n = len(sizes)
    null = ptr_array([0] * n)
    numel = N.i64_array(sizes)
    st = stream(N)
    assert N.call_raw("bcnf_grad_partials", 0) == 2
    sb, step = guarded1(1, [7.0])
    cb, cur = guarded1(1, [1], dtype=torch.int64)
    db, done = guarded1(1, [0], dtype=torch.int32)
    hb, hist = guarded(2, 3)
    nb, nv = guarded1(1)
    for advance in (1, 0):
        pb, pv = guarded1(2)
        assert N.call_raw("bcnf_adam_step", n, null, null, null, null, numel, step, *hyper(0.01), pv, advance, None,
                          st) == OK
        sync()
        assert pv[0].item() == 0.0 and bool(torch.isnan(pv[1])) and canaries_alive1(pb, 2, written=False)
    assert step.item() == 8.0
    assert N.call_raw("bcnf_adam_step_bookkeep", n, null, null, null, null, numel, step, *hyper(0.01), cur, 2,
                      log_values(1), hist, done, None, st) == OK
    sync()
    assert step.item() == 9.0 and cur.item() == 0 and done.item() == 0
    assert torch.equal(hist[1], log_values(1)) and bool(torch.isnan(hist[0]).all())
    pb, pv = guarded1(2)
    assert N.call_raw("bcnf_grad_sumsq", n, null, numel, pv, st) == OK
    sync()
    assert pv[0].item() == 0.0 and bool(torch.isnan(pv[1]))
    assert N.call_raw("bcnf_clip_grad_norm", n, null, numel, pv, 1.0, nv, step, cur, 2, log_values(2), hist, None,
                      st) == OK
    sync()
    assert nv.item() == 0.0 and step.item() == 10.0 and cur.item() == 1 and torch.equal(hist[0], log_values(2))
    assert bool(torch.isnan(pv[1])) and canaries_alive1(pb, 2, written=False)
    assert all(canaries_alive1(b, 1) for b in (sb, cb, db, nb)) and canaries_alive(hb, 2, 3)


def test_null_empty_tensor_inside_a_list(N):
    """seams' zero-length tensor with a NULL pointer is accepted, and the results equal the list without it, bit for
    bit; a NULL pointer of a tensor with elements is still refused."""
    sizes = R.LISTS["seams"]
    z = sizes.index(0)
    A, B = TSet.of("seams", 7), TSet(sizes[:z] + sizes[z + 1:], step0=7)
    out = []
    for S, null in ((A, (z,)), (B, ())):
        pb, pv, nwg = partials(N, S.total)
        nb, nv = guarded1(1)
        assert adam(N, S, hyper(0.01), pv, null=null) == OK
        assert clip(N, S, pv, 1.0, nv, null=null) == OK
        sb, sv, _ = partials(N, S.total)
        assert sumsq(N, S, sv, null=null) == OK
        sync()
        assert S.alive() and canaries_alive1(pb, nwg + 1, written=False)
        out.append([a.flat() for a in S.arrays()] + [pv[:nwg].clone(), nv.clone(), sv[:nwg].clone(), S.step.clone()])
    assert all(same_bits(a, b) for a, b in zip(*out))
    snap = A.snapshot()
    pb, pv, _ = partials(N, A.total)
    assert adam(N, A, hyper(), pv, null=(0,)) == ERR_ARG and sumsq(N, A, pv, null=(3,)) == ERR_ARG
    assert clip(N, A, pv, 1.0, None, null=(3,)) == ERR_ARG
    sync()
    assert A.unchanged(snap) and bool(torch.isnan(pv).all())


def test_fused_adam_with_an_empty_parameter():
    """FusedAdam over [w, an empty tensor] with gradients on both, then clip_grad_norm_after_step: no error, and w,
    its moments, its clipped gradient and the norm equal FusedAdam([w])'s exactly. optim.clip_grad_norm_ likewise."""
    from bcnf_amd.optim import FusedAdam, clip_grad_norm_
    n = 3000
    p0, g0 = (torch.from_numpy(a.copy()).to(DEV) for a in (R.state_inputs(n)[0], R.grad_inputs(n, 0)))
    out = []
    for empty in (True, False):
        w = p0.clone().requires_grad_()
        w.grad = g0.clone()
        params = [w]
        if empty:
            e = torch.zeros(0, device=DEV, requires_grad=True)
            e.grad = torch.zeros(0, device=DEV)
            params.append(e)
        opt = FusedAdam(params, lr=R.LR, weight_decay=0.01)
        opt.step(defer_step_count=True)
        norm = opt.clip_grad_norm_after_step(1.0)
        w2 = p0.clone().requires_grad_()
        w2.grad = g0.clone()
        norm2 = clip_grad_norm_([w2] + params[1:], 1.0)
        sync()
        st = opt.state[w]
        assert float(st["step"]) == 1.0
        out.append([w.detach().clone(), st["exp_avg"], st["exp_avg_sq"], w.grad, norm.reshape(1), w2.grad,
                    norm2.reshape(1)])
    assert all(same_bits(a, b) for a, b in zip(*out))
    assert not torch.equal(out[0][0], p0)
