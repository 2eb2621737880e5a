"""GPU tests of the record reads of the D = 19 stacks and of the folded tail's Gx sum.

A D = 19 stack (D_a = 10, D_b = 9) keeps Linear 1's y-part, the mix and the backward's T / S head transposes in
broadcast form: the live words of such a section are its first 10, 38 and 9, the rest of its rotation-form size is dead.
k_forward and k_backward (the BC instantiations) read only the live words, and k_backward stages only the quads that
hold one, so the dead words of its LDS ring keep whatever the ring held before.

 * Against the fp64 oracle (oracle/cnf_oracle.py, fed the kernels' own masks in training mode, as
   tests/test_gpu_train_parity.py does) at the gates of tests/test_gpu_parity.py: z and log|det J| `close` at 1e-5, the
   loss 1e-5 |ref| + 1e-5, every gradient `close(rtol=1e-4, floor=1e-4)`. D = 19 with 1, 2, 3 blocks (a lone block has
   no ActNorm and an identity mix; with 2 the backward's two-deep pipeline holds the whole stack before its first
   barrier; 3 is the first with a steady-state interval), nested sizes [16] and [16] * 7 (the staging of 2 and of 3
   float4 per helper thread), B = 1 and 17 (one workgroup with 15 padded rows; two workgroups), C = 13 (one ragged
   column tile), training and eval, unfolded (m() + autograd, and nll_loss without the fold) and folded. The
   training-mode inverse (k_inverse) against the oracle's and as a round trip at one of the shapes.
 * One stack of size 20 (10 / 10: rotation form, the other instantiation of every kernel) at B = 17, same gates.
 * No dead word is read: the same steps with every CU's LDS filled with NaN and then with 1e30 (bcnf_lds_fill), before
   the step and, in the unfolded step, again between the forward and the backward, give the same bits.
 * Gx sum (k_fold_gx): fold == unfolded at the gates of tests/test_gpu_fold.py with one block and B = 1, 129, 2049,
   4100 -- 1, 2, 17 and 33 split-K partials per element: the remainder loop alone, one round of 16 loads plus one
   split, two rounds plus one."""
import copy
import ctypes
import types

import numpy as np
import pytest
import torch

from conftest import FC_SMALL_CFG, close
from dropout_ref import apply_gain, fold_config
from oracle import cnf_oracle as O
from test_gpu_train_parity import (DEV, INV_TAG, OFFSET, _perturb, _small_keep, check, compare, gpu_run, oracle_run,
                                   small_seed)

pytestmark = pytest.mark.gpu

C, X = 13, 21                       # conditions; in_features of the folded feature Linear (a 7 x 3 trajectory)
PATHS = ("unfused", "fused", "folded")
_CASES = {}


def _case(D, NH, nb, B):
    """A stack behind one feature Linear [X, C] on the GPU, in train mode at its seed, with its inputs: every path of
    gpu_run applies to it (unfused / fused run the Linear on its own, folded folds it in)."""
    from bcnf_amd import CondRealNVP_v2
    key = (D, NH, nb, B)
    if key in _CASES:
        return _CASES[key]
    shape = dict(size=D, nested_sizes=[16] * NH, n_blocks=nb, n_conditions=C, dropout=0.25, act_norm=True)
    torch.manual_seed(7)
    m = CondRealNVP_v2.from_config(fold_config(shape, X))
    _perturb(m)
    if NH >= 6:
        apply_gain(m, 2.0)          # dropout_ref.apply_gain: keeps the deepest gradients above their gate's floor
    spec = O.StackSpec(size=D, nested_sizes=shape["nested_sizes"], n_blocks=nb, n_conditions=C, dropout=0.25,
                       act_norm=True, feature_sizes=[X, C])
    sd = {k: v.detach().clone() for k, v in m.state_dict().items()}
    g = torch.Generator().manual_seed(1000 + B)
    y = torch.randn(B, D, generator=g)
    cond = torch.randn(B, X // 3, 3, generator=g)
    case = types.SimpleNamespace(name=f"d{D}_nh{NH}_nb{nb}-B{B}", m=m, spec=spec, sd=sd, y=y, cond=cond,
                                 seed=small_seed(B), wide=False)
    m.to(DEV).train()
    assert type(m.fused).__name__ == "FusedStack"
    m.fused.set_seed(case.seed)
    _CASES[key] = case
    return case


def _refs(case):
    """The fp64 references of the case, computed once: the training step under the launch's masks, the eval step."""
    if not hasattr(case, "refs"):
        B = case.y.shape[0]
        case.refs = {True: oracle_run(case, _small_keep(case, OFFSET, B)),
                     False: oracle_run(case, None, training=False)}
    return case.refs


def _fill(value):
    from bcnf_amd import _native as N
    dev = torch.device("cuda", torch.cuda.current_device())
    N.check(N.lib().bcnf_lds_fill(ctypes.c_float(value), N.stream_handle(dev)), "bcnf_lds_fill")


BC_CASES = [(NH, nb, B) for NH in (1, 7) for nb in (1, 2, 3) for B in (1, 17)]


@pytest.mark.parametrize("NH,nb,B", BC_CASES, ids=[f"nh{NH}-nb{nb}-B{B}" for NH, nb, B in BC_CASES])
def test_broadcast_form_vs_fp64_oracle(NH, nb, B):
    case = _case(19, NH, nb, B)
    for training in (True, False):
        for path in PATHS:
            rows = compare(gpu_run(case, path, training=training), _refs(case)[training])
            check(case, f"{path}-{'train' if training else 'eval'}", rows)


def test_rotation_form_vs_fp64_oracle():
    case = _case(20, 3, 3, 17)
    for training in (True, False):
        for path in PATHS:
            rows = compare(gpu_run(case, path, training=training), _refs(case)[training])
            check(case, f"{path}-{'train' if training else 'eval'}", rows)


def test_training_mode_inverse_vs_fp64_oracle_and_round_trip():
    """k_inverse<7> (model.train(); model.inverse()) at D = 19, 3 blocks, B = 17: against the oracle's inverse under
    the launch's masks (tag 0x40000000) at 1e-5, and as a round trip -- the oracle's fp64 forward under those masks,
    then the kernel back to y -- at the 1e-4 of tests/test_gpu_parity.py's round trip."""
    case = _case(19, 7, 3, 17)
    m, st, spec, B = case.m, case.m.fused, case.spec, 17
    sd64 = {k: v.double() for k, v in case.sd.items()}
    h64 = O.feature_forward(sd64, spec, case.cond.double())
    keep = _small_keep(case, OFFSET, B, INV_TAG)
    zl = torch.randn(B, spec.size, generator=torch.Generator().manual_seed(B))
    with torch.no_grad():
        ref = O.model_inverse(sd64, spec, zl.double(), h64, training=True, keep=keep)
        z_of_y, _ = O.model_forward(sd64, spec, case.y.double(), h64, training=True, keep=keep)
    m.train()
    out = []
    for z in (zl, z_of_y.float()):
        st.rng_state()[1] = OFFSET
        with torch.no_grad():
            out.append(m.inverse(z.to(DEV), case.cond.to(DEV)).cpu())
        assert int(st.rng_state()[1].item()) == OFFSET + 1
    ok, err = close(out[0], ref)
    assert ok, err
    ok, err = close(out[1], case.y, rtol=1e-4, floor=1e-4)
    assert ok, err


def _bits(out):
    """Every tensor a gpu_run exposes, as int32 words in a fixed order."""
    ts = [out[k] for k in ("z", "ldj", "loss", "dy", "dh") if out.get(k) is not None]
    ts += [out["grads"][k] for k in sorted(out["grads"])]
    return torch.cat([t.detach().cpu().float().reshape(-1).view(torch.int32) for t in ts])


DEAD_CASES = [(19, 1, 1, 17), (19, 7, 2, 1), (19, 7, 3, 17), (20, 3, 3, 17)]


@pytest.mark.parametrize("D,NH,nb,B", DEAD_CASES, ids=[f"d{D}-nh{NH}-nb{nb}-B{B}" for D, NH, nb, B in DEAD_CASES])
def test_no_dead_word_is_read(D, NH, nb, B):
    case = _case(D, NH, nb, B)
    got = {}
    for value in (float("nan"), 1e30):
        parts = []
        for training in (True, False):
            for path in PATHS:
                _fill(value)
                parts.append(_bits(gpu_run(case, path, training=training)))
        parts.append(_bits(_unfolded_step_filled_twice(case, value)))
        got[value] = torch.cat(parts)
        assert torch.isfinite(got[value].view(torch.float32)).all()
    assert torch.equal(*got.values())


def _unfolded_step_filled_twice(case, value):
    """m() + inn_nll_loss + autograd in train mode with the LDS filled before the forward and again before the
    backward: what k_backward's ring holds where it stages nothing is then the fill, not the forward's records."""
    from bcnf_amd import inn_nll_loss
    m, st = case.m, case.m.fused
    m.train()
    m.zero_grad(set_to_none=True)
    st.rng_state()[1] = OFFSET
    y = case.y.to(DEV).requires_grad_(True)
    _fill(value)
    z = m(y, case.cond.to(DEV), log_det_J=True)
    loss = inn_nll_loss(z, m.log_det_J)
    _fill(value)
    loss.backward()
    out = dict(z=z, ldj=m.log_det_J, loss=loss, dy=y.grad,
               grads={n: p.grad.detach().clone() for n, p in m.named_parameters() if p.grad is not None})
    m.zero_grad(set_to_none=True)
    return out


def _fold_grads(m, y, traj, fold, seed):
    m.fold_features = fold
    m.zero_grad(set_to_none=True)
    m.fused.flat_param.grad = None
    m.fused.set_seed(seed)
    vals = m.nll_loss(y, traj)
    torch.autograd.backward(vals, torch.tensor([1.0, 0.0, 0.0], device=DEV))
    lin = m.feature_network_stack.feature_networks[1].nn[0]
    return vals.detach().clone(), m.fused.flat_param.grad.clone(), lin.weight.grad.clone(), lin.bias.grad.clone()


@pytest.fixture(scope="module")
def one_block_model():
    from bcnf_amd import CondRealNVP_v2
    cfg = copy.deepcopy(FC_SMALL_CFG)
    cfg["model"]["kwargs"]["n_blocks"] = 1
    torch.manual_seed(3)
    m = CondRealNVP_v2.from_config(cfg)
    m.to(DEV).train()
    m.flat_parameters()
    return m


@pytest.mark.parametrize("B", [1, 129, 2049, 4100])
def test_gx_sum_fold_equals_unfolded(one_block_model, B):
    m = one_block_model
    assert -(-B // 128) in (1, 2, 17, 33)                           # split-K partials per Gx element (KC = 128 rows)
    gen = torch.Generator().manual_seed(B)
    y = torch.randn(B, 19, generator=gen).to(DEV)
    traj = torch.randn(B, 30, 3, generator=gen).to(DEV)
    assert m._foldable_linear(y, (traj,)) is not None
    v1, g1, w1, b1 = _fold_grads(m, y, traj, True, 1234)
    v0, g0, w0, b0 = _fold_grads(m, y, traj, False, 1234)
    del m.fold_features
    assert abs(v1[0].item() - v0[0].item()) <= 2e-6 * abs(v0[0].item()) + 1e-6
    for a, b, what in ((g1, g0, "stack"), (w1, w0, "feature W"), (b1, b0, "feature b")):
        ok, err = close(a.cpu(), b.cpu(), rtol=1e-4, floor=1e-5)
        assert ok, (what, err)
        assert float(b.abs().max()) > 0.0, what
