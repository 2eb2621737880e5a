"""Posterior draws with their log-density (bcnf_stack_inverse_logdet / bcnf_wide_inverse_logdet, sample / draw with
return_log_prob=True), the parts that need no GPU: the density is refused -- before any launch -- where the inverse is
not the forward's inverse (two_way, cnf.py:198-213) or not deterministic (train mode with dropout); the C entry points
validate their arguments before any HIP call; draw_sharded gathers a (draws, log_prob) pair like a single tensor."""
import ctypes
import os
import socket

import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp


def _model(two_way=False, dropout=0.0, nested=(16, 16)):
    from bcnf_amd import CondRealNVP_v2
    cfg = {"global": {"parameter_selection": [f"p{i}" for i in range(19)]},
           "model": {"kwargs": {"size": 19, "nested_sizes": list(nested), "n_conditions": 24, "n_blocks": 3,
                                "dropout": dropout, "act_norm": True, "two_way": two_way}},
           "feature_networks": [{"type": "ConcatenateCondition", "kwargs": {"input_size": None, "output_size": 24}}]}
    torch.manual_seed(3)
    return CondRealNVP_v2.from_config(cfg)


def _calls(m):
    from bcnf_amd.sampling import draw, posterior_mode
    z, c = torch.zeros(5, 19), torch.zeros(5, 24)
    return {
        "inverse": lambda: m.inverse(z, c, log_det_J=True),
        "sample": lambda: m.sample(4, c, outer=True, return_log_prob=True),
        "draw": lambda: draw(m, 4, c, return_log_prob=True),
        "posterior_mode": lambda: posterior_mode(m, 4, c),
    }


@pytest.mark.parametrize("nested", [(16, 16), (40, 40)], ids=["small-shaped", "wide"])
@pytest.mark.parametrize("call", ["inverse", "sample", "draw", "posterior_mode"])
def test_two_way_has_no_density(call, nested):
    m = _model(two_way=True, nested=nested).eval()           # CPU tensors: a launch would raise RuntimeError instead
    with pytest.raises(ValueError, match="two_way"):
        _calls(m)[call]()


@pytest.mark.parametrize("nested", [(16, 16), (40, 40)], ids=["small", "wide"])
@pytest.mark.parametrize("call", ["inverse", "sample", "draw", "posterior_mode"])
def test_train_mode_with_dropout_has_no_density(call, nested):
    m = _model(dropout=0.3, nested=nested).train()
    with pytest.raises(ValueError, match="dropout"):
        _calls(m)[call]()


def test_stack_level_checks_raise_before_the_launch():
    """launch_inverse(want_ldj=True) itself refuses (a caller that bypasses the model), again before touching tensors."""
    z, h = torch.zeros(5, 19), torch.zeros(5, 24)
    for m in (_model(two_way=True, nested=(40, 40)).eval(), ):
        with pytest.raises(ValueError, match="two_way"):
            m.fused.launch_inverse(z, h, want_ldj=True)
    for nested in ((16, 16), (40, 40)):
        with pytest.raises(ValueError, match="dropout"):
            _model(dropout=0.3, nested=nested).fused.launch_inverse(z, h, training=True, want_ldj=True)


def test_entry_points_validate_before_any_device_call():
    """No GPU here: a HIP call would return BCNF_ERR_HIP_BASE + hipError, not these statuses."""
    from bcnf_amd import _native as N
    L = N.lib()
    host = (ctypes.c_float * 64)()
    p = ctypes.cast(host, ctypes.c_void_p)                       # never dereferenced: the calls return first
    i64 = ctypes.c_int64
    for nested, fn, extra in (((16, 16), L.bcnf_stack_inverse_logdet, ()), ((40, 40), L.bcnf_wide_inverse_logdet, (p,))):
        two = N.make_desc(19, list(nested), 3, 24, act_norm=True, two_way=True)
        one = N.make_desc(19, list(nested), 3, 24, act_norm=True)
        args = lambda d, y, ldj: (ctypes.byref(d), *extra, p, p, p, i64(2), None, i64(2), y, ldj, None, p, None)
        assert fn(*args(two, p, p)) == N.ERR_UNSUPPORTED
        assert fn(*args(two, None, None)) == N.ERR_UNSUPPORTED
        assert fn(*args(one, p, None)) == N.ERR_ARG
        assert fn(*args(one, None, p)) == N.ERR_ARG
        assert fn(None, *extra, p, p, p, i64(2), None, i64(2), p, p, None, p, None) == N.ERR_ARG
        # n_rows == 0 is a no-op; rows without cond_index need h_rows == n_rows
        assert fn(ctypes.byref(one), *extra, p, p, p, i64(2), None, i64(0), p, p, None, p, None) == N.OK
        assert fn(ctypes.byref(one), *extra, p, p, p, i64(3), None, i64(2), p, p, None, p, None) == N.ERR_ARG


# ------------------------------------------------------------------------------------------ draw_sharded with a pair
def _free_port():
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        return s.getsockname()[1]


def _pair_sampler(c):
    # deterministic per condition: draw s of condition row c -> c.sum() * (s + 1); its "log_prob" -> -c.sum() - s
    s = torch.arange(1, 4, dtype=torch.float32).view(3, 1, 1)
    base = c.sum(dim=(1, 2))
    y = (base.view(1, -1, 1) * s).expand(3, c.shape[0], 19).contiguous()
    lp = -base.view(1, -1) - torch.arange(3, dtype=torch.float32).view(3, 1)
    return y, lp


def _worker(rank, world, port, q):
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        from bcnf_amd.sampling import draw_sharded
        cond = torch.arange(7 * 30 * 3, dtype=torch.float32).view(7, 30, 3)
        out = draw_sharded(None, 3, cond, sampler=_pair_sampler)
        local = draw_sharded(None, 3, cond, sampler=_pair_sampler, gather=False)
        ry, rlp = _pair_sampler(cond)
        ok = (isinstance(out, tuple) and len(out) == 2 and torch.equal(out[0], ry) and torch.equal(out[1], rlp)
              and out[1].shape == (3, 7))
        q.put((rank, ok, (tuple(local[0].shape), tuple(local[1].shape))))
    except Exception as e:  # pragma: no cover
        q.put((rank, repr(e), None))
    finally:
        dist.destroy_process_group()


@pytest.mark.parametrize("world", [2, 3])
def test_draw_sharded_gathers_draws_and_log_prob(world):
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = _free_port()
    procs = [ctx.Process(target=_worker, args=(r, world, port, q)) for r in range(world)]
    for p in procs:
        p.start()
    res = sorted(q.get(timeout=120) for _ in procs)
    for p in procs:
        p.join(timeout=60)
    from bcnf_amd.sampling import shard_range
    for rank, ok, shapes in res:
        assert ok is True, ok
        a, b = shard_range(7, rank, world)
        assert shapes == ((3, b - a, 19), (3, b - a))


def test_draw_sharded_single_process_passes_a_pair_through():
    from bcnf_amd.sampling import draw_sharded
    cond = torch.arange(5 * 30 * 3, dtype=torch.float32).view(5, 30, 3)
    y, lp = draw_sharded(None, 3, cond, sampler=_pair_sampler)
    ry, rlp = _pair_sampler(cond)
    assert torch.equal(y, ry) and torch.equal(lp, rlp)


def test_posterior_mode_is_exported():
    import bcnf_amd
    from bcnf_amd.sampling import posterior_mode
    assert bcnf_amd.posterior_mode is posterior_mode and "posterior_mode" in bcnf_amd.__all__
