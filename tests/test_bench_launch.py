"""bench.py's multi-rank launcher on CPU: `python bench.py --gpus 2` started directly (no WORLD_SIZE) must run two
ranks through torch.distributed.run as a child process, and every rank must see a world of 2 (gloo here; the
GPU box uses the same path with RCCL)."""
import json
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _run(*extra, env=None):
    e = dict(os.environ)
    for k in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "MASTER_PORT"):
        e.pop(k, None)
    e.update(env or {})
    return subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), *extra], capture_output=True, text=True,
                          timeout=240, env=e, cwd=ROOT)


@pytest.mark.timeout(300)
def test_gpus2_launches_two_ranks():
    r = _run("--gpus", "2", "--launch-check")
    assert r.returncode == 0, r.stderr[-2000:]
    lines = [json.loads(x) for x in r.stdout.splitlines() if x.startswith("{")]
    assert len(lines) == 1, r.stdout          # ONE JSON line, from rank 0
    assert lines[0]["n_gpus"] == 2 and lines[0]["ranks_seen"] == 2 and lines[0]["backend"] == "gloo"
    # every sub-line of the default run (configs[2] - [4], re-simulation) runs on both ranks at world 2
    from bench import SUBLINES
    sub = lines[0]["secondary"]
    assert list(sub) == [wl for wl, _ in SUBLINES]
    for wl, res in sub.items():
        assert "error" not in res, (wl, res)
        assert res["ranks_seen"] == 2 and res["n_gpus"] == 2, (wl, res)


def test_dump_outputs_types_budget_and_fixed_sample(tmp_path, monkeypatch):
    """--dump-outputs: float64 stays float64, everything else becomes float32; arrays within the budget are written
    whole; one beyond its share is cut to a sample that is the same in every run and fills the share."""
    import numpy as np
    import torch
    import bench
    monkeypatch.setattr(bench, "DUMP_BUDGET_BYTES", 4096)
    rng = np.random.Generator(np.random.PCG64(5))
    small = rng.standard_normal(3)                                   # float64, 24 bytes
    half = torch.from_numpy(rng.standard_normal((7, 11))).to(torch.float16)
    big = rng.standard_normal((50, 41)).astype(np.float32)          # 8200 bytes > what is left
    for d in ("a", "b"):
        bench.dump_outputs(str(tmp_path / d), [("small", small), ("half", half), ("big", big)])
    a = {n: np.load(tmp_path / "a" / f"{n}.npy") for n in ("small", "half", "big")}
    b = {n: np.load(tmp_path / "b" / f"{n}.npy") for n in ("small", "half", "big")}
    assert sorted(p.name for p in (tmp_path / "a").iterdir()) == ["big.npy", "half.npy", "small.npy"]
    assert a["small"].dtype == np.float64 and np.array_equal(a["small"], small)
    assert a["half"].dtype == np.float32 and np.array_equal(a["half"], half.float().numpy())
    assert a["big"].dtype == np.float32 and a["big"].ndim == 1
    assert sum(p.stat().st_size for p in (tmp_path / "a").iterdir()) <= 4096       # the files, headers included
    assert a["big"].nbytes > 4096 - 3 * 128 - 24 - 7 * 11 * 4 - 4   # the sample uses what is left of the budget
    flat = big.reshape(-1)
    assert np.isin(a["big"], flat).all() and len(set(a["big"].tolist())) == a["big"].size
    for n in a:
        assert np.array_equal(a[n], b[n]), n


def test_plain_run_is_the_default_and_full_is_an_option(monkeypatch):
    import bench
    monkeypatch.setattr(sys, "argv", ["bench.py", "--gpus", "1", "--steps", "3", "--warmup", "2"])
    args = bench.parse()
    assert args.full is False and args.dump_outputs is None and args.steps == 3 and args.warmup == 2
    monkeypatch.setattr(sys, "argv", ["bench.py", "--full", "--dump-outputs", "somewhere"])
    args = bench.parse()
    assert args.full is True and args.dump_outputs == "somewhere"


@pytest.mark.timeout(120)
def test_gpus_disagreeing_with_world_size_fails():
    r = _run("--gpus", "2", "--launch-check", env={"WORLD_SIZE": "1", "RANK": "0", "LOCAL_RANK": "0"})
    assert r.returncode != 0 and "WORLD_SIZE=1" in r.stderr
