"""CPU tests of bcnf_amd.render: the package's own Philox and draw rule, the camera geometry against the reference's
(tests/golden/g19_render.npz, written by tests/golden/make_golden_render.py), and render_host against the reference's
camera() fed the same draws. The fixture holds no sample within 1e-9 rad of a bin edge, so images are compared bit for
bit."""
import numpy as np
import pytest

from conftest import load_golden
from dropout_ref import philox4x32_10 as philox_ref

from bcnf_amd import render as R


@pytest.fixture(scope="module")
def g19():
    return load_golden("g19_render.npz")


def cases(g):
    return [str(n) for n in g["names"]]


def host_case(g, name, **kw):
    return R.render_host(g[f"{name}/ball"][None], g[f"{name}/cam_pos"][None, None], g[f"{name}/angle"][None, None],
                         g[f"{name}/radius"][None], seed=int(g["seed"]), offset=int(g[f"{name}/offset"]), **kw)


def test_philox_equals_the_dropout_restatement():
    rng = np.random.Generator(np.random.PCG64(19))
    c = rng.integers(0, 2**32, size=(6, 4096), dtype=np.uint64)
    got = R.philox4x32_10(*c)
    want = philox_ref(*c)
    for a, b in zip(got, want):
        assert np.array_equal(a, b)
    # the Random123 known-answer vector for an all-ones-bits counter and key
    kat = R.philox4x32_10(0xFFFFFFFF, 0xFFFFFFFF, 0xFFFFFFFF, 0xFFFFFFFF, 0xFFFFFFFF, 0xFFFFFFFF)
    assert [int(v) for v in kat] == [0x408F276D, 0x41C83B0E, 0xA20BC7C6, 0x6D5451FD]


def test_standard_normals_are_deterministic_and_keyed():
    a = R.standard_normals(7, 3, 11, 4096)
    assert a.shape == (4096, 3) and a.dtype == np.float64 and np.isfinite(a).all()
    assert np.array_equal(a, R.standard_normals(7, 3, 11, 4096))
    assert np.array_equal(a[:100], R.standard_normals(7, 3, 11, 100))          # a prefix of a longer draw
    for other in (R.standard_normals(7, 3, 12, 4096), R.standard_normals(7, 4, 11, 4096),
                  R.standard_normals(8, 3, 11, 4096), R.standard_normals(7 + 2**32, 3, 11, 4096),
                  R.standard_normals(7, 3 + 2**32, 11, 4096)):
        assert not np.array_equal(a, other)
        assert abs(np.corrcoef(a.ravel(), other.ravel())[0, 1]) < 0.05
    both = R.standard_normals(7, 3, np.array([11, 12]), 64)                     # an array of frames
    assert np.array_equal(both[0], a[:64]) and np.array_equal(both[1], R.standard_normals(7, 3, 12, 64))


def test_standard_normals_moments():
    """Mean, variance and the 90 % mass inside +-1.644854 (camera.py:113) over 1e6 draws, each within 4 standard errors:
    se(mean) = 1 / sqrt(n), se(variance) = sqrt(2 / n), se(share) = sqrt(0.9 0.1 / n)."""
    z = R.standard_normals(2024, 0, np.arange(4), 83334).reshape(-1)[:1_000_000]
    n = z.size
    assert n == 1_000_000
    assert abs(z.mean()) <= 4.0 / np.sqrt(n)
    assert abs(z.var() - 1.0) <= 4.0 * np.sqrt(2.0 / n)
    assert abs((np.abs(z) < 1.644854).mean() - 0.9) <= 4.0 * np.sqrt(0.09 / n)
    comps = R.standard_normals(2024, 1, 0, 200_000)                             # the three components are uncorrelated
    assert np.abs(np.corrcoef(comps.T) - np.eye(3)).max() <= 4.0 / np.sqrt(200_000)


def test_camera_basis_is_bit_identical(g19):
    names = cases(g19)
    for name in names:
        got = R.camera_basis(g19[f"{name}/cam_pos"], g19[f"{name}/angle"])
        assert got.dtype == np.float64 and np.array_equal(got.view(np.uint64), g19[f"{name}/basis"].view(np.uint64)), name
    pos = np.stack([g19[f"{n}/cam_pos"] for n in names]).reshape(1, len(names), 3)        # batched: the same bits
    ang = np.stack([g19[f"{n}/angle"] for n in names]).reshape(1, len(names))
    want = np.stack([g19[f"{n}/basis"] for n in names])[None]
    assert np.array_equal(R.camera_basis(pos, ang).view(np.uint64), want.view(np.uint64))


def test_get_cams_position_is_bug_compatible(g19):
    rad, cr, hh, want = (g19[f"cams/{k}"] for k in ("radiants", "radius", "heights", "pos"))
    got = R.get_cams_position(rad, cr, hh)
    assert got.shape == (3, 2, 3) and np.array_equal(got.view(np.uint64), want.view(np.uint64))
    for i in range(3):
        assert np.array_equal(R.get_cams_position(rad[i], cr[i], hh[i]), want[i])
    # the swapped arguments, explicitly: camera 0 takes its HEIGHT from radiants[1], camera 1 its RADIANT from heights[0]
    p = R.get_cams_position(np.array([0.0, 1.2]), 25, np.array([1.5, 2.5]))
    assert np.array_equal(p[0], [-25.0 * np.cos(0.0), 25.0 * np.sin(0.0), 1.2])
    assert np.array_equal(p[1], [-25.0 * np.cos(1.5), 25.0 * np.sin(1.5), 2.5])
    assert np.allclose(p, [[-25, 0, 1.2], [-1.76843004, 24.93737467, 2.5]], rtol=0, atol=1e-8)
    with pytest.raises(ValueError, match="too many values to unpack"):
        R.get_cams_position(np.zeros(3), 25, np.zeros(3))
    with pytest.raises(ValueError, match="not enough values to unpack"):
        R.get_cams_position(np.zeros(1), 25, np.zeros(1))


def test_render_host_equals_the_reference_bit_for_bit(g19):
    lit = {}
    for name in cases(g19):
        img, counts, n_in, near = host_case(g19, name, return_counts=True, edge_margin=float(g19["margin"]))
        want = g19[f"{name}/images"]
        assert near == [], name                                   # the maker's condition still holds here
        assert img.dtype == np.float64 and img.shape == (1, 1) + want.shape
        assert np.array_equal(img[0, 0].view(np.uint64), want.view(np.uint64)), name
        assert np.array_equal(n_in[0, 0], g19[f"{name}/n_in"]) and np.array_equal(counts.sum((-1, -2)), n_in)
        lit[name] = int((want > 0).sum())
    assert lit["c2"] == 0 and lit["c4"] == 0 and lit["c1"] > 1000 and 0 < lit["c0"] < 50      # the cases are what they say
    assert 0 < int(g19["c6/n_in"][0]) < 5000 and int(g19["c3/n_in"][0]) == 5000


def test_camera_and_record_trajectory_follow_the_reference(g19):
    seed = int(g19["seed"])
    for name in ("c0", "c2", "c6"):
        img = R.camera(g19[f"{name}/ball"][0], (16, 9), 70.0, g19[f"{name}/cam_pos"], False, float(g19[f"{name}/radius"]),
                       float(g19[f"{name}/angle"]), seed=seed, offset=int(g19[f"{name}/offset"]), device="cpu")
        assert img.shape == (90, 160) and img.dtype == np.float64
        assert np.array_equal(img, g19[f"{name}/images"][0])
        s = img.sum()
        assert s == 0.0 if int(g19[f"{name}/n_in"][0]) == 0 else abs(s - 1.0) <= 1e-12
    film = R.record_trajectory(g19["c5/ball"], cam_pos=g19["c5/cam_pos"], radius=float(g19["c5/radius"]),
                               viewing_angle=float(g19["c5/angle"]), seed=seed, offset=int(g19["c5/offset"]),
                               device="cpu")
    assert film.shape == (4, 90, 160) and film.dtype == np.float64 and np.array_equal(film, g19["c5/images"])
    assert np.abs(film.sum((1, 2)) - 1.0).max() <= 1e-12
    default = R.camera(device="cpu")                              # the reference's defaults: the ball is in view
    assert default.shape == (90, 160) and abs(default.sum() - 1.0) <= 1e-12
    with pytest.raises(NotImplementedError):
        R.record_trajectory(g19["c5/ball"], make_gif=True, device="cpu")
    small = R.render_host(np.zeros((1, 2, 3)), np.array([[[-25.0, 0, 1.5]]]), np.zeros((1, 1)), np.array([0.1]),
                          ratio=(4, 3), n_samples=100)
    assert small.shape == (1, 1, 2, 30, 40)


def test_render_device_refuses_the_cpu():
    with pytest.raises(RuntimeError, match="HIP device only"):
        R.render_device(np.zeros((1, 1, 3)), np.zeros((1, 1, 3)), np.zeros((1, 1)), np.ones(1), device="cpu")


def test_visibility_counts_lit_frames():
    import torch
    videos = torch.zeros(2, 2, 3, 90, 160)
    videos[0, 0, 1, 5, 7] = 1.0
    videos[0, 1, 2, 0, 0] = 0.5
    videos[0, 1, 2, 89, 159] = 0.5
    vis = R.visibility(videos)
    host = np.array([sum(float(cam.sum()) for cam in v) / (len(v) * len(v[0])) for v in videos.numpy()])
    assert vis.dtype == torch.float64 and np.array_equal(vis.numpy(), host) and host[0] == 2 / 6
    n_in = torch.tensor([[[0, 9, 0], [0, 0, 5000]], [[0, 0, 0], [0, 0, 0]]], dtype=torch.int32)
    assert torch.equal(R.visibility(None, n_in=n_in), vis)
