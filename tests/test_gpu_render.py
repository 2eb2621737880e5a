"""GPU tests of the camera kernel (bcnf_amd/csrc/bcnf_render.hip through bcnf_amd.render.render_device): the reference's
own images for the kernel's draws (tests/golden/g19_render.npz) bit for bit, integer counts against render_host on
random geometry, independence of how a batch is sliced, empty frames, visibility, empty batches and VideoBatches feeding
a videos_CNN_LSTM_large-shaped model. The fixture holds no sample within 1e-9 rad of a bin edge (its maker enforces it),
so exact equality is demanded there; on random geometry a mismatch is tolerated only at a sample render_host itself
reports inside that margin, and at most one such sample per test."""
import numpy as np
import pytest
import torch

from conftest import load_golden
from gpu_guard import DEV, canaries_alive1, guarded1

from bcnf_amd import render as R

pytestmark = pytest.mark.gpu

MARGIN = 1e-9
NAMES = ['x0_x', 'x0_y', 'x0_z', 'v0_x', 'v0_y', 'v0_z', 'g', 'w_x', 'w_y', 'w_z', 'b', 'm', 'a_x', 'a_y', 'a_z', 'r',
         'A', 'Cd', 'rho']


@pytest.fixture(scope="module")
def g19():
    return load_golden("g19_render.npz")


def fixture_batch(g):
    """Every fixture case as one sample of one camera; the cases hold 1 or 4 frames, so they are rendered per case."""
    for name in [str(n) for n in g["names"]]:
        yield name, (g[f"{name}/ball"][None], g[f"{name}/cam_pos"][None, None], g[f"{name}/angle"][None, None],
                     g[f"{name}/radius"][None]), dict(seed=int(g["seed"]), offset=int(g[f"{name}/offset"]))


def test_fixture_images_bit_for_bit(g19):
    for name, args, kw in fixture_batch(g19):
        want = g19[f"{name}/images"]
        img64, counts, n_in = R.render_device(*args, dtype=torch.float64, return_counts=True, device=DEV, **kw)
        assert img64.shape == (1, 1) + want.shape and img64.dtype == torch.float64
        assert np.array_equal(n_in[0, 0].cpu().numpy(), g19[f"{name}/n_in"]), name
        assert np.array_equal(img64[0, 0].cpu().numpy().view(np.uint64), want.view(np.uint64)), name
        img32 = R.render_device(*args, device=DEV, **kw)
        assert img32.dtype == torch.float32
        assert np.array_equal(img32[0, 0].cpu().numpy().view(np.uint32), want.astype(np.float32).view(np.uint32)), name
        assert torch.equal(counts.sum((-1, -2)), n_in)


def test_camera_and_record_trajectory_run_on_the_device(g19):
    seed = int(g19["seed"])
    film = R.record_trajectory(g19["c5/ball"], cam_pos=g19["c5/cam_pos"], radius=float(g19["c5/radius"]),
                               viewing_angle=float(g19["c5/angle"]), seed=seed, offset=int(g19["c5/offset"]))
    assert film.dtype == np.float64 and np.array_equal(film, g19["c5/images"])
    img = R.camera(g19["c1/ball"][0], cam_pos=g19["c1/cam_pos"], radius=float(g19["c1/radius"]),
                   viewing_angle=float(g19["c1/angle"]), seed=seed, offset=int(g19["c1/offset"]))
    assert img.shape == (90, 160) and np.array_equal(img, g19["c1/images"][0])


def random_geometry(seed):
    """B = 3 samples x 2 cameras x T = 5: sample 0 flies through the view, sample 1 sits on the horizontal range edge of
    camera 0 (about half of each cloud is dropped), sample 2 is far above / below the cameras (empty frames)."""
    rng = np.random.Generator(np.random.PCG64(seed))
    B, T = 3, 5
    cam_radian = np.stack([np.zeros(B), rng.uniform(0.5, 2.0, B)], 1)
    cam_pos = R.get_cams_position(cam_radian, rng.uniform(15, 30, B), rng.uniform(0.4, 1.4, (B, 2)))
    angles = rng.uniform(0.0, 8.0, (B, 2))
    angles[1, 0] = 0.0                 # a level camera: the ball below sits exactly on its range edge
    pos = np.empty((B, T, 3))
    t = np.linspace(0, 1, T)[:, None]
    pos[0] = np.array([-3.0, -2.0, 1.0]) + t * np.array([5.0, 4.0, 3.0])
    d0 = np.linalg.norm(cam_pos[1, 0, :2])
    pos[1] = np.array([0.0, d0 * np.tan(np.deg2rad(35.0)), cam_pos[1, 0, 2]]) + t * np.array([0.0, 0.0, 0.5])
    pos[2] = np.array([0.0, 0.0, 60.0]) + t * np.array([1.0, 1.0, 5.0])
    pos[2, 3:] = [0.0, 0.0, -60.0]
    radius = np.array([0.1143, 0.4, 0.2])
    return pos, cam_pos, angles, radius


@pytest.mark.parametrize("n_samples", [5000, 37])
def test_counts_against_render_host(n_samples):
    geo = random_geometry(23)
    kw = dict(n_samples=n_samples, seed=99, offset=(5 << 32) + 3, first_frame=1000)
    _, counts_h, n_h, near = R.render_host(*geo, return_counts=True, edge_margin=MARGIN, **kw)
    assert len(near) <= 1, f"the input has {len(near)} samples within {MARGIN} rad of an edge: pick another seed"
    assert n_h[0].min() > 0 and 0 < n_h[1, 0].min() and n_h[1, 0].max() < n_samples and n_h[2].max() == 0
    img, counts, n_in = R.render_device(*geo, return_counts=True, device=DEV, **kw)
    counts, n_in = counts.cpu().numpy(), n_in.cpu().numpy()
    assert counts.shape == (3, 2, 5, 90, 160) and counts.dtype == np.int32
    diff = counts.astype(np.int64) - counts_h
    if near:       # one sample may sit in a neighbouring bin, or on the other side of a range edge: only in its frame
        b, c, t = near[0][:3]
        assert np.abs(diff[b, c, t]).sum() <= 2 and abs(int(n_in[b, c, t]) - int(n_h[b, c, t])) <= 1
        diff[b, c, t] = 0
        n_in[b, c, t] = n_h[b, c, t]
    assert not diff.any() and np.array_equal(n_in, n_h)
    assert np.array_equal(counts.sum((-1, -2)), R.render_device(*geo, return_counts=True, device=DEV, **kw)[2].cpu())


def test_slices_repeats_and_offsets():
    pos, cam_pos, angles, radius = random_geometry(29)
    pos, cam_pos, angles, radius = pos[:1, :4], cam_pos[:1], np.repeat(angles[:1], 3, 1)[:, :3], radius[:1]
    cam_pos = np.concatenate([cam_pos, cam_pos[:, :1] + [0.0, 3.0, 0.5]], 1)            # 1 sample x 3 cameras x 4 = 12
    full, counts, n_in = R.render_device(pos, cam_pos, angles, radius, seed=5, offset=7, dtype=torch.float64,
                                         return_counts=True, device=DEV)
    again = R.render_device(pos, cam_pos, angles, radius, seed=5, offset=7, dtype=torch.float64, device=DEV)
    assert torch.equal(full, again)
    flat = full.reshape(12, 90, 160)
    # frames [4:9] alone: camera 1's four frames (first_frame 4) and camera 2's first (first_frame 8)
    part1 = R.render_device(pos, cam_pos[:, 1:2], angles[:, 1:2], radius, seed=5, offset=7, first_frame=4,
                            dtype=torch.float64, device=DEV)
    part2 = R.render_device(pos[:, :1], cam_pos[:, 2:3], angles[:, 2:3], radius, seed=5, offset=7, first_frame=8,
                            dtype=torch.float64, device=DEV)
    assert torch.equal(torch.cat([part1.reshape(4, 90, 160), part2.reshape(1, 90, 160)]), flat[4:9])
    other, counts2, n2 = R.render_device(pos, cam_pos, angles, radius, seed=5, offset=8, dtype=torch.float64,
                                         return_counts=True, device=DEV)
    assert not torch.equal(counts, counts2)
    for img, n in ((full, n_in), (other, n2)):
        sums = img.sum((-1, -2))
        assert bool((n > 0).all()) and float((sums - 1.0).abs().max()) <= 1e-12
    assert torch.equal(counts.sum((-1, -2)), n_in) and torch.equal(counts2.sum((-1, -2)), n2)


def test_empty_frames_and_visibility():
    geo = random_geometry(31)
    img, counts, n_in = R.render_device(*geo, return_counts=True, device=DEV)
    assert not bool(torch.isnan(img).any())
    empty = n_in == 0
    assert bool(empty[2].all()) and not bool(empty[0].any())
    assert float(img[empty].abs().max()) == 0.0 and int(counts[empty].abs().max()) == 0
    host = R.render_host(*geo)
    formula = np.array([np.sum([np.sum(cam) for cam in v]) / (len(v) * len(v[0])) for v in host])   # sampling.py:370
    for vis in (R.visibility(img), R.visibility(img, n_in=n_in)):
        assert vis.is_cuda and vis.dtype == torch.float64
        assert np.abs(vis.cpu().numpy() - formula).max() <= 1e-12         # a lit float64 frame sums to 1 within 1e-13
    assert formula[0] == pytest.approx(1.0, abs=1e-12) and formula[2] == 0.0


def test_output_stays_inside_its_buffers():
    """The raw entry point on guarded buffers: every image / count / n_in element written, nothing outside."""
    from bcnf_amd import _native as N
    pos, cam_pos, angles, radius = random_geometry(37)
    F = 7                                           # sample 0's camera-0 frames, then two frames of an invalid camera
    ball = torch.from_numpy(np.concatenate([pos[0], pos[0, :2]])).to(DEV)
    cam_index = torch.tensor([0, 0, 0, 0, 0, 5, -1], dtype=torch.int32, device=DEV)
    sigma = torch.full((F,), 0.1143 / R.COVERAGE, dtype=torch.float64, device=DEV)
    ph, th = R.bin_edges()
    d = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(DEV)  # noqa: E731
    ibuf, iview = guarded1(F * 14400)
    cbuf, cview = guarded1(F * 14400, dtype=torch.int32)
    nbuf, nview = guarded1(F, dtype=torch.int32)
    N.call("bcnf_render_frames", ball, cam_index, sigma, F, d(cam_pos[0, :1]), d(R.camera_basis(cam_pos[0, :1],
           angles[0, :1])), 1, d(ph), d(th), 5000, 1, 2, 3, iview, False, cview, nview, N.stream_handle(torch.device(DEV)))
    torch.cuda.synchronize()
    assert canaries_alive1(ibuf, F * 14400) and canaries_alive1(cbuf, F * 14400) and canaries_alive1(nbuf, F)
    assert nview.tolist()[5:] == [-1, -1] and min(nview.tolist()[:5]) > 0
    assert float(iview[5 * 14400:].abs().max()) == 0.0 and int((cview == 0x5A5A5A5A).sum()) == 0
    want = R.render_device(pos[:1], cam_pos[:1, :1], angles[:1, :1], radius[:1], seed=1, offset=2, first_frame=3, device=DEV)
    assert torch.equal(iview[:5 * 14400].view(5, 90, 160), want[0, 0])
    assert N.call_raw("bcnf_render_frames", ball, cam_index, sigma, F, d(cam_pos[0, :1]), d(R.camera_basis(
        cam_pos[0, :1], angles[0, :1])), 1, d(ph), d(th), 5000, 1, 2, 2**32 - 3, iview, False, cview, nview,
        N.stream_handle(torch.device(DEV))) == N.ERR_UNSUPPORTED


def test_empty_batches():
    for B, T in ((0, 5), (2, 0)):
        img, counts, n_in = R.render_device(np.zeros((B, T, 3)), np.zeros((B, 2, 3)), np.zeros((B, 2)), np.ones(B),
                                            return_counts=True, device=DEV)
        assert img.shape == counts.shape == (B, 2, T, 90, 160) and n_in.shape == (B, 2, T)
        assert img.is_cuda and img.dtype == torch.float32 and img.numel() == 0


def test_video_batches_feed_a_videos_model():
    from bcnf_amd import CondRealNVP_v2, VideoBatches
    vb = VideoBatches(n_pool=4, batch=2, device=DEV)
    y, videos, tail = vb.next_batch()
    assert videos.shape == (2, 2, 30, 90, 160) and videos.dtype == torch.float32 and videos.is_cuda
    assert tail.shape == (2, 7) and tail.dtype == torch.float32 and y.shape == (2, 19)
    sums = vb.videos.sum((-1, -2))
    assert bool(((sums - 1.0).abs() <= 1e-5).logical_or(sums == 0).all()) and float(sums.max()) > 0.5
    assert bool((tail[:, 0] == 0).all())                       # camera 1 sits at radian 0
    online = VideoBatches(n_pool=4, batch=2, device=DEV, online=True)
    a = online.next_batch()[1]
    assert online.offset == 1 and a.shape == (2, 2, 30, 90, 160) and online.videos is None
    cfg = {"global": {"parameter_selection": NAMES},
           "model": {"kwargs": {"size": 19, "nested_sizes": [32], "n_conditions": 1367, "n_blocks": 2,
                                "dropout": 0.407, "act_norm": True}},
           "feature_networks": [
               {"type": "ConcatenateCondition", "kwargs": {"input_size": None, "output_size": [90, 160]}},
               {"type": "CNN", "kwargs": {"hidden_channels": [8, 16, 32], "kernel_sizes": [8, 5, 3],
                                          "strides": [1, 1, 1], "dropout_prob": 0.5, "image_input_size": [90, 160],
                                          "output_size_lin": 1000, "output_size": 1000}},
               {"type": "LSTM", "kwargs": {"input_size": 1000, "hidden_size": 212, "output_size": 1360,
                                           "num_layers": 2, "dropout": 0.111, "bidirectional": True,
                                           "pooling": "mean", "pool_dim": 1}},
               {"type": "ConcatenateCondition", "kwargs": {"input_size": 1360, "output_size": 1367, "dim": -1}}]}
    torch.manual_seed(19)
    model = CondRealNVP_v2.from_config(cfg).to(DEV).eval()
    with torch.no_grad():
        z = model(y, videos, tail, log_det_J=True)
    assert z.shape == (2, 19) and bool(torch.isfinite(z).all()) and bool(torch.isfinite(model.log_det_J).all())
