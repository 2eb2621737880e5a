"""Generate g19_render.npz by running the REFERENCE's camera (psaegert/bcnf src/bcnf/simulation/camera.py: camera,
record_trajectory) and get_cams_position (simulation/sampling.py) on CPU, fed the draws of bcnf_amd's renderer.

Test infrastructure only, run like make_golden_cnn.py (same dynaconf stub; nothing of the reference is copied, only
inputs / outputs). The reference checkout's src directory is the first argument, or $BCNF_REFERENCE_SRC:

    python tests/golden/make_golden_render.py path/to/reference/src

The reference draws its 5000 points per frame with numpy's global np.random.normal(loc, scale, (5000, 3)), which no
kernel can follow. While the reference runs, np.random.normal is replaced by
    loc + scale * bcnf_amd.render.standard_normals(seed, offset, frame, 5000),     frame = 0, 1, ... per call of a case
(the documented draw of bcnf_render_frames), so the stored images are the reference's own projection, histogram,
normalisation and flip of exactly the points the kernel draws. np.histogram2d is wrapped to record the in-range count.

  case  call                                                                                   lit pixels
  c0    camera(ball (3, 2, 4), cam (-25, 0, 1.5), r 0.1143, angle 0)                            a few
  c1    camera(ball (-24, 0.3, 1.6), 1 m from the camera, r 0.2, angle 10)                      thousands
  c2    camera(ball (0, 0, 30), above the view of the rotated second camera)                    0
  c3    camera(ball (5, 17.3, 1), 30 degrees off the axis of a 35 degree half-view, r 0.3)      a few dozen
  c4    camera(ball (-40, 0, 1.5), behind the camera)                                           0
  c5    record_trajectory(a 4-frame arc, cam (-25, 0, 1.5), r 0.1143, angle -5)
  c6    camera(ball (5, 21, 1.5), on the horizontal range edge (30 tan 35 deg = 21.006), r 0.3)  about half the cloud
                                                                                               dropped

Condition, enforced here: no sample of a stored frame lies within MARGIN = 1e-9 rad of a bin edge or range edge in
either angle (as bcnf_amd.render.render_host computes the angles) -- about 1e6 times the disagreement to expect between
two correctly rounded float64 implementations of log / sincos / atan2. A case that violates it moves to the next
`offset`, which is stored. Under this condition another implementation of the same draws must give the same integer
counts, hence bit-identical images. Also stored: each case's inputs, basis (the reference's three camera vectors) and
n_in, and get_cams_position for three parameter sets.
"""
import os
import sys
import tempfile
from unittest import mock

import numpy as np

REF_SRC = sys.argv[1] if len(sys.argv) > 1 else os.environ.get("BCNF_REFERENCE_SRC")
OUT = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(OUT))
SEED = 2024_03_25
MARGIN = 1e-9
N = 5000
CAM0 = [-25.0, 0.0, 1.5]
CAM1 = [-1.76843004, 24.93737467, 2.5]          # get_cams_position([0, 1.2], 25, [1.5, 2.5])[1]
ARC = [[-2.0, 1.0, 1.5], [-1.4, 1.3, 2.6], [-0.8, 1.6, 3.3], [-0.2, 1.9, 3.6]]
CASES = [("c0", "camera", [[3.0, 2.0, 4.0]], CAM0, 0.1143, 0.0),
         ("c1", "camera", [[-24.0, 0.3, 1.6]], CAM0, 0.2, 10.0),
         ("c2", "camera", [[0.0, 0.0, 30.0]], CAM1, 0.1143, 15.0),
         ("c3", "camera", [[5.0, 17.3, 1.0]], CAM0, 0.3, 0.0),
         ("c4", "camera", [[-40.0, 0.0, 1.5]], CAM0, 0.1143, 0.0),
         ("c5", "record_trajectory", ARC, CAM0, 0.1143, -5.0),
         ("c6", "camera", [[5.0, 21.0, 1.5]], CAM0, 0.3, 0.0)]
CAM_SETS = [([0.0, 1.2], 25.0, [1.5, 2.5]), ([0.0, 4.7], 9.3, [0.4, 1.4]), ([0.0, 0.0], 25.0, [1.0, 1.0])]


def _import_reference():
    if not REF_SRC or not os.path.isdir(REF_SRC):
        raise SystemExit("usage: make_golden_render.py path/to/reference/src (or set BCNF_REFERENCE_SRC)")
    stub = tempfile.mkdtemp(prefix="bcnf_stub_")
    os.makedirs(os.path.join(stub, "dynaconf"))
    with open(os.path.join(stub, "dynaconf", "__init__.py"), "w") as f:
        f.write("class Dynaconf:\n    def __init__(self, *a, **k):\n        raise RuntimeError('stub')\n")
    sys.dont_write_bytecode = True
    sys.path[:0] = [stub, REF_SRC, ROOT]
    import matplotlib
    matplotlib.use("Agg")
    import bcnf.simulation.camera as camera  # noqa
    import bcnf.simulation.sampling as sampling  # noqa
    return camera, sampling


def run_reference(cam_mod, kind, balls, cam_pos, radius, angle, offset):
    """(images (T, 90, 160), n_in (T,)) of the reference fed standard_normals(SEED, offset, frame, 5000)."""
    from bcnf_amd.render import standard_normals
    calls, totals = [0], []
    real_hist = np.histogram2d

    def normal(loc=0.0, scale=1.0, size=None):
        assert tuple(size) == (N, 3)
        z = standard_normals(SEED, offset, calls[0], N)
        calls[0] += 1
        return loc + scale * z

    def hist(*a, **k):
        vals = real_hist(*a, **k)
        totals.append(int(np.sum(vals[0])))
        return vals

    with mock.patch.object(np.random, "normal", normal), mock.patch.object(np, "histogram2d", hist):
        if kind == "camera":
            img = cam_mod.camera(ball_pos=np.array(balls[0]), cam_pos=np.array(cam_pos), radius=radius,
                                 viewing_angle=angle)[None]
        else:
            img = cam_mod.record_trajectory(np.array(balls), cam_pos=np.array(cam_pos), make_gif=False, radius=radius,
                                            viewing_angle=angle)
    assert calls[0] == len(balls) == len(totals) and img.dtype == np.float64 and img.shape == (len(balls), 90, 160)
    return img, np.array(totals, dtype=np.int32)


def reference_basis(cam_mod, cam_pos, angle):
    cam_pos = np.array(cam_pos)
    focus_point = np.array([0, 0, cam_pos[2]])
    cam_dir = (focus_point - cam_pos) / np.linalg.norm(focus_point - cam_pos)
    cam_dir = cam_mod.rotate_vector(cam_dir, angle)
    cam_orthogonal_z = cam_mod.rotate_vector(cam_dir, 90)
    return np.stack([cam_dir, np.cross(cam_dir, cam_orthogonal_z), cam_orthogonal_z])


def main():
    cam_mod, sampling = _import_reference()
    from bcnf_amd.render import render_host
    arrays = {"seed": np.int64(SEED), "margin": np.float64(MARGIN), "names": np.array([c[0] for c in CASES])}
    for name, kind, balls, cam_pos, radius, angle in CASES:
        offset = 0
        while True:
            host, counts, n_host, near = render_host(np.array([balls]), np.array([[cam_pos]]), np.array([[angle]]),
                                                     np.array([radius]), seed=SEED, offset=offset, return_counts=True,
                                                     edge_margin=MARGIN)
            if not near:
                break
            print(f"case {name}: offset {offset} has {len(near)} sample(s) within {MARGIN} rad of an edge; next offset")
            offset += 1
        img, n_in = run_reference(cam_mod, kind, balls, cam_pos, radius, angle, offset)
        if not (np.array_equal(img, host[0, 0]) and np.array_equal(n_in, n_host[0, 0])):
            raise SystemExit(f"case {name}: render_host and the reference disagree outside the margin")
        for t in range(len(balls)):
            s = img[t].sum()
            assert (n_in[t] == 0 and s == 0.0) or abs(s - 1.0) < 1e-12
        print(f"case {name}: offset {offset}, n_in {n_in.tolist()}, lit pixels {[int((f > 0).sum()) for f in img]}")
        arrays.update({f"{name}/ball": np.array(balls), f"{name}/cam_pos": np.array(cam_pos),
                       f"{name}/radius": np.float64(radius), f"{name}/angle": np.float64(angle),
                       f"{name}/offset": np.int64(offset), f"{name}/images": img, f"{name}/n_in": n_in,
                       f"{name}/basis": reference_basis(cam_mod, cam_pos, angle)})
    arrays["cams/radiants"] = np.array([c[0] for c in CAM_SETS])
    arrays["cams/radius"] = np.array([c[1] for c in CAM_SETS])
    arrays["cams/heights"] = np.array([c[2] for c in CAM_SETS])
    arrays["cams/pos"] = np.array([np.array(sampling.get_cams_position(np.array(r), c, np.array(h)))
                                   for r, c, h in CAM_SETS])
    path = os.path.join(OUT, "g19_render.npz")
    np.savez_compressed(path, **arrays)
    size = os.path.getsize(path)
    print(f"{path}: {size} bytes")
    if size > 1000_000:
        raise SystemExit("g19_render.npz is over 1 MB")


if __name__ == "__main__":
    main()
