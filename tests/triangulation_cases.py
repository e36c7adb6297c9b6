"""Synthetic tracks for test_triangulation.py and their CPU reference results
(triangulation_reference).

Scenes.  A point near the origin seen by n cameras on an arc of radius 4 to 6
around it (an arc of 40 to 120 degrees, so nearly every pair of views is above
the 1.5 degree minimum angle), each looking at the origin with a jitter of a
few degrees.  Angular tracks carry noise of 1 / 1200 on point_normalized and
round(0.2 n) gross outliers displaced by 40 / 1200 per coordinate (normal);
they run under IncrementalTriangulator::Create's options (min angle 1.5
degrees, max angular error 2 degrees, confidence 0.9999, min inlier ratio 0.02,
at most 10000 trials, C(n, 2) trials at least for n <= 15).  Reprojection
tracks carry 1 px of noise and outliers of 40 px under cameras of about 1200 px
focal length and run under CompleteImage's options (max error 4 px).

Failing tracks: all rays nearly parallel (a baseline of 1e-3 at distance 5:
every pair is far below 1.5 degrees), a point behind one of two cameras, and
two views whose rays disagree by far more than max_error.

Decision stability.  A case is compared only if the restatement's discrete
outputs (success, num_trials, best_is_local, num_inliers, mask) are unchanged
under four runs with every projection-matrix entry and image coordinate
perturbed by a relative 1e-9.  On the seeds below: 0 of the 120 general scenes
(lengths 2 to 65) are unstable, all succeed and 98 end before C(n, 2) trials;
none of the 29 named cases of test_triangulation.py is unstable.

Bound on xyz: the larger of 1e-9 max(1, |xyz|) and ten times the restatement's
own spread under inputs perturbed by one ulp (three runs).  Measured spread:
at most 3.5e-15 absolute on the named cases below (len9_derived) and 8.8e-15
over the 120 general scenes.  Ten times that stays below 1e-9, so the base
bound is the one that applies on these seeds; the rule stays in the code for
other seeds."""
import functools
import math

import numpy as np

import mi_ba
import triangulation_reference as tref

NOISE = 1.0 / 1200
OUTLIER = 40.0 / 1200
FOCAL = 1200.0
M = mi_ba

CAMERAS = {
    "pinhole": (M.PINHOLE, [FOCAL, FOCAL * 1.01, 600.0, 500.0]),
    "opencv": (M.OPENCV, [FOCAL, FOCAL * 0.99, 610.0, 490.0, -0.1, 0.01, 1e-4, -1e-4]),
    "fisheye": (M.OPENCV_FISHEYE, [FOCAL, FOCAL * 0.99, 590.0, 505.0, -0.05, 0.01, -1e-3, 1e-3]),
}


def create_options(n=None, **kw):
    """IncrementalTriangulator::Create (incremental_triangulator.cc:508-522)."""
    o = tref.Options(max_error=math.radians(2.0), min_tri_angle=math.radians(1.5), residual_type=tref.ANGULAR,
                     confidence=0.9999, min_inlier_ratio=0.02, max_num_trials=10000)
    if n is not None and n <= 15:
        o.min_num_trials = n * (n - 1) // 2
    for k, v in kw.items():
        setattr(o, k, v)
    return o


def complete_options(n=None, **kw):
    """IncrementalTriangulator::CompleteImage (incremental_triangulator.cc:138-145, 198-203)."""
    return create_options(n, residual_type=tref.REPROJECTION, max_error=4.0, **kw)


def look_at(center, rng, jitter=0.03):
    """[R | t] of a camera at `center` looking at the origin, rotated by a small random angle."""
    z = -center / np.linalg.norm(center)
    x = np.cross([0.0, 0.0, 1.0], z)
    x /= np.linalg.norm(x)
    R = np.stack([x, np.cross(z, x), z])
    w = rng.normal(size=3) * jitter
    a = np.linalg.norm(w)
    K = np.array([[0, -w[2], w[1]], [w[2], 0, -w[0]], [-w[1], w[0], 0]])
    R = (np.eye(3) + np.sin(a) / a * K + (1 - np.cos(a)) / a ** 2 * K @ K) @ R
    return np.concatenate([R, (-R @ center)[:, None]], axis=1)


def make_track(n, seed, outliers=0.2, cameras=("pinhole",), kind="normal"):
    """One track of n observations.  kind: "normal", "parallel", "behind" or
    "disagree" (the failing tracks above)."""
    rng = np.random.default_rng(seed)
    cams = [CAMERAS[c] for c in cameras]
    X = rng.uniform(-0.3, 0.3, size=3)
    arc = math.radians(rng.uniform(40.0, 120.0))
    phi0 = rng.uniform(0, 2 * math.pi)
    proj, centers = [], []
    for k in range(n):
        phi = phi0 + arc * (k / max(n - 1, 1)) + rng.normal() * 0.01
        r = rng.uniform(4.0, 6.0)
        c = np.array([r * math.cos(phi), r * math.sin(phi), rng.uniform(-0.5, 0.5)])
        if kind == "parallel":
            c = np.array([5.0 + 1e-3 * k, 1e-3 * rng.normal(), 0.0])
        P = look_at(c, rng)
        if kind == "behind" and k == 1:
            # turned away from the point: the two rays still meet at it, behind this camera
            R = np.diag([-1.0, 1.0, -1.0]) @ P[:, :3]
            P = np.concatenate([R, (-R @ c)[:, None]], axis=1)
        proj.append(P)
        centers.append(-P[:, :3].T @ P[:, 3])
    proj, centers = np.array(proj), np.array(centers)
    cam = np.arange(n) % len(cams)
    pc = proj[:, :, :3] @ X + proj[:, :, 3]
    pn = pc[:, :2] / pc[:, 2:] + rng.normal(size=(n, 2)) * NOISE
    bad = rng.permutation(n)[:int(round(outliers * n))] if kind == "normal" else []
    pn[bad] += rng.normal(size=(len(bad), 2)) * OUTLIER
    if kind == "disagree":
        pn[1] += [0.0, 0.3]
    px = np.zeros((n, 2))
    for c, (model, prm) in enumerate(cams):
        px[cam == c, 0], px[cam == c, 1] = tref.cref.world_to_image(model, prm, pn[cam == c, 0], pn[cam == c, 1])
    return tref.Track(proj, centers, pn, px, cam, cams)


def derive_normalized(track):
    """The track with point_normalized = Camera::ImageToWorld(point), as the triangulator's callers set it."""
    pn = np.array([M.image_to_world(track.cameras[c][0], track.cameras[c][1], x, y)
                   for c, (x, y) in zip(track.camera, track.points)])
    return tref.Track(track.proj, track.centers, pn, track.points, track.camera, track.cameras)


def perturbed(track, rel, seed):
    """Every projection-matrix entry and image coordinate times 1 +- rel; rel
    None: one ulp up or down."""
    rng = np.random.default_rng(seed)

    def p(a):
        s = rng.integers(0, 2, size=a.shape) * 2 - 1
        return np.nextafter(a, a + s) if rel is None else a * (1.0 + rel * s)
    return tref.Track(p(track.proj), track.centers, p(track.normalized), p(track.points), track.camera, track.cameras)


@functools.lru_cache(maxsize=None)
def solved(key):
    """(track, options, reference result, stable, xyz bound) of a named case; computed once."""
    track, o = CASES[key]()
    ref = tref.estimate_triangulation(o, track)
    want = tref.discrete(ref)
    stable = all(tref.discrete(tref.estimate_triangulation(o, perturbed(track, 1e-9, 100 + s))) == want
                 for s in range(4))
    bound = None
    if ref["success"]:
        spread = 0.0
        for s in range(3):
            r = tref.estimate_triangulation(o, perturbed(track, None, 200 + s))
            if r["success"]:
                spread = max(spread, float(np.abs(r["xyz"] - ref["xyz"]).max()))
        bound = max(1e-9 * max(1.0, float(np.linalg.norm(ref["xyz"]))), 10.0 * spread)
    return track, o, ref, stable, bound


def _case(n, seed, opt=create_options, derived=False, **kw):
    def build():
        t = make_track(n, seed, **kw)
        if derived:
            t = derive_normalized(t)
        return t, opt(n)
    return build


MIXED = ("pinhole", "opencv", "fisheye")
CASES = {}
# track lengths: 2, 3, 4, the exhaustive-sampling edge 15 / 16, one speculation round and one trial more
for _n in (2, 3, 4, 15, 16, 64, 65):
    CASES[f"len{_n}"] = _case(_n, 1000 + _n)
    CASES[f"len{_n}_reproj"] = _case(_n, 2000 + _n, complete_options, cameras=MIXED)
# max_num_trials binds (the dynamic bound would end these runs after a few trials, so min_num_trials
# holds them up to the cap): 40 trials of the 66, then one speculation round exactly and one trial more
CASES["len12_cap40"] = _case(12, 3012, lambda n: create_options(n, max_num_trials=40, min_num_trials=40))
CASES["len12_trials64"] = _case(12, 3013, lambda n: create_options(n, max_num_trials=64, min_num_trials=64))
CASES["len12_trials65"] = _case(12, 3014, lambda n: create_options(n, max_num_trials=65, min_num_trials=65))
CASES["len20_min150"] = _case(20, 3020, lambda n: create_options(n, min_num_trials=150))
CASES["len9_derived"] = _case(9, 3009, derived=True, cameras=MIXED)
CASES["len9_derived_reproj"] = _case(9, 3109, complete_options, derived=True, cameras=MIXED)
CASES["len30_outliers"] = _case(30, 3030)
CASES["len40_outliers_reproj"] = _case(40, 3040, complete_options, cameras=MIXED)
CASES["parallel"] = _case(5, 4001, kind="parallel", outliers=0.0)
CASES["behind"] = _case(2, 4002, kind="behind", outliers=0.0)
CASES["disagree"] = _case(2, 4003, kind="disagree", outliers=0.0)
FAILING = ("parallel", "behind", "disagree")


def capacity_cases(capacity):
    """n at the kernel's LDS capacity and one more (names only; built lazily)."""
    for n in (capacity, capacity + 1):
        for name, opt, cams in ((f"len{n}", create_options, ("pinhole",)),
                                (f"len{n}_reproj", complete_options, MIXED)):
            if name not in CASES:
                CASES[name] = _case(n, 5000 + n, opt, cameras=cams)
            yield name


def general_scenes():
    """The 120 scenes of the stability statement: lengths 2 to 65."""
    rng = np.random.default_rng(7)
    return [(int(n), 6000 + k) for k, n in enumerate(rng.integers(2, 66, size=120))]


def pack(tracks):
    """(TriangulationViews, [TriangulationProblem]) of a list of (track, options):
    every track brings its own views; the cameras are shared by name."""
    names, proj, centers, view_cam, problems = [], [], [], [], []
    cams = []
    for track, o in tracks:
        local = []
        for c in track.cameras:
            key = (c[0], tuple(c[1]))
            if key not in names:
                names.append(key)
                cams.append(c)
            local.append(names.index(key))
        base = len(view_cam)
        proj.extend(track.proj)
        centers.extend(track.centers)
        view_cam.extend(local[c] for c in track.camera)
        problems.append(M.TriangulationProblem(np.arange(base, base + len(track), dtype=np.int32), track.points,
                                               track.normalized, o.min_num_trials))
    views = M.TriangulationViews(np.array(proj), np.array(centers), np.array(view_cam, np.int32),
                                 np.array([c[0] for c in cams], np.int32), [c[1] for c in cams])
    return views, problems


def device_options(o, **kw):
    return M.default_triangulation_options(
        min_tri_angle=o.min_tri_angle, residual_type=o.residual_type, max_error=o.max_error,
        min_inlier_ratio=o.min_inlier_ratio, confidence=o.confidence,
        dyn_num_trials_multiplier=o.dyn_num_trials_multiplier, min_num_trials=o.min_num_trials,
        max_num_trials=o.max_num_trials, **kw)
