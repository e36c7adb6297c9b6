"""Scenes and named cases of the robust absolute pose tests
(tests/test_absolute_pose.py): one image's 2D-3D correspondences under a
camera, with the numpy reference's answer computed once per case.

Scenes follow the issue's statement of what "equal to the reference" covers:
focal length about 1000, inlier noise at most 0.5 px (uniform), outliers at
least 50 px away, max_error 12 px."""
import functools
import math
from dataclasses import dataclass, field

import numpy as np

import absolute_pose_reference as aref
import camera_model_ref as cref
import mi_ba as M
from estimator_testing import quat, ulp_solves

FOCAL = 1000.0
# every supported model once; the two-focal ones with fx != fy so that the
# mean-focal threshold shows
CAMERAS = {
    "simple_pinhole": (M.SIMPLE_PINHOLE, [FOCAL, 640.0, 480.0]),
    "pinhole": (M.PINHOLE, [FOCAL, FOCAL * 1.08, 640.0, 480.0]),
    "simple_radial": (M.SIMPLE_RADIAL, [FOCAL, 640.0, 480.0, 0.05]),
    "radial": (M.RADIAL, [FOCAL, 640.0, 480.0, 0.05, -0.02]),
    "opencv": (M.OPENCV, [FOCAL, FOCAL * 0.93, 640.0, 480.0, 0.04, -0.01, 0.001, -0.002]),
    "opencv_fisheye": (M.OPENCV_FISHEYE, [FOCAL, FOCAL * 1.05, 640.0, 480.0, 0.02, -0.005, 0.001, 0.0]),
    "fov": (M.FOV, [FOCAL, FOCAL * 0.96, 640.0, 480.0, 0.6]),
    "simple_radial_fisheye": (M.SIMPLE_RADIAL_FISHEYE, [FOCAL, 640.0, 480.0, 0.03]),
    "radial_fisheye": (M.RADIAL_FISHEYE, [FOCAL, 640.0, 480.0, 0.03, -0.004]),
}


@dataclass
class Problem:
    """One image: pixels, 3D points, its camera, the hypothesis and the truth."""
    points2D: np.ndarray
    points3D: np.ndarray
    model: int
    params: np.ndarray
    factor: float = 1.0
    R: np.ndarray = None
    t: np.ndarray = None
    inlier: np.ndarray = None

    def copy(self):
        return Problem(self.points2D.copy(), self.points3D.copy(), self.model, self.params.copy(), self.factor,
                       self.R, self.t, self.inlier)


def make_problem(n, seed, camera="simple_pinhole", outliers=0.3, noise=0.5, kind="normal", true_factor=1.0):
    """n correspondences.  kind: "normal"; "coincident" (the first points of
    the set are one and the same correspondence); "collinear" (all 3D points on
    a line); "behind" (every third point behind the camera under the true
    pose).  true_factor: the pixels are made with the focal parameters times
    this, so that the given camera is off by it."""
    rng = np.random.default_rng(seed)
    model, prm = CAMERAS[camera]
    prm = np.array(prm, np.float64)
    R = M.quat_to_rot(quat(rng.normal(size=3) * 0.3))
    t = np.array([rng.uniform(-0.5, 0.5), rng.uniform(-0.5, 0.5), rng.uniform(0.0, 1.0)])
    uv = rng.uniform(-0.4, 0.4, size=(n, 2))
    depth = rng.uniform(4.0, 10.0, size=n)
    if kind == "collinear":
        s = np.linspace(-0.4, 0.4, n)
        uv = np.stack([s, 0.5 * s + 0.05], axis=1)
        depth = 6.0 + 3.0 * s
    pc = np.concatenate([uv * depth[:, None], depth[:, None]], axis=1)
    if kind == "collinear":  # a straight line in space
        pc = pc[0] + np.outer(np.linspace(0, 1, n), pc[-1] - pc[0])
        uv = pc[:, :2] / pc[:, 2:]
    X = (pc - t) @ R
    true_prm = aref.scaled_params(model, prm, true_factor)
    x, y = cref.world_to_image(model, true_prm, uv[:, 0], uv[:, 1])
    px = np.stack([x, y], axis=1) + rng.uniform(-noise, noise, size=(n, 2))
    inlier = np.ones(n, bool)
    bad = rng.random(n) < outliers
    if n >= 8:
        bad[:3] = False
    ang = rng.uniform(0, 2 * math.pi, size=n)
    off = rng.uniform(50.0, 300.0, size=n)
    px[bad] += np.stack([off * np.cos(ang), off * np.sin(ang)], axis=1)[bad]
    inlier[bad] = False
    if kind == "behind":
        sel = np.arange(n) % 3 == 2
        X[sel] = (pc[sel] * np.array([1.0, 1.0, -1.0]) - t) @ R
        inlier[sel] = False
    if kind == "coincident":
        k = min(4, n)
        px[:k] = px[0]
        X[:k] = X[0]
    return Problem(np.ascontiguousarray(px), np.ascontiguousarray(X), model, prm, 1.0, R, t, inlier)


def options(**kw):
    """The mapper's max_error on RANSACOptions' defaults."""
    return aref.Options(**{**dict(max_error=12.0), **kw})


def mapper_options(**kw):
    """IncrementalMapper's abs_pose options (incremental_mapper.cc:436-447)."""
    return options(**{**dict(confidence=0.99999, min_num_trials=100, max_num_trials=10000, min_inlier_ratio=0.25), **kw})


def device_options(o, **kw):
    return M.default_absolute_pose_estimation_options(
        max_error=o.max_error, min_inlier_ratio=o.min_inlier_ratio, confidence=o.confidence,
        dyn_num_trials_multiplier=o.dyn_num_trials_multiplier, min_num_trials=o.min_num_trials,
        max_num_trials=o.max_num_trials, seed=o.seed, **kw)


def option_key(o):
    """What a batch shares; the seed goes per problem."""
    return (o.max_error, o.min_inlier_ratio, o.confidence, o.dyn_num_trials_multiplier, o.min_num_trials,
            o.max_num_trials)


def reference(problem, o):
    return aref.estimate_kernel(o, problem.model, problem.params, problem.factor, problem.points2D, problem.points3D)


CASES = {}


def _case(n, seed, opt=None, **kw):
    def build():
        return make_problem(n, seed, **kw), (opt or options)(seed=seed)
    return build


# With four correspondences M'M has an exact null space of dimension four, whose
# basis rounding decides, and EPnP's answer is the same for every basis only
# where its Gauss-Newton steps reach the same optimum from each.  Seed 1104 is
# such a scene (tests/test_absolute_pose.py checks that the reference's
# decisions on it survive one-ulp perturbations); on 104 they do not.
_LENGTH_SEEDS = {4: 1104}
for _n in (2, 3, 4, 5, 63, 64, 65):
    CASES[f"n{_n}"] = _case(_n, _LENGTH_SEEDS.get(_n, 100 + _n), outliers=0.0 if _n < 8 else 0.3)
for _i, _cam in enumerate(CAMERAS):
    CASES[f"model_{_cam}"] = _case(40, 200 + _i, camera=_cam)
# (on seed 364 the 64 trials end at a four-inlier model, the case above)
for _t, _seed in ((1, 301), (64, 1364), (65, 365)):
    CASES[f"max_trials{_t}"] = _case(30, _seed, opt=functools.partial(options, max_num_trials=_t), outliers=0.5)
for _t in (63, 64, 65):
    CASES[f"min_trials{_t}"] = _case(30, 400 + _t, opt=functools.partial(options, min_num_trials=_t), outliers=0.0)
CASES["coincident"] = _case(24, 501, kind="coincident")
CASES["collinear"] = _case(24, 502, kind="collinear", outliers=0.0)
CASES["behind"] = _case(30, 503, kind="behind", outliers=0.0)
CASES["mapper_outliers"] = _case(120, 504, opt=mapper_options)
CASES["mapper_pinhole"] = _case(90, 505, opt=mapper_options, camera="pinhole")
MODEL_CASES = [k for k in CASES if k.startswith("model_")]
LENGTH_CASES = [f"n{n}" for n in (2, 3, 4, 5, 63, 64, 65)]
DEGENERATE_CASES = ["coincident", "collinear", "behind"]


def capacity_cases(capacity):
    """n one below, at and one above the kernel's LDS capacity (names; built lazily)."""
    out = []
    for n in (capacity - 1, capacity, capacity + 1):
        key = f"n{n}_capacity"
        CASES.setdefault(key, _case(n, 600 + n % 7))
        out.append(key)
    return out


@functools.lru_cache(maxsize=None)
def built(key):
    return CASES[key]()


@functools.lru_cache(maxsize=None)
def solved(key):
    """(problem, options, reference result) of a named case; computed once."""
    p, o = built(key)
    return p, o, reference(p, o)


@functools.lru_cache(maxsize=None)
def rounding_decided(key):
    """True when the reference itself changes a discrete output under inputs
    moved by one ulp (estimator_testing.ulp_solves): the case's decisions are
    then decided by rounding and a comparison may excuse it."""
    p, o, ref = solved(key)
    want = aref.discrete(ref)
    for got in ulp_solves(p, lambda q: aref.discrete(reference(q, o)), ("points2D", "points3D")):
        if got != want:
            return True
    return False
