"""Synthetic absolute-pose problems and their CPU references for
test_pose_refine.py: the unchanged oracle on the equivalent scene (one image,
one camera, every correspondence a constant point, Cauchy loss, Ceres'
default tolerances)."""
import functools

import numpy as np

import mi_ba
import oracle
from estimator_testing import qmul, quat, same_stop, ulp_solves

TRUE_PARAMS = {
    mi_ba.SIMPLE_RADIAL: [1200.0, 500.0, 500.0, 0.02],
    mi_ba.OPENCV: [1200.0, 1180.0, 500.0, 500.0, 0.05, -0.02, 1e-3, -1e-3],
    mi_ba.OPENCV_FISHEYE: [600.0, 590.0, 500.0, 500.0, 0.02, -0.01, 2e-3, -1e-3],
}
START_OFFSET = {
    mi_ba.SIMPLE_RADIAL: [20.0, 0.0, 0.0, 0.01],
    mi_ba.OPENCV: [20.0, -15.0, 0.0, 0.0, 0.01, 0.01, 5e-4, 5e-4],
    mi_ba.OPENCV_FISHEYE: [10.0, -8.0, 0.0, 0.0, 5e-3, 5e-3, 1e-3, 1e-3],
}


def make_problem(model, n, seed, outlier_fraction=0.1, outlier_px=40.0, noise_px=0.5):
    """n correspondences of a camera 5 units in front of a unit cloud, pixel
    noise, round(outlier_fraction n) gross outliers moved by outlier_px, and a
    start off the true pose and intrinsics."""
    rng = np.random.default_rng(seed)
    prm = np.array(TRUE_PARAMS[model])
    q = quat(rng.normal(size=3) * 0.1)
    t = np.array([0.1, -0.2, 5.0]) + rng.normal(size=3) * 0.1
    X = rng.uniform(-1.0, 1.0, size=(n, 3)) * [1.5, 1.5, 1.0]
    R = mi_ba.quat_to_rot(q)
    P = X @ R.T + t
    xy = np.array([mi_ba.world_to_image(model, prm, p[0] / p[2], p[1] / p[2]) for p in P]).reshape(n, 2)
    xy += rng.normal(size=(n, 2)) * noise_px
    n_out = int(round(outlier_fraction * n))
    if n_out:
        who = rng.choice(n, n_out, replace=False)
        ang = rng.uniform(0, 2 * np.pi, n_out)
        xy[who] += outlier_px * np.stack([np.cos(ang), np.sin(ang)], axis=1)
    q0 = qmul(quat(rng.normal(size=3) * 0.01), q)
    q0 /= np.linalg.norm(q0)
    t0 = t + rng.normal(size=3) * 0.03
    return mi_ba.PoseProblem(model, prm + START_OFFSET[model], q0, t0, xy, X)


def oracle_options(refine_focal_length=True, refine_extra_params=True, gradient_tolerance=1.0,
                   max_num_iterations=100, loss_function_scale=1.0):
    """mi_ba_options of the equivalent scene (Ceres' defaults where
    RefineAbsolutePose leaves them alone)."""
    return mi_ba.default_options(loss_function_type=mi_ba.LOSS_CAUCHY, loss_function_scale=loss_function_scale,
                                 refine_focal_length=int(refine_focal_length), refine_principal_point=0,
                                 refine_extra_params=int(refine_extra_params), gradient_tolerance=gradient_tolerance,
                                 function_tolerance=1e-6, parameter_tolerance=1e-8,
                                 max_num_consecutive_invalid_steps=5, max_num_iterations=max_num_iterations)


def oracle_solve(problem, **kw):
    """(summary, trace rows that ran, refined scene) of the oracle."""
    sc = mi_ba.pose_problem_scene(problem)
    s, trace = oracle.solve_traced(oracle_options(**kw), sc)
    return s, trace[trace[:, 0] >= 0], sc


def is_stable(problem, summary, **kw):
    """The oracle's step counts survive ulp perturbations of the inputs: its
    stop is not decided by rounding (tests/test_lm_semantics.py); and its own
    final cost moves by less than 1e-7 relative under them, a tenth of the
    parity bound (an exactly fitted problem ends at a cost near zero whose
    relative value is rounding)."""
    for s, _, _ in ulp_solves(problem, lambda p: oracle_solve(p, **kw), ("tvec", "points2D", "points3D")):
        if not same_stop(s, summary) or abs(s.final_cost - summary.final_cost) > 1e-7 * summary.final_cost:
            return False
    return True


def streaming_count():
    """One count just above the LDS-resident limit: the streaming path."""
    return mi_ba.pose_refine_lds_capacity() + 1


# (model, refine focal, refine extra).  The oracle has the five older camera
# models only: the OPENCV_FISHEYE problems ride in the same batch and are
# checked against the existing GPU solver on the equivalent scene instead
# (fisheye_cases).
CONFIGS = [
    (mi_ba.SIMPLE_RADIAL, False, False),
    (mi_ba.SIMPLE_RADIAL, True, False),
    (mi_ba.SIMPLE_RADIAL, True, True),
    (mi_ba.OPENCV, True, True),
]


def counts():
    return [1, 2, 3, 4, 63, 64, 65, 257, streaming_count()]


def case_seed(ci, n):
    # seeds chosen on the CPU so that the oracle's own stops are stable under
    # ulp perturbations in at least nine cases of ten (is_stable)
    return SEEDS.get((ci, n), 100 * ci + n)


# 4 correspondences with the intrinsics refined: long trajectories with
# rejected steps (34 accepted / 8 rejected, 7 / 3), the reject path's exercise
SEEDS = {(1, 4): 388, (2, 4): 233}


@functools.lru_cache(maxsize=None)
def parity_cases():
    """[(config index, count, problem, oracle summary, trace, refined scene,
    stable)] of the trajectory-parity batch; computed once."""
    out = []
    for ci, (model, rf, re) in enumerate(CONFIGS):
        for n in counts():
            pr = make_problem(model, n, case_seed(ci, n))
            kw = dict(refine_focal_length=rf, refine_extra_params=re)
            s, tr, sc = oracle_solve(pr, **kw)
            out.append((ci, n, pr, s, tr, sc, is_stable(pr, s, **kw)))
    return out


@functools.lru_cache(maxsize=None)
def fisheye_cases():
    """[(count, problem)] OPENCV_FISHEYE, focal + extra refined."""
    return [(n, make_problem(mi_ba.OPENCV_FISHEYE, n, 400 + n)) for n in counts()]
