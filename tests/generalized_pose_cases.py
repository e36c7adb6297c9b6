"""Synthetic generalized absolute-pose problems (camera rigs) for
test_generalized_pose.py, and their CPU reference solutions
(generalized_pose_reference)."""
import functools

import numpy as np

import camera_model_ref as cm
import generalized_pose_reference as gref
import mi_ba
from estimator_testing import qmul, quat, same_stop, ulp_solves

TRUE_PARAMS = {
    mi_ba.SIMPLE_PINHOLE: [1200.0, 500.0, 500.0],
    mi_ba.PINHOLE: [1200.0, 1180.0, 500.0, 500.0],
    mi_ba.SIMPLE_RADIAL: [1200.0, 500.0, 500.0, 0.02],
    mi_ba.RADIAL: [1200.0, 500.0, 500.0, 0.02, -0.01],
    mi_ba.OPENCV: [1200.0, 1180.0, 500.0, 500.0, 0.05, -0.02, 1e-3, -1e-3],
    mi_ba.OPENCV_FISHEYE: [600.0, 590.0, 500.0, 500.0, 0.02, -0.01, 2e-3, -1e-3],
    mi_ba.FOV: [600.0, 590.0, 500.0, 500.0, 0.6],
    mi_ba.SIMPLE_RADIAL_FISHEYE: [600.0, 500.0, 500.0, 0.02],
    mi_ba.RADIAL_FISHEYE: [600.0, 500.0, 500.0, 0.02, -0.01],
}
START_OFFSET = {
    mi_ba.SIMPLE_PINHOLE: [20.0, 0.0, 0.0],
    mi_ba.PINHOLE: [20.0, -15.0, 0.0, 0.0],
    mi_ba.SIMPLE_RADIAL: [20.0, 0.0, 0.0, 0.01],
    mi_ba.RADIAL: [20.0, 0.0, 0.0, 0.01, 0.005],
    mi_ba.OPENCV: [20.0, -15.0, 0.0, 0.0, 0.01, 0.01, 5e-4, 5e-4],
    mi_ba.OPENCV_FISHEYE: [10.0, -8.0, 0.0, 0.0, 5e-3, 5e-3, 1e-3, 1e-3],
    mi_ba.FOV: [10.0, -8.0, 0.0, 0.0, 0.02],
    mi_ba.SIMPLE_RADIAL_FISHEYE: [10.0, 0.0, 0.0, 5e-3],
    mi_ba.RADIAL_FISHEYE: [10.0, 0.0, 0.0, 5e-3, 5e-3],
}
ALL_MODELS = sorted(TRUE_PARAMS)


def make_rig_problem(models, counts, seed, identity=False, outlier_fraction=0.1, outlier_px=40.0, noise_px=0.5,
                     masked_extra=0, interleave=True):
    """A rig of len(models) cameras; camera c sees counts[c] correspondences of
    a cloud 5 units in front of it (pixel noise, round(outlier_fraction n)
    gross outliers of outlier_px), relative rotations up to 90 degrees and
    baselines 0.1-0.5 (identity: no relative pose), a start off the true rig
    pose and intrinsics.  masked_extra correspondences per camera are added
    with a zero mask; camera_idxs is interleaved."""
    rng = np.random.default_rng(seed)
    q = quat(rng.normal(size=3) * 0.1)
    t = np.array([0.1, -0.2, 0.3]) + rng.normal(size=3) * 0.1
    R = mi_ba.quat_to_rot(q)
    rq, rt, p2, p3, ci, mk, prms = [], [], [], [], [], [], []
    for c, (model, n) in enumerate(zip(models, counts)):
        if identity:
            qr, tr = np.array([1.0, 0, 0, 0]), np.zeros(3)
        else:
            ax = rng.normal(size=3)
            qr = quat(ax / np.linalg.norm(ax) * rng.uniform(0.2, np.pi / 2))
            tr = rng.normal(size=3)
            tr *= rng.uniform(0.1, 0.5) / np.linalg.norm(tr)
        rq.append(qr)
        rt.append(tr)
        prm = np.array(TRUE_PARAMS[model])
        prms.append(prm + START_OFFSET[model])
        m = n + masked_extra
        if m == 0:
            continue
        Rr = mi_ba.quat_to_rot(qr)
        P = rng.uniform(-1.0, 1.0, size=(m, 3)) * [1.5, 1.5, 1.0] + [0.1, -0.2, 5.0]  # camera frame
        Y = (P - tr) @ Rr        # rig frame: Rr^T (P - tr)
        X = (Y - t) @ R          # world
        x, y = cm.world_to_image(model, prm, P[:, 0] / P[:, 2], P[:, 1] / P[:, 2])
        xy = np.stack([x, y], 1) + rng.normal(size=(m, 2)) * noise_px
        n_out = int(round(outlier_fraction * n))
        if n_out:
            who = rng.choice(n, n_out, replace=False)
            ang = rng.uniform(0, 2 * np.pi, n_out)
            xy[who] += outlier_px * np.stack([np.cos(ang), np.sin(ang)], axis=1)
        p2.append(xy)
        p3.append(X)
        ci.append(np.full(m, c, np.int32))
        mk.append(np.concatenate([np.ones(n, np.uint8), np.zeros(masked_extra, np.uint8)]))
    p2, p3, ci, mk = np.concatenate(p2), np.concatenate(p3), np.concatenate(ci), np.concatenate(mk)
    if interleave:
        order = rng.permutation(len(ci))
        p2, p3, ci, mk = p2[order], p3[order], ci[order], mk[order]
    q0 = qmul(quat(rng.normal(size=3) * 0.01), q)
    q0 /= np.linalg.norm(q0)
    t0 = t + rng.normal(size=3) * 0.03
    return mi_ba.GeneralizedPoseProblem(list(models), prms, np.array(rq), np.array(rt), q0, t0,
                                        np.ascontiguousarray(p2), np.ascontiguousarray(p3), ci,
                                        mk if masked_extra else None)


def reference_problem(pr, rf=True, re=True, loss_function_scale=1.0):
    return gref.Problem(pr.camera_models, pr.camera_params, pr.rig_qvecs, pr.rig_tvecs, pr.qvec, pr.tvec, pr.points2D,
                        pr.points3D, pr.camera_idxs, pr.inlier_mask, rf, re, loss_function_scale)


def reference_solve(pr, rf=True, re=True, **kw):
    return reference_problem(pr, rf, re).solve(**kw)


def is_stable(problem, result, rf, re, **kw):
    """pose_cases.is_stable applied to the reference: its step counts and stop
    survive ulp perturbations of the inputs and its final cost moves by less
    than 1e-7 relative under them."""
    for s in ulp_solves(problem, lambda p: reference_solve(p, rf, re, **kw), ("tvec", "points2D", "points3D")):
        if not same_stop(s, result) or abs(s.final_cost - result.final_cost) > 1e-7 * result.final_cost:
            return False
    return True


M = mi_ba
# rigs of 2, 3 and 5 cameras: (models, inlier counts per camera, masked extras per camera).  Over the rigs the
# models cover all nine, the counts 0 and every tile edge (1, 63, 64, 65, 130).
RIGS = [
    ((M.PINHOLE, M.SIMPLE_RADIAL_FISHEYE), (63, 65), 0),
    ((M.SIMPLE_PINHOLE, M.FOV), (1, 130), 2),
    ((M.SIMPLE_RADIAL, M.RADIAL, M.OPENCV_FISHEYE), (64, 0, 65), 3),
    ((M.OPENCV, M.SIMPLE_PINHOLE, M.RADIAL_FISHEYE, M.FOV, M.SIMPLE_RADIAL), (130, 1, 63, 0, 64), 0),
]
FLAGS = [(0, 0), (1, 0), (1, 1)]
# seeds chosen on the CPU so that the reference's own stops are stable under
# ulp perturbations in at least nine cases of ten (is_stable)
SEEDS = {}


def case_seed(ri, fi):
    return SEEDS.get((ri, fi), 7000 + 10 * ri + fi)


def streaming_counts():
    """Three cameras, one inlier above the LDS-resident limit in all."""
    cap = mi_ba.generalized_pose_limits()[2]
    return (cap - 160, 96, 65)


@functools.lru_cache(maxsize=None)
def parity_cases():
    """[(name, rf, re, problem, reference result, stable)]; computed once."""
    specs = []
    for ri, (models, counts, extra) in enumerate(RIGS):
        for fi, (rf, re) in enumerate(FLAGS):
            specs.append((f"rig{ri}-{rf}{re}", rf, re, make_rig_problem(models, counts, case_seed(ri, fi),
                                                                        masked_extra=extra)))
    specs.append(("streaming", 1, 1, make_rig_problem((M.SIMPLE_RADIAL, M.OPENCV, M.RADIAL), streaming_counts(),
                                                      case_seed(8, 0))))
    specs.append(("seven-opencv", 1, 1, make_rig_problem((M.OPENCV,) * 7, (40, 30, 64, 20, 65, 25, 33),
                                                         case_seed(9, 0))))
    # The principal point is never refined, so an OPENCV camera adds 6 columns: the seven-OPENCV rig has a
    # tangent of 48.  Ten cameras reach 62, eleven the kernel's 64.
    specs.append(("tangent-62", 1, 1, make_rig_problem((M.OPENCV,) * 9 + (M.SIMPLE_RADIAL,),
                                                       (30, 22, 64, 20, 35, 25, 33, 21, 28, 40), case_seed(10, 0))))
    specs.append(("tangent-64", 1, 1, make_rig_problem((M.OPENCV,) * 9 + (M.PINHOLE,) * 2,
                                                       (30, 22, 40, 20, 35, 25, 33, 21, 28, 19, 65), case_seed(11, 0))))
    out = []
    for name, rf, re, pr in specs:
        s = reference_solve(pr, rf, re)
        out.append((name, rf, re, pr, s, is_stable(pr, s, rf, re)))
    return out
