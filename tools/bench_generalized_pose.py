"""Generalized absolute-pose refinement throughput: N problems, each a rig of
C cameras with K correspondences per camera (10 % gross outliers), through
mi_ba_refine_generalized_absolute_pose_batch (one launch) in three
configurations:

  1. pose only (SIMPLE_RADIAL data),
  2. focal + extra parameters on SIMPLE_RADIAL,
  3. focal + extra parameters on OPENCV,

and, as the yardstick,

  4. the correspondences of configuration 2 as N single-camera problems of
     C * K correspondences through mi_ba_refine_absolute_pose_batch.

The rig's cameras share one centre (identity relative poses) and start from
the same intrinsics, so that the correspondences of a rig are also those of
one camera; every rig camera still owns its parameter block and its tiles, and
the kernel's arithmetic does not depend on the relative poses' values.
Correspondence i belongs to camera i % C (interleaved).  Prints one JSON line
per configuration, warm-up first, best of five: "s" times the whole Python
call (packing included, as tools/bench_pose_refine.py does), "c_call_s" the C
entry point alone on arrays packed beforehand; the ratios use the latter.

    python tools/bench_generalized_pose.py [N=1024] [C=5] [K=60] [--yardstick-only]"""
import json
import sys
import time

import numpy as np

sys.path[:0] = ["tests", "semantic-bundle-adjustment-colmap_amd", "oracle"]
import mi_ba  # noqa: E402
import pose_cases as pc  # noqa: E402

args = [a for a in sys.argv[1:] if not a.startswith("--")]
N = int(args[0]) if len(args) > 0 else 1024
C = int(args[1]) if len(args) > 1 else 5
K = int(args[2]) if len(args) > 2 else 60
YARDSTICK_ONLY = "--yardstick-only" in sys.argv


def best_of(call, problems, opts, repeats=5):
    call(opts, problems[:2])  # warm-up (library load, code objects)
    best, res = None, None
    for _ in range(repeats):
        t = time.perf_counter()
        res = call(opts, problems)
        dt = time.perf_counter() - t
        best = dt if best is None else min(best, dt)
    assert all(int(u) == 1 for u in res.usable)
    return best, res


def c_call_generalized(opts, problems, repeats=5):
    """Best time of the C entry point alone."""
    import ctypes as C_
    a = mi_ba._GeneralizedPoseArrays(problems)
    q0, t0, c0 = a.q.copy(), a.t.copy(), a.cams.copy()
    n = len(problems)
    st, us, sums = np.zeros(n, np.int32), np.zeros(n, np.int32), (mi_ba.Summary * n)()
    best = None
    for _ in range(repeats):
        a.q[:], a.t[:], a.cams[:] = q0, t0, c0
        t = time.perf_counter()
        rc = mi_ba.load().mi_ba_refine_generalized_absolute_pose_batch(
            C_.byref(opts), C_.byref(a.batch), st.ctypes.data_as(mi_ba._i32p), C_.cast(sums, C_.c_void_p),
            us.ctypes.data_as(mi_ba._i32p))
        dt = time.perf_counter() - t
        assert rc == 0
        best = dt if best is None else min(best, dt)
    return best


def c_call_single(opts, problems, repeats=5):
    """Best time of mi_ba_refine_absolute_pose_batch alone."""
    import ctypes as C_
    n = len(problems)
    cnt = [len(p.points2D) for p in problems]
    obs_off = np.concatenate([[0], np.cumsum(cnt)]).astype(np.int64)
    p2 = np.ascontiguousarray(np.concatenate([p.points2D for p in problems]))
    p3 = np.ascontiguousarray(np.concatenate([p.points3D for p in problems]))
    models = np.array([p.camera_model for p in problems], np.int32)
    cam_off = np.concatenate([[0], np.cumsum([len(p.camera_params) for p in problems])]).astype(np.int64)
    c0 = np.ascontiguousarray(np.concatenate([p.camera_params for p in problems]))
    q0 = np.ascontiguousarray(np.array([p.qvec for p in problems]))
    t0 = np.ascontiguousarray(np.array([p.tvec for p in problems]))
    cams, q, t = c0.copy(), q0.copy(), t0.copy()
    b = mi_ba.PoseBatch()
    b.num_problems = n
    b.obs_offsets = obs_off.ctypes.data_as(mi_ba._i64p)
    b.points2D = p2.ctypes.data_as(mi_ba._dp)
    b.points3D = p3.ctypes.data_as(mi_ba._dp)
    b.camera_model_ids = models.ctypes.data_as(mi_ba._i32p)
    b.camera_param_offsets = cam_off.ctypes.data_as(mi_ba._i64p)
    b.camera_params = cams.ctypes.data_as(mi_ba._dp)
    b.qvec = q.ctypes.data_as(mi_ba._dp)
    b.tvec = t.ctypes.data_as(mi_ba._dp)
    st, us, sums = np.zeros(n, np.int32), np.zeros(n, np.int32), (mi_ba.Summary * n)()
    best = None
    for _ in range(repeats):
        cams[:], q[:], t[:] = c0, q0, t0
        tt = time.perf_counter()
        rc = mi_ba.load().mi_ba_refine_absolute_pose_batch(C_.byref(opts), C_.byref(b), st.ctypes.data_as(mi_ba._i32p),
                                                           C_.cast(sums, C_.c_void_p), us.ctypes.data_as(mi_ba._i32p))
        dt = time.perf_counter() - tt
        assert rc == 0
        best = dt if best is None else min(best, dt)
    return best


def row(config, mode, best, res, **kw):
    its = sum(s.num_successful_steps + s.num_unsuccessful_steps for s in res.summaries)
    out = {"config": config, "mode": mode, "problems": N, "cameras": C, "correspondences_per_camera": K,
           "s": round(best, 5), "us_per_problem": round(1e6 * best / N, 2), "iterations": its,
           "final_cost_sum": sum(s.final_cost for s in res.summaries)}
    out.update(kw)
    print(json.dumps(out), flush=True)
    return out


def rig_of(p):
    """The single-camera problem as a rig of C coincident cameras."""
    n = len(p.points2D)
    rq = np.zeros((C, 4))
    rq[:, 0] = 1.0
    return mi_ba.GeneralizedPoseProblem([p.camera_model] * C, [p.camera_params.copy() for _ in range(C)], rq,
                                        np.zeros((C, 3)), p.qvec, p.tvec, p.points2D, p.points3D,
                                        (np.arange(n) % C).astype(np.int32))


single = {m: [pc.make_problem(m, C * K, 7000 + k) for k in range(N)] for m in (mi_ba.SIMPLE_RADIAL, mi_ba.OPENCV)}
o_full = mi_ba.default_pose_refine_options()
o_pose = mi_ba.default_pose_refine_options(refine_focal_length=0, refine_extra_params=0)

best4, res4 = best_of(mi_ba.refine_absolute_pose_batch, single[mi_ba.SIMPLE_RADIAL], o_full)
c4 = c_call_single(o_full, single[mi_ba.SIMPLE_RADIAL])
y = row(4, "refine_absolute_pose_batch, SIMPLE_RADIAL focal + extra, one camera", best4, res4, c_call_s=round(c4, 5),
        c_call_us_per_problem=round(1e6 * c4 / N, 2))
if YARDSTICK_ONLY:
    sys.exit(0)

for config, name, model, o in ((1, "pose only", mi_ba.SIMPLE_RADIAL, o_pose),
                               (2, "SIMPLE_RADIAL focal + extra", mi_ba.SIMPLE_RADIAL, o_full),
                               (3, "OPENCV focal + extra", mi_ba.OPENCV, o_full)):
    rigs = [rig_of(p) for p in single[model]]
    best, res = best_of(mi_ba.refine_generalized_absolute_pose_batch, rigs, o)
    cc = c_call_generalized(o, rigs)
    row(config, "refine_generalized_absolute_pose_batch, " + name, best, res,
        tangent=int(res.summaries[0].num_effective_parameters_reduced), c_call_s=round(cc, 5),
        c_call_us_per_problem=round(1e6 * cc / N, 2), c_call_over_config_4=round(cc / c4, 2))
