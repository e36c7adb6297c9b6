"""Relative-pose refinement throughput: N image pairs of K correspondences
(10 % gross outliers) through the C entry point
mi_ba_refine_relative_pose_batch on arrays packed beforehand.

No earlier version of this call exists, so the yardstick is the nearest
existing path: the same number of problems and correspondences, pose only,
through mi_ba_refine_absolute_pose_batch (csrc/pose_refine.hip, which this
feature does not touch: tangent 6, two rows per correspondence).  The two
calls alternate in one session, warm-up first, best of five each.  Prints one
JSON line per call (and appends them to --out FILE): seconds of the C call,
microseconds per problem, the LM iterations (successful + unsuccessful
steps) summed over the batch, nanoseconds per correspondence-iteration, and
on the relative-pose line the ratio to the yardstick.

    python tools/bench_relative_pose.py [N=4096] [K=200] [--out FILE]"""
import ctypes as C
import json
import sys
import time

import numpy as np

sys.path[:0] = ["tests", "semantic-bundle-adjustment-colmap_amd", "oracle"]
import mi_ba  # noqa: E402
import pose_cases as pc  # noqa: E402
import relative_pose_cases as rc  # noqa: E402

args = [a for a in sys.argv[1:] if not a.startswith("--")]
OUT = sys.argv[sys.argv.index("--out") + 1] if "--out" in sys.argv else None
if OUT:
    args.remove(OUT)
N = int(args[0]) if len(args) > 0 else 4096
K = int(args[1]) if len(args) > 1 else 200
REPEATS = 5


class RelativeCall:
    def __init__(self, problems):
        self.o = mi_ba.default_relative_pose_options()
        self.a = mi_ba._RelativePoseArrays(problems)
        self.q0, self.t0 = self.a.q.copy(), self.a.t.copy()
        n = len(problems)
        self.st, self.us, self.sums = np.zeros(n, np.int32), np.zeros(n, np.int32), (mi_ba.Summary * n)()

    def __call__(self):
        self.a.q[:], self.a.t[:] = self.q0, self.t0
        t = time.perf_counter()
        rc_ = mi_ba.load().mi_ba_refine_relative_pose_batch(
            C.byref(self.o), C.byref(self.a.batch), self.st.ctypes.data_as(mi_ba._i32p),
            C.cast(self.sums, C.c_void_p), self.us.ctypes.data_as(mi_ba._i32p))
        dt = time.perf_counter() - t
        assert rc_ == 0 and np.all(self.us == 1)
        return dt


class AbsoluteCall:
    """mi_ba_refine_absolute_pose_batch, pose only, on packed arrays."""

    def __init__(self, problems):
        n = len(problems)
        self.o = mi_ba.default_pose_refine_options(refine_focal_length=0, refine_extra_params=0)
        self.a = mi_ba._PoseArrays(problems)
        self.c0, self.q0, self.t0 = self.a.cams.copy(), self.a.q.copy(), self.a.t.copy()
        self.st, self.us, self.sums = np.zeros(n, np.int32), np.zeros(n, np.int32), (mi_ba.Summary * n)()

    def __call__(self):
        self.a.cams[:], self.a.q[:], self.a.t[:] = self.c0, self.q0, self.t0
        t = time.perf_counter()
        rc_ = mi_ba.load().mi_ba_refine_absolute_pose_batch(
            C.byref(self.o), C.byref(self.a.batch), self.st.ctypes.data_as(mi_ba._i32p), C.cast(self.sums, C.c_void_p),
            self.us.ctypes.data_as(mi_ba._i32p))
        dt = time.perf_counter() - t
        assert rc_ == 0 and np.all(self.us == 1)
        return dt


def row(call, name, best):
    its = sum(s.num_successful_steps + s.num_unsuccessful_steps for s in call.sums)
    return {"call": name, "problems": N, "correspondences": K, "c_call_s": round(best, 5),
            "us_per_problem": round(1e6 * best / N, 2), "iterations": its,
            "iterations_per_problem": round(its / N, 2), "ns_per_correspondence_iteration": round(1e9 * best / (its * K), 3)}


relative = RelativeCall([rc.make_problem(K, 7000 + k) for k in range(N)])
absolute = AbsoluteCall([pc.make_problem(mi_ba.SIMPLE_RADIAL, K, 7000 + k) for k in range(N)])
relative(), absolute()  # warm-up (library load, code objects)
best_r = best_a = None
for _ in range(REPEATS):  # alternating
    dr, da = relative(), absolute()
    best_r = dr if best_r is None else min(best_r, dr)
    best_a = da if best_a is None else min(best_a, da)
rows = [row(absolute, "mi_ba_refine_absolute_pose_batch, pose only (yardstick)", best_a),
        row(relative, "mi_ba_refine_relative_pose_batch", best_r)]
rows[1]["c_call_over_yardstick"] = round(best_r / best_a, 3)
rows[1]["per_correspondence_iteration_over_yardstick"] = round(
    rows[1]["ns_per_correspondence_iteration"] / rows[0]["ns_per_correspondence_iteration"], 3)
for r in rows:
    print(json.dumps(r), flush=True)
if OUT:
    with open(OUT, "a") as f:
        for r in rows:
            f.write(json.dumps(r) + "\n")
