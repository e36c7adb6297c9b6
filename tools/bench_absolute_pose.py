"""Robust absolute pose throughput through the C entry point
mi_ba_estimate_absolute_pose_batch on arrays packed beforehand, allocations
and copies included, under the mapper's options (max_error 12 px, confidence
0.99999, 100 <= trials <= 10 000, min_inlier_ratio 0.25;
incremental_mapper.cc:436-447):

  images  IMAGES (default 1 024) problems of POINTS (default 1 000)
          correspondences, 30 % outliers at least 50 px away, 0.5 px noise;
  sweep   the 31 focal-length hypotheses (pose.cc:91-98, ratios 0.2 to 5) of
          32 images of the same size: 992 problems on 32 correspondence sets.

Nothing comparable existed on the device, so the yardstick is the host build
of the same block header (tests/cpp/absolute_pose_block_test, ap_loransac per
problem) under an OpenMP loop on THREADS threads, alternating with the device
in one session, best of REPEATS each.  Per workload one JSON line (appended to
--out FILE): seconds of the C call, problems/s and trials/s of both, their
ratio, the problems on which the two differ in a discrete output (with the
focal factor and both sides' trials, inliers and local flag of the first
few), and the share of the trials the 64-wide rounds evaluated that an abort discarded (from
num_trials, so within one trial per problem).

    python tools/bench_absolute_pose.py [IMAGES=1024] [POINTS=1000] [THREADS=16] [--out FILE]
"""
import ctypes as C
import json
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(ROOT, "tests"), os.path.join(ROOT, "semantic-bundle-adjustment-colmap_amd")]
import mi_ba as M  # noqa: E402
import absolute_pose_cases as ac  # noqa: E402
import absolute_pose_reference as aref  # noqa: E402

args = [a for a in sys.argv[1:] if not a.startswith("--")]
OUT = sys.argv[sys.argv.index("--out") + 1] if "--out" in sys.argv else None
if OUT:
    args.remove(OUT)
IMAGES = int(args[0]) if len(args) > 0 else 1024
POINTS = int(args[1]) if len(args) > 1 else 1000
THREADS = int(args[2]) if len(args) > 2 else 16
REPEATS = 3
SWEEP_IMAGES = 32


class Call:
    """The C entry point on packed arrays."""

    def __init__(self, sets, cameras, problems, o):
        self.o = o
        self.a = a = M._AbsolutePoseEstimationArrays(sets, cameras, problems, o)
        n, total = a.n, int(a.mask_off[-1])
        self.P, self.q, self.t = np.zeros((n, 12)), np.zeros((n, 4)), np.zeros((n, 3))
        self.mask = np.zeros(total, np.uint8)
        self.success, self.inl, self.local = np.zeros(n, np.int32), np.zeros(n, np.int32), np.zeros(n, np.int32)
        self.trials = np.zeros(n, np.int64)

    def __call__(self):
        t = time.perf_counter()
        st = M.load().mi_ba_estimate_absolute_pose_batch(
            C.byref(self.o), C.byref(self.a.batch), M._ptr(self.P, M._dp), M._ptr(self.q, M._dp),
            M._ptr(self.t, M._dp), M._ptr(self.mask, M._u8p), M._ptr(self.success, M._i32p),
            M._ptr(self.trials, M._i64p), M._ptr(self.inl, M._i32p), M._ptr(self.local, M._i32p))
        dt = time.perf_counter() - t
        assert st == 0, st
        return dt


def write_batch(path, a, o):
    """The binary form tests/cpp/absolute_pose_block_test.cc reads."""
    prm8 = np.zeros((len(a.models), 8))
    for c in range(len(a.models)):
        prm8[c, :a.prm_off[c + 1] - a.prm_off[c]] = a.prm[a.prm_off[c]:a.prm_off[c + 1]]
    with open(path, "wb") as f:
        np.array([a.n, len(a.set_off) - 1, int(a.set_off[-1]), len(a.models)], np.int64).tofile(f)
        np.array([o.max_error, o.min_inlier_ratio, o.confidence, o.dyn_num_trials_multiplier], np.float64).tofile(f)
        np.array([o.min_num_trials, o.max_num_trials], np.int64).tofile(f)
        for arr in (a.set_off, a.points2D, a.points3D, a.models, prm8, a.set_index, a.camera_index, a.factor, a.seed):
            np.ascontiguousarray(arr).tofile(f)


def host_once(path):
    """One timed pass of the host build on THREADS threads: (seconds, per-problem rows)."""
    exe = os.path.join(ROOT, "tests", "cpp", "absolute_pose_block_test")
    out = subprocess.run([exe, "estimate", path, path + ".out", str(THREADS), "1"], check=True, capture_output=True,
                         text=True).stdout
    seconds = float([l for l in out.splitlines() if l.startswith("SECONDS")][0].split()[1])
    return seconds, [l.split() for l in open(path + ".out")]


def discarded_share(trials, cap):
    """Of the trials the 64-wide rounds evaluated, the share past the last one the reference runs."""
    used = np.where(trials < cap, trials - 1, cap)  # an abort counts one trial more than it ran
    evaluated = np.minimum(cap, (used + 63) // 64 * 64)
    return float((evaluated - used).sum() / max(1, evaluated.sum()))


def measure(name, sets, cameras, problems, ref_o):
    o = ac.device_options(ref_o)
    call = Call(sets, cameras, problems, o)
    path = os.path.join(ROOT, "out", "absolute_pose_bench.bin")
    write_batch(path, call.a, ref_o)
    call()  # warm-up (library load, code objects)
    dev, host, rows = [], [], None
    for _ in range(REPEATS):  # alternating
        dev.append(call())
        s, rows = host_once(path)
        host.append(s)
    best, host_s = min(dev), min(host)
    off = call.a.mask_off
    differing = [k for k, w in enumerate(rows)
                 if (int(w[0]), int(w[1]), int(w[2]), int(w[3])) !=
                 (call.success[k], call.trials[k], call.inl[k], call.local[k])
                 or (w[0] == "1" and w[23] != "".join(map(str, call.mask[off[k]:off[k + 1]])))]
    differ = len(differing)
    # what differs, for the first few: focal factor, then (trials, inliers, local) of host and device
    detail = [{"problem": k, "focal_length_factor": round(float(call.a.factor[k]), 4),
               "host": [int(v) for v in rows[k][1:4]],
               "device": [int(call.trials[k]), int(call.inl[k]), int(call.local[k])]} for k in differing[:8]]
    cap = min(ref_o.max_num_trials, aref.compute_num_trials(int(ref_o.min_inlier_ratio * 100000), 100000,
                                                            ref_o.confidence, ref_o.dyn_num_trials_multiplier))
    trials = int(call.trials.sum())
    n = call.a.n
    row = {"call": "mi_ba_estimate_absolute_pose_batch", "workload": name, "problems": n,
           "correspondence_sets": len(sets), "correspondences_per_problem": POINTS,
           "resident_in_lds": bool(POINTS <= M.absolute_pose_lds_capacity()),
           "succeeded": int(call.success.sum()), "trials": trials, "trial_cap": int(cap),
           "c_call_s": round(best, 4), "problems_per_s": round(n / best), "trials_per_s": round(trials / best),
           "host_threads": THREADS, "host_s": round(host_s, 4), "host_problems_per_s": round(n / host_s),
           "host_trials_per_s": round(trials / host_s), "device_over_host": round(host_s / best, 3),
           "problems_differing_from_host": differ, "first_differing": detail,
           "discarded_share_of_evaluated_trials": round(discarded_share(call.trials, cap), 4),
           "c_call_s_all": [round(x, 4) for x in dev], "host_s_all": [round(x, 4) for x in host]}
    print(json.dumps(row), flush=True)
    return row


os.makedirs(os.path.join(ROOT, "out"), exist_ok=True)
subprocess.run(["make", "-C", os.path.join(ROOT, "tests", "cpp"), "-f", "absolute_pose.mk", "absolute_pose_block_test"],
               check=True, capture_output=True)
o = ac.mapper_options()
scenes = [ac.make_problem(POINTS, 5000 + k) for k in range(IMAGES)]
rows = [measure("images", [(p.points2D, p.points3D) for p in scenes], [(p.model, p.params) for p in scenes],
                [M.AbsolutePoseEstimationProblem(k, k, 1.0, k) for k in range(IMAGES)], o)]
factors = aref.focal_length_factors(30, 0.2, 5.0)
sweep = scenes[:SWEEP_IMAGES]
rows.append(measure("sweep", [(p.points2D, p.points3D) for p in sweep], [(p.model, p.params) for p in sweep],
                    [M.AbsolutePoseEstimationProblem(k, k, f, k) for k in range(len(sweep)) for f in factors], o))
if OUT:
    with open(OUT, "a") as f:
        for r in rows:
            f.write(json.dumps(r) + "\n")
