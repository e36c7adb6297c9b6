"""Robust triangulation throughput: N tracks (default 100 000) whose lengths
are drawn from a fixed histogram (median 4, tail to 200) through the C entry
point mi_ba_estimate_triangulation_batch on arrays packed beforehand, once
with the angular residual under IncrementalTriangulator::Create's options and
once with the reprojection residual under CompleteImage's
(incremental_triangulator.cc:138-145, 508-522; C(n, 2) trials at least for
n <= 15).

Nothing comparable existed on the device, so the yardstick is the host build
of the same block header (tests/cpp/triangulation_block_test, tri_loransac per
track) under an OpenMP loop on THREADS threads, in the same session, best of
REPEATS each.  Per residual type one JSON line (appended to --out FILE):
seconds of the C call (upload, record build, kernel and download included),
tracks/s and trials/s of both, their ratio, the tracks on which the two differ
in a discrete output, the mean trials per track that a 64-wide round evaluated
beyond the one that ended the run (the price of speculation; from num_trials,
so within one trial per track), the lanes idle in the only round of a track of
median length, and the Python packing time of the same batch from
TriangulationProblem objects.

    python tools/bench_triangulation.py [N=100000] [THREADS=16] [--out FILE]

Scene: 2 000 views on a ring of radius 4 to 6 around the origin, three cameras
(PINHOLE, OPENCV, OPENCV_FISHEYE, about 1200 px focal length); a track sees a
point near the origin from n views spread over an arc of 40 to 120 degrees;
noise 1 / 1200 (1.2 px), 20 % gross outliers of 40 / 1200 per coordinate."""
import ctypes as C
import json
import math
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(ROOT, "tests"), os.path.join(ROOT, "semantic-bundle-adjustment-colmap_amd")]
import mi_ba as M  # noqa: E402
import triangulation_cases as tc  # noqa: E402

args = [a for a in sys.argv[1:] if not a.startswith("--")]
OUT = sys.argv[sys.argv.index("--out") + 1] if "--out" in sys.argv else None
if OUT:
    args.remove(OUT)
N = int(args[0]) if len(args) > 0 else 100000
THREADS = int(args[1]) if len(args) > 1 else 16
REPEATS = 5
VIEWS = 2000
LENGTHS = np.array([2, 3, 4, 5, 6, 8, 10, 15, 20, 30, 50, 100, 200])
WEIGHTS = np.array([.22, .20, .15, .10, .08, .08, .06, .04, .03, .02, .012, .006, .002])


def scene(seed=1):
    rng = np.random.default_rng(seed)
    cams = [tc.CAMERAS[c] for c in tc.MIXED]
    proj = np.zeros((VIEWS, 3, 4))
    for v in range(VIEWS):
        phi = 2 * math.pi * v / VIEWS
        r = rng.uniform(4.0, 6.0)
        proj[v] = tc.look_at(np.array([r * math.cos(phi), r * math.sin(phi), rng.uniform(-0.5, 0.5)]), rng)
    centers = -np.einsum("vji,vj->vi", proj[:, :, :3], proj[:, :, 3])
    view_cam = (np.arange(VIEWS) % len(cams)).astype(np.int32)
    lengths = rng.choice(LENGTHS, size=N, p=WEIGHTS / WEIGHTS.sum())
    off = np.concatenate([[0], np.cumsum(lengths)]).astype(np.int64)
    total = int(off[-1])
    track = np.repeat(np.arange(N), lengths)
    k = np.arange(total) - off[track]
    arc = rng.uniform(40.0, 120.0, size=N) / 360.0 * VIEWS
    stride = np.maximum(1, (arc / np.maximum(lengths - 1, 1)).astype(np.int64))
    view = ((rng.integers(0, VIEWS, size=N)[track] + stride[track] * k) % VIEWS).astype(np.int32)
    X = rng.uniform(-0.3, 0.3, size=(N, 3))[track]
    pc = np.einsum("oij,oj->oi", proj[view][:, :, :3], X) + proj[view][:, :, 3]
    pn = pc[:, :2] / pc[:, 2:] + rng.normal(size=(total, 2)) * tc.NOISE
    bad = rng.random(total) < 0.2
    pn[bad] += rng.normal(size=(int(bad.sum()), 2)) * tc.OUTLIER
    px = np.zeros((total, 2))
    for c, (model, prm) in enumerate(cams):
        sel = view_cam[view] == c
        px[sel, 0], px[sel, 1] = tc.tref.cref.world_to_image(model, prm, pn[sel, 0], pn[sel, 1])
    min_trials = np.where(lengths <= 15, lengths * (lengths - 1) // 2, 0).astype(np.int64)
    return dict(cams=cams, proj=proj.reshape(VIEWS, 12), centers=centers, view_cam=view_cam, lengths=lengths, off=off,
                view=view, pn=np.ascontiguousarray(pn), px=np.ascontiguousarray(px), min_trials=min_trials)


class Call:
    """The C entry point on packed arrays."""

    def __init__(self, s, o):
        self.s, self.o = s, o
        self.models = np.array([c[0] for c in s["cams"]], np.int32)
        self.prm = np.concatenate([np.asarray(c[1], np.float64) for c in s["cams"]])
        self.prm_off = np.concatenate([[0], np.cumsum([len(c[1]) for c in s["cams"]])]).astype(np.int64)
        b = self.b = M.TriangulationBatch()
        b.num_problems = N
        b.obs_offsets = M._ptr(s["off"], M._i64p)
        b.view_index = M._ptr(s["view"], M._i32p)
        b.points = M._ptr(s["px"], M._dp)
        b.points_normalized = M._ptr(s["pn"], M._dp)
        b.num_views = VIEWS
        b.proj_matrices = M._ptr(s["proj"], M._dp)
        b.proj_centers = M._ptr(s["centers"], M._dp)
        b.camera_index = M._ptr(s["view_cam"], M._i32p)
        b.num_cameras = len(self.models)
        b.camera_model_ids = M._ptr(self.models, M._i32p)
        b.camera_param_offsets = M._ptr(self.prm_off, M._i64p)
        b.camera_params = M._ptr(self.prm, M._dp)
        b.min_num_trials = M._ptr(s["min_trials"], M._i64p)
        total = int(s["off"][-1])
        self.xyz, self.mask = np.zeros((N, 3)), np.zeros(total, np.uint8)
        self.success, self.inl, self.local = np.zeros(N, np.int32), np.zeros(N, np.int32), np.zeros(N, np.int32)
        self.trials = np.zeros(N, np.int64)

    def __call__(self):
        t = time.perf_counter()
        st = M.load().mi_ba_estimate_triangulation_batch(
            C.byref(self.o), C.byref(self.b), M._ptr(self.xyz, M._dp), M._ptr(self.mask, M._u8p),
            M._ptr(self.success, M._i32p), M._ptr(self.trials, M._i64p), M._ptr(self.inl, M._i32p),
            M._ptr(self.local, M._i32p))
        dt = time.perf_counter() - t
        assert st == 0, st
        return dt


def host(s, o, path):
    """The host build of the block header on the same batch: (best seconds, per-track outputs)."""
    exe = os.path.join(ROOT, "tests", "cpp", "triangulation_block_test")
    subprocess.run(["make", "-C", os.path.dirname(exe), "triangulation_block_test"], check=True, capture_output=True)
    prm8 = np.zeros((len(s["cams"]), 8))
    for c, (_, prm) in enumerate(s["cams"]):
        prm8[c, :len(prm)] = prm
    with open(path, "wb") as f:
        np.array([N, int(s["off"][-1]), VIEWS, len(s["cams"]), 1, 1], np.int64).tofile(f)
        np.array([o.min_tri_angle, o.residual_type, o.max_error, o.min_inlier_ratio, o.confidence,
                  o.dyn_num_trials_multiplier, 0, float(o.max_num_trials)], np.float64).tofile(f)
        for a in (s["off"], s["min_trials"], s["view"], s["px"], s["pn"], s["proj"], s["centers"], s["view_cam"],
                  np.array([c[0] for c in s["cams"]], np.int32), prm8):
            np.ascontiguousarray(a).tofile(f)
    out = subprocess.run([exe, "estimate", path, path + ".out", str(THREADS), str(REPEATS)], check=True,
                         capture_output=True, text=True).stdout
    seconds = float([l for l in out.splitlines() if l.startswith("SECONDS")][0].split()[1])
    rows = [l.split() for l in open(path + ".out")]
    return seconds, rows


def discarded(trials, lengths, min_trials, max_trials):
    """Trials a 64-wide round evaluated past the last one the reference runs."""
    cap = np.minimum(max_trials, lengths * (lengths - 1) // 2)
    used = np.where(trials < cap, trials - 1, cap)  # an abort counts one trial more than it ran
    return np.minimum(cap, (used + 63) // 64 * 64) - used


s = scene()
os.makedirs(os.path.join(ROOT, "out"), exist_ok=True)
t0 = time.perf_counter()
views = M.TriangulationViews(s["proj"], s["centers"], s["view_cam"], np.array([c[0] for c in s["cams"]], np.int32),
                             [c[1] for c in s["cams"]])
problems = [M.TriangulationProblem(s["view"][a:b], s["px"][a:b], s["pn"][a:b], int(m))
            for a, b, m in zip(s["off"][:-1], s["off"][1:], s["min_trials"])]
M._TriangulationArrays(views, problems)
packing = time.perf_counter() - t0
median = int(np.median(s["lengths"]))
rows = []
for name, ref_o in (("angular, Create's options", tc.create_options()),
                    ("reprojection, CompleteImage's options", tc.complete_options())):
    o = tc.device_options(ref_o)
    call = Call(s, o)
    call()  # warm-up (library load, code objects)
    best = min(call() for _ in range(REPEATS))
    host_s, host_rows = host(s, o, os.path.join(ROOT, "out", "triangulation_bench.bin"))
    differ = sum(1 for k, w in enumerate(host_rows)
                 if (int(w[0]), int(w[1]), int(w[2]), int(w[3])) !=
                 (call.success[k], call.trials[k], call.inl[k], call.local[k])
                 or (w[0] == "1" and w[7] != "".join(map(str, call.mask[s["off"][k]:s["off"][k + 1]]))))
    cap = tc.tref.compute_num_trials(int(o.min_inlier_ratio * 100000), 100000, o.confidence,
                                     o.dyn_num_trials_multiplier)
    disc = discarded(call.trials, s["lengths"], s["min_trials"], min(o.max_num_trials, cap))
    trials = int(call.trials.sum())
    rows.append({
        "call": "mi_ba_estimate_triangulation_batch", "residual": name, "tracks": N,
        "observations": int(s["off"][-1]), "median_length": median, "succeeded": int(call.success.sum()),
        "trials": trials, "c_call_s": round(best, 4), "tracks_per_s": round(N / best),
        "trials_per_s": round(trials / best), "host_threads": THREADS, "host_s": round(host_s, 4),
        "host_tracks_per_s": round(N / host_s), "host_trials_per_s": round(trials / host_s),
        "device_over_host": round(host_s / best, 3), "tracks_differing_from_host": differ,
        "mean_discarded_trials_per_track": round(float(disc.mean()), 2),
        "idle_lanes_at_median_length": 64 - median * (median - 1) // 2,
        "python_packing_s": round(packing, 3)})
    print(json.dumps(rows[-1]), flush=True)
if OUT:
    with open(OUT, "a") as f:
        for r in rows:
            f.write(json.dumps(r) + "\n")
