#!/usr/bin/env python3
"""Linearization time per camera model at the C4 shape (1k cameras, 1M points,
10M observations, geometric term only): OPENCV against OPENCV_FISHEYE, FOV,
SIMPLE_RADIAL_FISHEYE and RADIAL_FISHEYE, whose Jacobians add an atan / sqrt /
divide chain in FP64 to a kernel that sits on the HBM write roof at OPENCV.

One process, one resident context per model, bench.py's warm-up and step
counts.  The models are timed in alternation over --rounds rounds, so a drift
of the box shows as spread inside every row instead of as a difference
between rows.  Per model and round: the host wall time per ctx.linearize()
(ends in a device synchronise) and the reproj_jacobian kernel's average
(device events, mi_ba_kernel_time).  Needs an MI355X; uses only the package.

  python tools/bench_models.py [--models OPENCV,FOV] [--out out/bench_models.jsonl]
  --package DIR  import mi_ba from DIR (another build of the package, e.g. the
                 parent commit's, to state its OPENCV row beside this one's)
"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

EXTRA = {
    "OPENCV": (-0.1, 0.01, 1e-4, -1e-4),
    "OPENCV_FISHEYE": (-0.05, 0.01, -1e-3, 1e-3),
    "FOV": (0.9, 0, 0, 0),
    "SIMPLE_RADIAL_FISHEYE": (0.05, 0, 0, 0),
    "RADIAL_FISHEYE": (0.05, -0.01, 0, 0),
}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--models", default=",".join(EXTRA))
    ap.add_argument("--images", type=int, default=1000)
    ap.add_argument("--points", type=int, default=1_000_000)
    ap.add_argument("--track", type=int, default=10)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=30)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--package", default=os.path.join(ROOT, "semantic-bundle-adjustment-colmap_amd"))
    ap.add_argument("--label", default="this build")
    ap.add_argument("--out", default=os.path.join(ROOT, "out", "bench_models.jsonl"))
    args = ap.parse_args()
    sys.path.insert(0, args.package)
    import mi_ba
    mi_ba.load()
    if mi_ba.device_count() == 0:
        raise SystemExit("bench_models.py: no MI355X visible (nothing is measured without one)")

    names = [n for n in args.models.split(",") if n]
    ctxs = {}
    for n in names:
        cfg = mi_ba.synth_config(mi_ba.MODEL_NAMES[n], args.images, args.points, track_length=args.track,
                                 rotation_range=0.05, extra=EXTRA[n])
        sc = mi_ba.generate_scene(cfg).gauge()
        ctxs[n] = mi_ba.Context(mi_ba.default_options(), sc)
        for _ in range(args.warmup):
            ctxs[n].linearize()
        ctxs[n].synchronize()
    wall = {n: [] for n in names}
    kern = {n: [] for n in names}
    for _ in range(args.rounds):
        for n in names:
            ctx = ctxs[n]
            ctx.set_timing(True)
            ctx.reset_kernel_times()
            ctx.synchronize()
            t0 = time.perf_counter()
            for _ in range(args.steps):
                ctx.linearize()
            ctx.synchronize()
            wall[n].append((time.perf_counter() - t0) * 1e3 / args.steps)
            ms, cnt = ctx.kernel_time("reproj_jacobian")
            kern[n].append(ms / max(1, cnt))  # the total over the window's launches
            ctx.set_timing(False)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "a") as f:
        print(f"| model ({args.label}) | blocks | W | jacobian kernel ms: min / median / max | linearize ms: min / median / max |")
        print("|---|---|---|---|---|")
        for n in names:
            nb, W, _ = ctxs[n].dims()
            row = dict(label=args.label, model=n, blocks=nb, jacobian_width=W, steps=args.steps, warmup=args.warmup,
                       rounds=args.rounds, kernel_ms=kern[n], linearize_ms=wall[n],
                       kernel_ms_median=statistics.median(kern[n]), linearize_ms_median=statistics.median(wall[n]))
            f.write(json.dumps(row) + "\n")
            print(f"| {n} | {nb} | {W} | {min(kern[n]):.4f} / {statistics.median(kern[n]):.4f} / {max(kern[n]):.4f} | "
                  f"{min(wall[n]):.4f} / {statistics.median(wall[n]):.4f} / {max(wall[n]):.4f} |")
    for c in ctxs.values():
        c.close()


if __name__ == "__main__":
    main()
