#!/usr/bin/env python3
"""Rig bundle adjustment against the same scene solved as free images.

5 cameras x 200 snapshots (1000 images) by default, points with 10
observations each.  Per run: mi_ba_rig_solve and mi_ba_solve
(DENSE_SCHUR, every image a free pose) on resident contexts.  Per run and
solver: the per-iteration wall time (the iteration callback's
iteration_time_in_seconds of the iterations after the first two, all listed,
with their median) from a solve with the kernel timers off, and the
per-iteration times of rig_project (and its two halves), the Cholesky, the Schur build and the other
phases from a second solve with the timers on.  rig_project's rate is given
against the nf^2 / 2 * 8 bytes of the per-image system's stored triangle.
One JSON line per run, appended to --out.

    python tools/bench_rig.py --runs 3 --out profiles/rig_bench.jsonl
"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "semantic-bundle-adjustment-colmap_amd"))
import mi_ba  # noqa: E402


def quat_mul(a, b):
    return np.stack([a[..., 0] * b[..., 0] - a[..., 1] * b[..., 1] - a[..., 2] * b[..., 2] - a[..., 3] * b[..., 3],
                     a[..., 0] * b[..., 1] + a[..., 1] * b[..., 0] + a[..., 2] * b[..., 3] - a[..., 3] * b[..., 2],
                     a[..., 0] * b[..., 2] - a[..., 1] * b[..., 3] + a[..., 2] * b[..., 0] + a[..., 3] * b[..., 1],
                     a[..., 0] * b[..., 3] + a[..., 1] * b[..., 2] - a[..., 2] * b[..., 1] + a[..., 3] * b[..., 0]], -1)


def rotate(q, p):
    qc = q * np.array([1.0, -1, -1, -1])
    return quat_mul(quat_mul(q, np.concatenate([np.zeros(p.shape[:-1] + (1,)), p], -1)), qc)[..., 1:]


def small_quats(rng, n, scale):
    q = np.concatenate([np.ones((n, 1)), rng.uniform(-scale, scale, (n, 3))], 1)
    return q / np.linalg.norm(q, axis=1, keepdims=True)


def rig_scene(cameras, snapshots, points, track, seed=0, noise=0.5):
    rng = np.random.default_rng(seed)
    rel_q = small_quats(rng, cameras, 0.05)
    rel_t = np.concatenate([0.3 * np.arange(cameras)[:, None], np.zeros((cameras, 2))], 1)
    rel_q[0], rel_t[0] = [1, 0, 0, 0], 0
    snap_q = small_quats(rng, snapshots, 0.05)
    snap_t = rng.uniform(-0.5, 0.5, (snapshots, 3))
    si, ci = np.repeat(np.arange(snapshots), cameras), np.tile(np.arange(cameras), snapshots)
    q = quat_mul(rel_q[ci], snap_q[si])
    t = rotate(rel_q[ci], snap_t[si]) + rel_t[ci]
    I = len(q)
    X = rng.uniform(-1, 1, (points, 3)) + np.array([0, 0, 6.0])
    oi = np.argsort(rng.random((points, I)), axis=1)[:, :track].reshape(-1).astype(np.int32)
    op = np.repeat(np.arange(points), track).astype(np.int32)
    P = rotate(q[oi], X[op]) + t[oi]
    u, v = P[:, 0] / P[:, 2], P[:, 1] / P[:, 2]
    f, k = 600.0, 0.01
    r2 = u * u + v * v
    xy = np.stack([f * u * (1 + k * r2) + 500, f * v * (1 + k * r2) + 500], 1) + noise * rng.standard_normal((len(u), 2))
    cams = np.tile([f, 500.0, 500.0, k], (cameras, 1))
    # perturbed start
    X = X + rng.uniform(-0.02, 0.02, X.shape)
    snap_t = snap_t + rng.uniform(-0.02, 0.02, snap_t.shape)
    sc = mi_ba.Scene(mi_ba.SIMPLE_RADIAL, cams, q, t, ci.astype(np.int32), X, xy, oi, op)
    snaps = [list(range(s * cameras, (s + 1) * cameras)) for s in range(snapshots)]
    rig = mi_ba.RigInput(rigs=[dict(cameras=list(range(cameras)), ref_camera=0, rel_qvec=rel_q, rel_tvec=rel_t,
                                    snapshots=snaps)], snapshot_qvec=snap_q, snapshot_tvec=snap_t)
    # the free solve starts from the concatenation of the perturbed rig poses
    sc.qvec = quat_mul(rel_q[ci], snap_q[si])
    sc.tvec = rotate(rel_q[ci], snap_t[si]) + rel_t[ci]
    return sc, rig


KERNELS = ("rig_project", "rig_project_blocks", "rig_project_tail", "rig_udiag", "cholesky", "cholesky_solve", "schur_build", "fblock", "backsub", "trial_cost")


def solve_ctx(sc, rig, iterations, timing):
    """One solve on a resident context -> (summary, steady iteration times in ms,
    {kernel: ms per LM iteration}).  Kernel times come from a run with the per-kernel
    event timers on, iteration times from a run with them off."""
    times = {}
    opts = mi_ba.default_options(max_num_iterations=iterations, linear_solver_type=mi_ba.SOLVER_DENSE_SCHUR)
    opts.set_callback(lambda it: times.__setitem__(it.iteration, it.iteration_time_in_seconds))
    with mi_ba.Context(opts, sc, rig=rig) as ctx:
        ctx.set_timing(timing)
        s = ctx.solve()
        kern = {}
        if timing:
            for k in KERNELS:
                ms, n = ctx.kernel_time(k)
                if n:
                    kern[k] = ms / max(1, s.num_successful_steps + s.num_unsuccessful_steps)  # per LM iteration
    return s, [1e3 * times[k] for k in sorted(times) if k >= 3], kern


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cameras", type=int, default=5)
    ap.add_argument("--snapshots", type=int, default=200)
    ap.add_argument("--points", type=int, default=20000)
    ap.add_argument("--track", type=int, default=10)
    ap.add_argument("--iterations", type=int, default=8)
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    mi_ba.load()
    for run in range(a.runs):
        line = dict(run=run, cameras=a.cameras, snapshots=a.snapshots, points=a.points, iterations=a.iterations)
        for name in ("rig", "free"):
            res = {}
            for timing in (False, True):
                sc, rig = rig_scene(a.cameras, a.snapshots, a.points, a.track)
                s, its, kern = solve_ctx(sc, rig if name == "rig" else None, a.iterations, timing)
                if timing:
                    res["kernels_ms_per_iteration"] = kern
                else:
                    res.update(ms_per_iteration=float(np.median(its)) if its else None, steady_iterations=its,
                               parameters=s.num_effective_parameters_reduced, initial_cost=s.initial_cost,
                               final_cost=s.final_cost, steps=[s.num_successful_steps, s.num_unsuccessful_steps])
            line["images"], line["observations"] = sc.num_images, sc.num_obs
            if name == "rig":
                # the projection reads the stored triangle of the per-image system once per owner pair
                nf = 6 * sc.num_images + 2 * a.cameras
                nslots = a.snapshots + a.cameras - 1
                res["nf_img"], res["nf_rig"] = nf, 6 * nslots + 2 * a.cameras
                t = res["kernels_ms_per_iteration"].get("rig_project")
                if t:
                    res["rig_project_required_bytes"] = nf * nf / 2 * 8
                    res["rig_project_required_GBs"] = nf * nf / 2 * 8 / (t * 1e-3) / 1e9
            line[name] = res
        print(json.dumps(line), flush=True)
        if a.out:
            with open(a.out, "a") as f:
                f.write(json.dumps(line) + "\n")


if __name__ == "__main__":
    main()
