"""mi_ba_rig_solve (RigBundleAdjuster on the GPU solver: csrc/rig.hip, the rig
branch of context_solve) against the independent CPU reference
(tests/rig_reference.py) and against mi_ba_solve.

Base scene (tests/rig_scenes.py): 3 cameras x 4 snapshots, 2 images of no
rig, 1 image outside the config seen by some tracks, 60 points,
SIMPLE_RADIAL with one OPENCV camera in the rig; some of the outside image's
tracks are variable points (AddVariablePoint), the rest of them constant.

Bounds: those tests/test_lm_semantics.py applies to the exact path against
the oracle — the same accept / reject sequence, costs within 1e-9 relative,
parameters within 1e-7 (unit-scale scene; intrinsics relative to their size).
"""
import numpy as np
import pytest

import mi_ba
import rig_scenes
from test_rig_setup import concatenate_poses

pytestmark = pytest.mark.gpu

ITERATIONS = 8


def base(seed=0, **kw):
    sc, rig = rig_scenes.base_scene(seed=seed, **kw)
    sc.point_config = (np.arange(sc.num_points) % 6 == 0).astype(np.uint8)
    return sc, rig


def gpu_rig_solve(opts, sc, rig):
    trace = {}
    opts.set_callback(lambda it: trace.__setitem__(it.iteration, (it.step_is_valid, it.step_is_successful, it.cost)))
    s = mi_ba.rig_solve(opts, sc, rig)
    return s, [trace[k] for k in sorted(trace) if k >= 1]


def substantive(trace, min_relative_decrease=1e-3):
    """Leading iterations whose accept / reject decision is above rounding.
    A step is accepted when relative decrease = cost change / model cost change
    exceeds 1e-3.  Both solvers evaluate the cost, a sum of ~700 squared
    residuals, to ~n eps = 8e-14 relative, so the relative decrease carries an
    error of ~2 * 8e-14 * cost / model cost change; a decision is compared when
    its margin |relative decrease - 1e-3| is more than 1e-12 * cost / model cost
    change (6x that error).  After the first decision without that margin the
    two trajectories may part by rounding alone, so from there only the costs
    are compared (tests/test_lm_semantics.py treats its end phase the same way)."""
    for k, (valid, _, cost, model_change, rel) in enumerate(trace):
        if valid and abs(rel - min_relative_decrease) * model_change <= 1e-12 * cost:
            return k
    return len(trace)


def close(a, b, tol, what):
    a, b = np.asarray(a, float), np.asarray(b, float)
    err = np.abs(a - b) / np.maximum(1.0, np.abs(b))
    print(f"  {what}: max scaled difference {err.max() if err.size else 0:.3g}")
    assert np.all(err <= tol), (what, float(err.max()))


VARIANTS = {
    "default": {},
    "constant_relative_poses": dict(refine=0),
    "soft_l1": dict(loss=mi_ba.LOSS_SOFT_L1),
    "constant_camera": dict(const_cam=1),
    "constant_points": dict(const_pts=True),
    "reference_camera_last": dict(ref_pos=2),
}


@pytest.mark.parametrize("name", list(VARIANTS))
def test_rig_lm_matches_reference(gpu, name):
    v = VARIANTS[name]
    sc, rig = base(seed=4, ref_pos=v.get("ref_pos", 0))
    rig.refine_relative_poses = v.get("refine", 1)
    if v.get("const_pts"):
        sc.point_config[np.arange(sc.num_points) % 5 == 1] = 2
    if "const_cam" in v:
        sc.camera_constant = np.zeros(sc.num_cameras, np.uint8)
        sc.camera_constant[v["const_cam"]] = 1
    opts = mi_ba.default_options(max_num_iterations=ITERATIONS, loss_function_type=v.get("loss", mi_ba.LOSS_TRIVIAL))
    prob = rig_scenes.reference_problem(opts, sc, rig)
    out = prob.solve(max_num_iterations=ITERATIONS)

    s, tr = gpu_rig_solve(opts, sc, rig)
    assert s.num_residuals_reduced == prob.num_residuals_reduced
    assert s.num_effective_parameters_reduced == prob.num_effective_parameters_reduced
    print(f"{name}: compared decisions {substantive(out['trace'])} of {len(out['trace'])}; "
          f"cost {s.initial_cost:.6g} -> {s.final_cost:.6g} (reference {out['final_cost']:.6g}), "
          f"{s.num_successful_steps} + {s.num_unsuccessful_steps} steps")
    assert abs(s.initial_cost - out["initial_cost"]) <= 1e-9 * out["initial_cost"]
    n = substantive(out["trace"])
    assert n >= 4 and len(tr) == len(out["trace"])
    assert [(a, b) for a, b, _ in tr[:n]] == [(a, b) for a, b, *_ in out["trace"][:n]]
    if n == len(tr):
        assert s.num_successful_steps == out["num_successful_steps"]
        assert s.num_unsuccessful_steps == out["num_unsuccessful_steps"]
    for (_, _, cg), (_, _, cr, *_) in zip(tr, out["trace"]):
        assert abs(cg - cr) <= 1e-9 * cr, (cg, cr)
    assert abs(s.final_cost - out["final_cost"]) <= 1e-9 * out["final_cost"]
    assert s.final_cost < 0.5 * s.initial_cost
    L = prob.layout
    close(np.hstack([rig.snapshot_qvec, rig.snapshot_tvec]), prob.poses[:L["nsnap"]], 1e-7, "rig poses")
    close(np.hstack([rig.rel_qvec, rig.rel_tvec]), prob.poses[L["nsnap"]:L["ident"]], 1e-7, "relative poses")
    free = [i for i in range(sc.num_images) if i >= 12]
    close(np.hstack([sc.qvec, sc.tvec])[free], prob.poses[L["ident"] + 1:][free], 1e-7, "free image poses")
    close(sc.xyz, prob.points, 1e-7, "points")
    off = sc.camera_param_offsets()
    for c in range(sc.num_cameras):
        close(sc.camera_params.reshape(-1)[off[c]:off[c + 1]], prob.cams[c, :off[c + 1] - off[c]], 1e-7, f"camera {c}")


def test_identity_rigs_take_the_steps_of_the_free_solve(gpu):
    """Every image a one-camera rig of its own (reference camera, identity
    relative pose): T is the identity, so the rig branch must take the steps
    of mi_ba_solve on the same problem."""
    sc = mi_ba.generate_scene(mi_ba.synth_config(mi_ba.SIMPLE_RADIAL, 7, 150, track_length=4, rotation_range=0.05,
                                                 extra=(0.01,), noise=0.5, seed=5))
    I = sc.num_images
    rigs = [dict(cameras=[i], ref_camera=i, rel_qvec=[[1.0, 0, 0, 0]], rel_tvec=[[0.0, 0, 0]], snapshots=[[i]])
            for i in range(I)]
    a, b = sc.copy(), sc.copy()
    rig = mi_ba.RigInput(rigs=rigs, snapshot_qvec=sc.qvec.copy(), snapshot_tvec=sc.tvec.copy())
    opts = mi_ba.default_options(max_num_iterations=ITERATIONS, linear_solver_type=mi_ba.SOLVER_DENSE_SCHUR)
    tr_free = {}
    opts.set_callback(lambda it: tr_free.__setitem__(
        it.iteration, (it.step_is_valid, it.step_is_successful, it.cost,
                       it.cost_change / it.relative_decrease if it.relative_decrease else 0.0, it.relative_decrease)))
    s_free = mi_ba.solve(opts, a)
    s_rig, tr = gpu_rig_solve(opts, b, rig)
    free = [tr_free[k] for k in sorted(tr_free) if k >= 1]
    assert s_rig.num_residuals_reduced == s_free.num_residuals_reduced
    assert s_rig.num_effective_parameters_reduced == s_free.num_effective_parameters_reduced
    n = substantive(free)
    assert n >= 3 and len(tr) == len(free)
    assert [(x, y) for x, y, _ in tr[:n]] == [(x, y) for x, y, *_ in free[:n]]
    if n == len(free):
        assert s_rig.num_successful_steps == s_free.num_successful_steps
    assert s_rig.num_successful_steps >= 2
    for (_, _, cg), (_, _, cf, *_) in zip(tr, free):
        assert abs(cg - cf) <= 1e-9 * cf
    assert abs(s_rig.final_cost - s_free.final_cost) <= 1e-9 * s_free.final_cost
    close(b.xyz, a.xyz, 1e-7, "points")
    close(np.hstack([b.qvec, b.tvec]), np.hstack([a.qvec, a.tvec]), 1e-7, "image poses")
    close(np.hstack([rig.snapshot_qvec, rig.snapshot_tvec]), np.hstack([a.qvec, a.tvec]), 1e-7, "rig poses")
    close(b.camera_params, a.camera_params, 1e-7, "cameras")


def test_filter_and_write_back(gpu):
    sc, rig = base(seed=6)
    opts = mi_ba.default_options(max_num_iterations=4)
    n0 = mi_ba.rig_setup_stats(opts, sc, rig).num_residuals_reduced
    k = int(np.flatnonzero(sc.obs_image == 4)[3])
    sc.obs_xy[k] += 3000.0  # beyond max_reproj_error = 1000 at the concatenated pose
    rel_q0, rel_t0 = np.array(rig.rigs[0]["rel_qvec"]).copy(), np.array(rig.rigs[0]["rel_tvec"]).copy()
    outside_q, outside_t = sc.qvec[-1].copy(), sc.tvec[-1].copy()
    s = mi_ba.rig_solve(opts, sc, rig)
    assert s.num_residuals_reduced == n0 - 2
    assert s.final_cost < s.initial_cost
    # the reference camera's relative pose: bitwise unchanged; the others moved
    assert np.array_equal(rig.rel_qvec[0], rel_q0[0]) and np.array_equal(rig.rel_tvec[0], rel_t0[0])
    assert not np.array_equal(rig.rel_tvec[1], rel_t0[1]) and not np.array_equal(rig.rel_qvec[2], rel_q0[2])
    # every rig image's pose is ConcatenatePoses(rig, rel) of the returned poses
    for sn, images in enumerate(rig.rigs[0]["snapshots"]):
        for i in images:
            c = int(sc.image_camera[i])
            q, t = concatenate_poses(rig.snapshot_qvec[sn], rig.snapshot_tvec[sn], rig.rel_qvec[c], rig.rel_tvec[c])
            assert np.abs(sc.qvec[i] - q).max() <= 4e-16 and np.abs(sc.tvec[i] - t).max() <= 4e-16 * max(1, np.abs(t).max())
    # the image outside the config keeps its pose
    assert np.array_equal(sc.qvec[-1], outside_q) and np.array_equal(sc.tvec[-1], outside_t)


def test_constant_relative_poses_stay_bitwise(gpu):
    sc, rig = base(seed=7)
    rig.refine_relative_poses = 0
    rel_q0, rel_t0 = np.array(rig.rigs[0]["rel_qvec"]).copy(), np.array(rig.rigs[0]["rel_tvec"]).copy()
    s = mi_ba.rig_solve(mi_ba.default_options(max_num_iterations=3), sc, rig)
    assert s.num_successful_steps >= 1
    assert np.array_equal(rig.rel_qvec, rel_q0) and np.array_equal(rig.rel_tvec, rel_t0)


def test_rig_solve_refuses_the_iterative_solver(gpu):
    sc, rig = base(seed=8)
    q0 = sc.qvec.copy()
    with pytest.raises(mi_ba.MiBaError) as e:
        mi_ba.rig_solve(mi_ba.default_options(linear_solver_type=mi_ba.SOLVER_ITERATIVE_SCHUR), sc, rig)
    assert e.value.status == mi_ba.ERR_UNSUPPORTED
    assert np.array_equal(sc.qvec, q0)


def test_rig_context_refuses_a_semantic_term(gpu):
    sc = mi_ba.generate_scene(mi_ba.synth_config(mi_ba.SIMPLE_PINHOLE, 3, 30, track_length=3, image_size=96,
                                                 rotation_range=0.05))
    depth, label = mi_ba.render_semantic(sc, 96, 96, cell=0.5)
    sem = mi_ba.SemanticInput(depth, label, np.array([(0, 1), (1, 2), (2, 0)], np.int32), pixel_step=8)
    rigs = [dict(cameras=[i], ref_camera=i, rel_qvec=[[1.0, 0, 0, 0]], rel_tvec=[[0.0, 0, 0]], snapshots=[[i]])
            for i in range(3)]
    rig = mi_ba.RigInput(rigs=rigs, snapshot_qvec=sc.qvec.copy(), snapshot_tvec=sc.tvec.copy())
    mi_ba.Context(mi_ba.default_options(), sc.copy(), sem).close()       # the semantic term alone is fine
    mi_ba.Context(mi_ba.default_options(), sc.copy(), rig=rig).close()   # and so are the rigs alone
    with pytest.raises(mi_ba.MiBaError) as e:
        mi_ba.Context(mi_ba.default_options(), sc.copy(), sem, rig=rig)
    assert e.value.status == mi_ba.ERR_UNSUPPORTED


def test_rig_context_refuses_a_host_reducer_and_solves_without(gpu):
    sc, rig = base(seed=8)
    sc2, rig2 = base(seed=8)
    opts = mi_ba.default_options(max_num_iterations=3)
    with mi_ba.Context(opts, sc, rig=rig) as ctx:
        with pytest.raises(mi_ba.MiBaError) as e:
            ctx.set_host_reducer(0, 1, lambda a: None)
        assert e.value.status == mi_ba.ERR_UNSUPPORTED
        s = ctx.solve()  # the refused call left the context usable
        ctx.writeback()
    s2 = mi_ba.rig_solve(opts, sc2, rig2)
    assert s.final_cost == s2.final_cost and s.num_successful_steps == s2.num_successful_steps
    assert np.array_equal(sc.xyz, sc2.xyz) and np.array_equal(rig.snapshot_tvec, rig2.snapshot_tvec)
    assert np.array_equal(rig.rel_qvec, rig2.rel_qvec) and np.array_equal(sc.qvec, sc2.qvec)


def test_rig_solve_is_repeatable(gpu):
    """No floating-point atomics on the rig path: two solves give the same bits."""
    out = []
    for _ in range(2):
        sc, rig = base(seed=9)
        s = mi_ba.rig_solve(mi_ba.default_options(max_num_iterations=4), sc, rig)
        out.append((s.final_cost, sc.xyz.copy(), rig.snapshot_tvec.copy(), rig.rel_qvec.copy()))
    assert out[0][0] == out[1][0]
    for a, b in zip(out[0][1:], out[1][1:]):
        assert np.array_equal(a, b)
