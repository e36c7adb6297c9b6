"""Batched absolute-pose refinement (mi_ba_refine_absolute_pose_batch,
RefineAbsolutePose of the reference): CPU tests of options, index sets and
argument checks, GPU tests against the oracle on the equivalent scene (one
image, one camera, every correspondence a constant point, Cauchy loss).

The refine flags are options of a call, so the trajectory-parity problems go
out in one call per flag combination; the focal + extra call mixes
SIMPLE_RADIAL, OPENCV and OPENCV_FISHEYE.  The oracle has no OPENCV_FISHEYE:
those problems are checked against the existing GPU solver (mi_ba.solve) on
the equivalent scene."""
import ctypes as C

import numpy as np
import pytest

import mi_ba
import oracle
import pose_cases as pc
from estimator_testing import gpu_sequence, oracle_sequence, run_program


def rel(a, b):
    return float(np.max(np.abs(np.asarray(a) - np.asarray(b)) / np.maximum(np.abs(np.asarray(b)), 1e-300)))


# --------------------------------------------------------------------------- CPU
def test_default_options_match_reference():
    # AbsolutePoseRefinementOptions (estimators/pose.h:93-124)
    o = mi_ba.default_pose_refine_options()
    assert o.gradient_tolerance == 1.0 and o.max_num_iterations == 100 and o.loss_function_scale == 1.0
    assert (o.refine_focal_length, o.refine_extra_params, o.device) == (1, 1, 0)


def one_problem_batch(pr, **kw):
    return mi_ba.refine_absolute_pose_batch(mi_ba.default_pose_refine_options(**kw), [pr])


@pytest.mark.parametrize("kw", [dict(gradient_tolerance=-1.0), dict(max_num_iterations=-1),
                                dict(loss_function_scale=-1.0)])
def test_options_check(kw):
    """AbsolutePoseRefinementOptions::Check: refused before any device is touched."""
    with pytest.raises(mi_ba.MiBaError) as e:
        one_problem_batch(pc.make_problem(mi_ba.SIMPLE_RADIAL, 5, 1), **kw)
    assert e.value.status == mi_ba.ERR_INVALID_ARGUMENT


@pytest.mark.parametrize("model", [mi_ba.SIMPLE_PINHOLE, mi_ba.PINHOLE, mi_ba.SIMPLE_RADIAL, mi_ba.RADIAL, mi_ba.OPENCV])
@pytest.mark.parametrize("rf,re", [(0, 0), (1, 0), (0, 1), (1, 1)])
def test_refined_index_sets_match_oracle(model, rf, re):
    """The refined-intrinsics sets (camera_models.h *Idxs, principal point
    fixed) against the oracle's reduced program of the equivalent scene."""
    idx = mi_ba.pose_refine_intrinsics(model, rf, re)
    pr = pc.make_problem(mi_ba.SIMPLE_RADIAL, 6, 1)
    pr.camera_model = model
    pr.camera_params = np.array([1200.0, 1190.0, 500.0, 500.0, 0.01, 0.01, 1e-3, 1e-3][:mi_ba.NUM_PARAMS[model]])
    if model == mi_ba.SIMPLE_PINHOLE or model == mi_ba.SIMPLE_RADIAL or model == mi_ba.RADIAL:
        pr.camera_params = np.array([1200.0, 500.0, 500.0, 0.01, 0.01][:mi_ba.NUM_PARAMS[model]])
    info = oracle.setup_stats(pc.oracle_options(refine_focal_length=rf, refine_extra_params=re),
                              mi_ba.pose_problem_scene(pr))
    assert info.num_effective_parameters_reduced == 6 + len(idx)
    assert list(idx) == sorted(idx)
    pp = {mi_ba.SIMPLE_PINHOLE: (1, 2), mi_ba.PINHOLE: (2, 3), mi_ba.SIMPLE_RADIAL: (1, 2), mi_ba.RADIAL: (1, 2),
          mi_ba.OPENCV: (2, 3)}[model]
    assert not set(idx) & set(pp)


def test_refined_index_sets_wide_angle_and_unsupported():
    assert list(mi_ba.pose_refine_intrinsics(mi_ba.OPENCV_FISHEYE)) == [0, 1, 4, 5, 6, 7]
    assert list(mi_ba.pose_refine_intrinsics(mi_ba.FOV)) == [0, 1, 4]
    assert list(mi_ba.pose_refine_intrinsics(mi_ba.SIMPLE_RADIAL_FISHEYE, True, False)) == [0]
    assert list(mi_ba.pose_refine_intrinsics(mi_ba.RADIAL_FISHEYE, False, True)) == [3, 4]
    assert mi_ba.pose_refine_intrinsics(6) is None and mi_ba.pose_refine_intrinsics(10) is None


def test_mismatched_sizes_are_refused():
    pr = pc.make_problem(mi_ba.SIMPLE_RADIAL, 5, 1)
    pr.points3D = pr.points3D[:4]
    with pytest.raises(ValueError):
        one_problem_batch(pr)
    pr = pc.make_problem(mi_ba.SIMPLE_RADIAL, 5, 1)
    pr.inlier_mask = np.ones(4, np.uint8)
    with pytest.raises(ValueError):
        one_problem_batch(pr)
    # a camera with the wrong number of parameters for its model: the C ABI's check
    pr = pc.make_problem(mi_ba.SIMPLE_RADIAL, 5, 1)
    pr.camera_params = pr.camera_params[:3]
    with pytest.raises(mi_ba.MiBaError) as e:
        one_problem_batch(pr)
    assert e.value.status == mi_ba.ERR_INVALID_ARGUMENT
    # negative problem count
    b = mi_ba.PoseBatch()
    b.num_problems = -1
    o = mi_ba.default_pose_refine_options()
    assert mi_ba.load().mi_ba_refine_absolute_pose_batch(C.byref(o), C.byref(b), None, None, None) == \
        mi_ba.ERR_INVALID_ARGUMENT


def test_new_symbols_are_declared():
    text = open(mi_ba.os.path.join(mi_ba._HERE, "..", "include", "mi_ba.h")).read()
    for name in ("mi_ba_refine_absolute_pose_batch", "mi_ba_default_pose_refine_options", "mi_ba_pose_batch",
                 "mi_ba_pose_refine_options"):
        assert name in text
    lib = mi_ba.load()
    assert lib.mi_ba_abi_version() == 4
    assert 64 <= mi_ba.pose_refine_lds_capacity() <= 4096


# --------------------------------------------------------------------------- GPU
def run(problems, covariance=False, trace_cap=0, **kw):
    tr = np.zeros((len(problems), trace_cap), np.uint8) if trace_cap else None
    res = mi_ba.refine_absolute_pose_batch(mi_ba.default_pose_refine_options(**kw), problems, covariance, trace=tr)
    return (res, tr) if trace_cap else res


def same_bits(res_a, i, res_b, j):
    return (np.array_equal(res_a.qvec[i], res_b.qvec[j]) and np.array_equal(res_a.tvec[i], res_b.tvec[j])
            and np.array_equal(res_a.camera_params[i], res_b.camera_params[j])
            and res_a.summaries[i].final_cost == res_b.summaries[j].final_cost
            and res_a.summaries[i].initial_cost == res_b.summaries[j].initial_cost
            and res_a.summaries[i].num_successful_steps == res_b.summaries[j].num_successful_steps
            and res_a.summaries[i].num_unsuccessful_steps == res_b.summaries[j].num_unsuccessful_steps
            and res_a.usable[i] == res_b.usable[j])


@pytest.mark.gpu
def test_trajectory_parity(gpu):
    """Counts 1, 2, 3, 4, 63, 64, 65, 257 and one above the LDS-resident limit
    (the streaming path), 10 % outliers of 40 px, pose only / focal / focal +
    extra on SIMPLE_RADIAL and OPENCV with focal + extra: the oracle's accept /
    reject sequence, termination, final cost within 1e-6 relative, qvec and
    tvec within 1e-5, intrinsics within 1e-5 relative (DESIGN 7's end-to-end
    LM figures).  Cases whose oracle stop moves under ulp perturbations of the
    inputs are not a fair comparison (at most one in ten)."""
    cases = pc.parity_cases()
    assert sum(not c[6] for c in cases) * 10 <= len(cases)
    fish = pc.fisheye_cases()
    by_flags = {}
    for k, c in enumerate(cases):
        by_flags.setdefault(pc.CONFIGS[c[0]][1:], []).append(k)
    for (rf, re), ks in by_flags.items():
        probs = [cases[k][2] for k in ks]
        if rf and re:
            probs = probs + [p for _, p in fish]  # mixed models in one call
        res, tr = run(probs, trace_cap=100, refine_focal_length=int(rf), refine_extra_params=int(re))
        assert np.all(res.statuses == mi_ba.OK) and np.all(res.usable == 1)
        for j, k in enumerate(ks):
            ci, n, pr, s, trace, sc, stable = cases[k]
            g = res.summaries[j]
            what = (ci, n)
            print(what, "gpu", g.num_successful_steps, g.num_unsuccessful_steps, g.termination_type,
                  "oracle", s.num_successful_steps, s.num_unsuccessful_steps, s.termination_type,
                  "dcost", abs(g.final_cost - s.final_cost) / s.final_cost,
                  "dq", np.abs(res.qvec[j] - sc.qvec[0]).max(), "dt", np.abs(res.tvec[j] - sc.tvec[0]).max())
            if not stable:
                continue
            assert g.num_residuals_reduced == 2 * n and g.num_effective_parameters_reduced == \
                s.num_effective_parameters_reduced
            assert abs(g.initial_cost - s.initial_cost) <= 1e-12 * s.initial_cost, what
            assert gpu_sequence(tr[j]) == oracle_sequence(trace), what
            assert g.termination_type == s.termination_type, what
            assert abs(g.final_cost - s.final_cost) <= 1e-6 * s.final_cost, what
            assert np.abs(res.qvec[j] - sc.qvec[0]).max() <= 1e-5 and np.abs(res.tvec[j] - sc.tvec[0]).max() <= 1e-5, what
            assert rel(res.camera_params[j], sc.camera_params[0]) <= 1e-5, what
            idx = mi_ba.pose_refine_intrinsics(pr.camera_model, rf, re)
            fixed = [m for m in range(len(pr.camera_params)) if m not in idx]
            assert np.array_equal(res.camera_params[j][fixed], pr.camera_params[fixed]), what
        if rf and re:
            # OPENCV_FISHEYE: the existing GPU solver on the equivalent scene
            for j, (n, pr) in enumerate(fish, start=len(ks)):
                sc = mi_ba.pose_problem_scene(pr)
                s = mi_ba.solve(pc.oracle_options(), sc)
                g = res.summaries[j]
                assert (g.num_successful_steps, g.num_unsuccessful_steps, g.termination_type) == \
                    (s.num_successful_steps, s.num_unsuccessful_steps, s.termination_type), n
                assert abs(g.final_cost - s.final_cost) <= 1e-6 * s.final_cost, n
                assert np.abs(res.qvec[j] - sc.qvec[0]).max() <= 1e-5 and np.abs(res.tvec[j] - sc.tvec[0]).max() <= 1e-5
                assert rel(res.camera_params[j], sc.camera_params[0]) <= 1e-5, n


@pytest.mark.gpu
@pytest.mark.parametrize("n", [4, 65])
def test_fixed_iteration_parity(gpu, n):
    """gradient_tolerance 0, three iterations: the parameters after exactly
    three iterations match the oracle within 1e-9 relative — a wrong damping,
    scaling or radius rule shows here, not after convergence."""
    pr = pc.make_problem(mi_ba.SIMPLE_RADIAL, n, 900 + n)
    s, trace, sc = pc.oracle_solve(pr, gradient_tolerance=0.0, max_num_iterations=3)
    res, tr = run([pr], trace_cap=8, gradient_tolerance=0.0, max_num_iterations=3)
    g = res.summaries[0]
    assert gpu_sequence(tr[0]) == oracle_sequence(trace) and len(trace) == 3
    assert g.termination_type == s.termination_type == mi_ba.NO_CONVERGENCE
    d = max(rel(res.qvec[0], sc.qvec[0]), rel(res.tvec[0], sc.tvec[0]), rel(res.camera_params[0], sc.camera_params[0]))
    print("fixed-iteration difference", n, d, "cost", abs(g.final_cost - s.final_cost) / s.final_cost)
    assert d <= 1e-9
    assert abs(g.final_cost - s.final_cost) <= 1e-9 * s.final_cost


@pytest.fixture(scope="module")
def batch130():
    probs = [pc.make_problem(mi_ba.SIMPLE_RADIAL if k % 2 else mi_ba.OPENCV, 20 + 3 * k, 2000 + k) for k in range(130)]
    probs[1] = probs[0].copy()
    probs[129] = probs[0].copy()
    return probs


@pytest.mark.gpu
def test_batch_position_and_run_to_run_bitwise(gpu, batch130):
    """The same problem at positions 0, 1 and last of a 130-problem batch, two
    runs of the batch, and the problem alone: bitwise identical."""
    a = run(batch130, covariance=True)
    b = run(batch130, covariance=True)
    assert np.all(a.usable == 1)
    assert same_bits(a, 0, a, 1) and same_bits(a, 0, a, 129)
    assert np.array_equal(a.covariance[0], a.covariance[1]) and np.array_equal(a.covariance[0], a.covariance[129])
    for k in range(130):
        assert same_bits(a, k, b, k), k
    assert np.array_equal(a.covariance, b.covariance)
    for k in (0, 64):
        one = run([batch130[k]], covariance=True)
        assert same_bits(one, 0, a, k) and np.array_equal(one.covariance[0], a.covariance[k])
    assert a.summaries[0].num_successful_steps >= 2


@pytest.mark.gpu
def test_inlier_mask(gpu):
    """Masks that remove the outliers equal the compacted arrays, bitwise; an
    all-zero mask does nothing."""
    masked, compact = [], []
    for k, n in enumerate((30, 65, 300)):
        pr = pc.make_problem(mi_ba.SIMPLE_RADIAL, n, 3000 + k, outlier_fraction=0.0)
        rng = np.random.default_rng(k)
        bad = rng.choice(n, n // 10, replace=False)
        pr.points2D[bad] += 40.0
        pr.inlier_mask = np.ones(n, np.uint8)
        pr.inlier_mask[bad] = 0
        masked.append(pr)
        keep = pr.inlier_mask != 0
        compact.append(mi_ba.PoseProblem(pr.camera_model, pr.camera_params.copy(), pr.qvec.copy(), pr.tvec.copy(),
                                         pr.points2D[keep].copy(), pr.points3D[keep].copy()))
    empty = pc.make_problem(mi_ba.SIMPLE_RADIAL, 12, 5)
    empty.inlier_mask = np.zeros(12, np.uint8)
    cov_in = np.full((4, 6, 6), 7.5)
    a = run(masked + [empty], covariance=cov_in)
    b = run(compact, covariance=True)
    for k in range(3):
        assert same_bits(a, k, b, k) and np.array_equal(a.covariance[k], b.covariance[k])
        assert a.summaries[k].num_residuals_reduced == 2 * int((masked[k].inlier_mask != 0).sum())
    s = a.summaries[3]
    assert a.usable[3] == 1 and a.statuses[3] == mi_ba.OK and s.termination_type == mi_ba.CONVERGENCE
    assert s.num_residuals_reduced == 0 and s.num_successful_steps == 0
    assert np.array_equal(a.qvec[3], empty.qvec) and np.array_equal(a.tvec[3], empty.tvec)
    assert np.array_equal(a.camera_params[3], empty.camera_params)
    assert np.all(a.covariance[3] == 7.5)


def covariance_reference(pr, res_k_params, rf, re):
    """numpy on oracle.reproj_eval at the given final point: the pose block of
    inv(J'J) over the pose and camera columns (loss-corrected Jacobians)."""
    q, t, cam = res_k_params
    final = mi_ba.PoseProblem(pr.camera_model, cam, q, t, pr.points2D, pr.points3D)
    opts = pc.oracle_options(refine_focal_length=rf, refine_extra_params=re)
    _, _, J = oracle.reproj_eval(opts, mi_ba.pose_problem_scene(final))
    cols = list(range(6)) + list(range(9, J.shape[2]))
    Jm = J[:, :, cols].reshape(-1, len(cols))
    return np.linalg.inv(Jm.T @ Jm)[:6, :6]


@pytest.mark.gpu
@pytest.mark.parametrize("n,rf,re", [(65, 0, 0), (300, 1, 1)])
def test_covariance(gpu, n, rf, re):
    """rot_tvec_covariance: symmetric to 1e-12 relative, within 1e-8 relative
    of the numpy reference's largest entry; a rank-deficient 1-point
    neighbour is not usable and disturbs nobody."""
    pr = pc.make_problem(mi_ba.SIMPLE_RADIAL, n, 4000 + n)
    one = pc.make_problem(mi_ba.SIMPLE_RADIAL, 1, 4001)
    cov_in = np.full((3, 6, 6), -3.0)
    res = run([one, pr, one.copy()], covariance=cov_in, refine_focal_length=rf, refine_extra_params=re)
    assert list(res.usable) == [0, 1, 0] and np.all(res.statuses == mi_ba.OK)
    assert np.all(res.covariance[0] == -3.0) and np.all(res.covariance[2] == -3.0)
    alone = run([pr], covariance=True, refine_focal_length=rf, refine_extra_params=re)
    assert same_bits(alone, 0, res, 1) and np.array_equal(alone.covariance[0], res.covariance[1])
    cov = res.covariance[1]
    ref = covariance_reference(pr, (res.qvec[1], res.tvec[1], res.camera_params[1]), rf, re)
    big = np.abs(ref).max()
    print("covariance", n, "asym", np.abs(cov - cov.T).max() / big, "diff", np.abs(cov - ref).max() / big)
    assert np.abs(cov - cov.T).max() <= 1e-12 * big
    assert np.abs(cov - ref).max() <= 1e-8 * big


@pytest.mark.gpu
def test_edge_semantics(gpu):
    good = [pc.make_problem(mi_ba.SIMPLE_RADIAL, 40, 5000 + k) for k in range(3)]
    # max_num_iterations 0
    res = run(good[:1], max_num_iterations=0)
    assert res.summaries[0].termination_type == mi_ba.NO_CONVERGENCE and res.usable[0] == 1
    assert np.array_equal(res.qvec[0], good[0].qvec) and np.array_equal(res.tvec[0], good[0].tvec)
    assert np.array_equal(res.camera_params[0], good[0].camera_params)
    assert res.summaries[0].initial_cost == res.summaries[0].final_cost > 0
    # an unsupported model and a NaN, between solvable neighbours
    ref = run(good)
    full = good[1].copy()
    full.camera_model = 6  # FULL_OPENCV
    full.camera_params = np.concatenate([full.camera_params, np.zeros(8)])
    nan = good[1].copy()
    nan.points3D[7, 1] = np.nan
    res = run([good[0], full, good[1], nan, good[2]])
    assert list(res.statuses) == [mi_ba.OK, mi_ba.ERR_UNSUPPORTED, mi_ba.OK, mi_ba.OK, mi_ba.OK]
    assert list(res.usable) == [1, 0, 1, 0, 1]
    assert res.summaries[3].termination_type == mi_ba.FAILURE
    assert np.array_equal(res.qvec[3], nan.qvec) and np.array_equal(res.tvec[3], nan.tvec)
    assert np.array_equal(res.camera_params[3], nan.camera_params)
    assert np.array_equal(res.qvec[1], full.qvec) and np.array_equal(res.camera_params[1], full.camera_params)
    for j, k in ((0, 0), (2, 1), (4, 2)):
        assert same_bits(res, j, ref, k)


@pytest.mark.gpu
@pytest.mark.parametrize("model", [mi_ba.SIMPLE_RADIAL, mi_ba.OPENCV])
def test_agrees_with_the_existing_gpu_solver(gpu, model):
    """300 correspondences: mi_ba.solve on the equivalent scene reaches the
    same final cost within 1e-6 relative with the same step counts."""
    pr = pc.make_problem(model, 300, 6000 + model)
    res = run([pr])
    sc = mi_ba.pose_problem_scene(pr)
    s = mi_ba.solve(pc.oracle_options(), sc)
    g = res.summaries[0]
    assert (g.num_successful_steps, g.num_unsuccessful_steps) == (s.num_successful_steps, s.num_unsuccessful_steps)
    assert abs(g.final_cost - s.final_cost) <= 1e-6 * s.final_cost
    assert g.num_successful_steps >= 3


# --------------------------------------------------------------------------- facade (C++)
def run_cpp(mode):
    """tests/cpp/pose_refinement_test.cc through include/colmap_amd/pose.h."""
    return run_program("pose_refinement_test", mode)


def test_pose_facade_host():
    """Options, Check() and the size checks throw without a device."""
    assert run_cpp("host").count("PASS") == 2


@pytest.mark.gpu
def test_pose_facade_gpu(gpu):
    """One SIMPLE_RADIAL problem with its covariance through RefineAbsolutePose,
    and the same problem through RefineAbsolutePoses: the same bits."""
    assert run_cpp("gpu").count("PASS") == 2
