"""Batched relative-pose refinement (mi_ba_refine_relative_pose_batch,
RefineRelativePose of the reference, pose.cc:324-352).

CPU: the defaults, the refusals, the ABI, the host build of
csrc/relative_pose_block.h against the independent reference
(relative_pose_reference: autograd Jacobians), SphereManifold<3> on every
branch, the reference against itself (the scene of the reference's
TestRefineEssentialMatrix, its Jacobian against central differences, the
stability cap of the parity cases) and the facade's host checks.  GPU:
evaluate parity, trajectory parity, the known answer, fixed-iteration parity,
bitwise properties, invariants and edges, and the C++ facade.

Tolerances: residuals and Jacobians the scaled 1e-10 of test_gpu_parity.py;
trajectories the bounds of test_generalized_pose.py (initial cost 1e-12
relative, final cost 1e-6 relative, q and t 1e-5 absolute; fixed iterations
1e-9 relative), each widened to ten times the reference's own spread under
ulp-perturbed inputs where that is larger (relative_pose_cases: on the
committed seeds it never is)."""
import ctypes as C
import os

import numpy as np
import pytest

import mi_ba
import relative_pose_cases as rc
import relative_pose_reference as rref
from estimator_testing import gpu_sequence, hexes, make, run_program

M = mi_ba


def opts(**kw):
    return M.default_relative_pose_options(**kw)


def write_problem(pr, path):
    """The text form the C++ tests read: q(4) t(3) n, then x1 y1 x2 y2 per line, hex floats."""
    with open(path, "w") as f:
        f.write(f"{hexes(pr.qvec)} {hexes(pr.tvec)}\n{len(pr.points1)}\n")
        for a, b in zip(pr.points1, pr.points2):
            f.write(f"{hexes(a)} {hexes(b)}\n")


def scaled_difference(got, want):
    """max |got - want| / max(1, max |want|) per row (test_gpu_parity.py)."""
    got, want = np.asarray(got).reshape(len(got), -1), np.asarray(want).reshape(len(want), -1)
    return float((np.abs(got - want).max(axis=1) / np.maximum(1.0, np.abs(want).max(axis=1))).max())


# --------------------------------------------------------------------------- CPU: ABI, defaults, refusals
def test_defaults_are_ceres_solver_options():
    o = opts()
    assert (o.max_num_iterations, o.function_tolerance, o.gradient_tolerance, o.parameter_tolerance) == \
        (50, 1e-6, 1e-10, 1e-8)
    assert o.loss_function_scale == 1.0 and o.device == 0


def test_new_symbols_are_declared():
    text = open(os.path.join(M._HERE, "..", "include", "mi_ba.h")).read()
    for name in ("mi_ba_relative_pose_options", "mi_ba_default_relative_pose_options", "mi_ba_relative_pose_batch",
                 "mi_ba_refine_relative_pose_batch", "mi_ba_relative_pose_lds_capacity",
                 "mi_ba_relative_pose_evaluate"):
        assert name in text
    assert "#define MI_BA_ABI_VERSION 4" in text
    assert M.load().mi_ba_abi_version() == 4


def test_lds_capacity():
    assert 64 <= M.relative_pose_lds_capacity() <= 8192


def solve_status(problems, o=None, mutate=None):
    a = M._RelativePoseArrays(problems)
    if mutate:
        mutate(a)
    n = len(problems)
    st, us = np.zeros(n, np.int32), np.zeros(n, np.int32)
    sums = (M.Summary * n)()
    return M.load().mi_ba_refine_relative_pose_batch(C.byref(o or opts()), C.byref(a.batch), st.ctypes.data_as(M._i32p),
                                                     C.cast(sums, C.c_void_p), us.ctypes.data_as(M._i32p))


def evaluate_status(problems, o=None, mutate=None):
    a = M._RelativePoseArrays(problems)
    if mutate:
        mutate(a)
    total = int(max(a.obs_off.max(), 1))
    r, J = np.zeros(total), np.zeros((total, 5))
    return M.load().mi_ba_relative_pose_evaluate(C.byref(o or opts()), C.byref(a.batch), r.ctypes.data_as(M._dp),
                                                 J.ctypes.data_as(M._dp))


@pytest.mark.parametrize("kw", [dict(function_tolerance=-1.0), dict(gradient_tolerance=-1e-300),
                                dict(parameter_tolerance=-1.0), dict(max_num_iterations=-1),
                                dict(loss_function_scale=-1.0), dict(function_tolerance=float("nan"))])
@pytest.mark.parametrize("call", [solve_status, evaluate_status])
def test_options_are_refused(kw, call):
    """Refused before any device is touched (this test needs none)."""
    two = [rc.make_problem(6, 1), rc.make_problem(5, 2)]
    assert call(two, opts(**kw)) == M.ERR_INVALID_ARGUMENT
    with pytest.raises(M.MiBaError) as e:
        M.refine_relative_pose_batch(opts(**kw), two)
    assert e.value.status == M.ERR_INVALID_ARGUMENT


@pytest.mark.parametrize("call", [solve_status, evaluate_status])
def test_arguments_are_refused(call):
    two = [rc.make_problem(6, 1), rc.make_problem(5, 2)]

    def decreasing(a):
        a.obs_off[1] = 12

    def negative_first(a):
        a.obs_off[0] = -1

    def no_points(a):
        a.batch.points2 = None

    def no_pose(a):
        a.batch.tvec = None

    for mutate in (decreasing, negative_first, no_points, no_pose):
        assert call(two, mutate=mutate) == M.ERR_INVALID_ARGUMENT, mutate.__name__
    b = M.RelativePoseBatch()
    b.num_problems = -1
    o = opts()
    assert M.load().mi_ba_refine_relative_pose_batch(C.byref(o), C.byref(b), None, None, None) == M.ERR_INVALID_ARGUMENT
    assert M.load().mi_ba_relative_pose_evaluate(C.byref(o), C.byref(b), None, None) == M.ERR_INVALID_ARGUMENT
    assert M.load().mi_ba_refine_relative_pose_batch(None, C.byref(b), None, None, None) == M.ERR_INVALID_ARGUMENT
    # an empty batch is fine and needs no device
    b.num_problems = 0
    assert M.load().mi_ba_refine_relative_pose_batch(C.byref(o), C.byref(b), None, None, None) == M.OK


def test_mismatched_sizes_are_refused():
    pr = rc.make_problem(6, 1)
    bad = pr.copy()
    bad.points2 = bad.points2[:5]
    with pytest.raises(ValueError):
        M.refine_relative_pose_batch(opts(), [bad])
    bad = pr.copy()
    bad.inlier_mask = np.ones(5, np.uint8)
    with pytest.raises(ValueError):
        M.refine_relative_pose_batch(opts(), [bad])


# --------------------------------------------------------------------------- CPU: the kernel's arithmetic on the host
def block_problem():
    """16 fixed correspondences, a quaternion that is not of unit length and a
    baseline that is not either."""
    pr = rc.make_problem(16, 77)
    pr.qvec = pr.qvec * 1.1
    pr.tvec = pr.tvec * 0.7
    return pr


def host_rows(target, pr, tmp_path):
    path = str(tmp_path / "rows.txt")
    write_problem(pr, path)
    out = run_program(target, "rows", path)
    rows = np.array([[float.fromhex(v) for v in l.split()[1:]] for l in out.splitlines() if l.startswith("ROW")])
    assert rows.shape == (len(pr.points1), 6)
    return rows[:, 0], rows[:, 1:]


def test_host_block_matches_autograd(tmp_path):
    """relative_pose_block.h compiled for the host: residuals and 5-wide
    tangent Jacobians against the reference's autograd values, scaled 1e-10."""
    pr = block_problem()
    r, J = host_rows("relative_pose_block_test", pr, tmp_path)
    r_ref, J_ref = rc.reference_problem(pr, normalize=False).evaluate()
    dr, dj = scaled_difference(r[:, None], r_ref[:, None]), scaled_difference(J, J_ref)
    print("host block: dr", dr, "dJ", dj, "relative dr", np.abs(r / r_ref - 1).max(), "relative dJ",
          (np.abs(J - J_ref).max(axis=1) / np.abs(J_ref).max(axis=1)).max())
    assert dr <= 1e-10 and dj <= 1e-10
    # the bound is absolute below 1: the values themselves are small, so the relative agreement is asserted too
    assert np.abs(r / r_ref - 1).max() <= 1e-10
    assert (np.abs(J - J_ref).max(axis=1) / np.abs(J_ref).max(axis=1)).max() <= 1e-10


def test_host_sphere_chart():
    """H x = |x| e3, |Plus(x, d)| = |x|, Plus(x, 0) = x and the PlusJacobian
    against a central difference, on every branch of the Householder vector."""
    out = run_program("relative_pose_block_test", "chart")
    assert out.count("PASS") == 8


def test_host_block_under_sanitizers(tmp_path):
    """The same stand-alone program built with AddressSanitizer and UBSan, run
    as a child process of its own (nothing is preloaded, nothing is loaded
    into Python).  A machine with a visible GPU builds it but does not run it."""
    binary = make("relative_pose_block_test_san")
    try:
        if M.device_count() > 0:
            return
    except Exception:
        pass
    pr = block_problem()
    r, J = host_rows("relative_pose_block_test_san", pr, tmp_path)
    r2, J2 = host_rows("relative_pose_block_test", pr, tmp_path)
    assert np.allclose(r, r2, rtol=1e-12, atol=0) and np.allclose(J, J2, rtol=1e-9, atol=1e-18)
    assert run_program("relative_pose_block_test_san", "chart").count("PASS") == 8
    assert os.path.exists(binary)


def test_reference_sphere_manifold():
    """The reference's own restatement of SphereManifold<3>: the same
    properties, on the same branches."""
    for x in ([0, 0, -1.0], [0, 0, 7.0], [0.3, -0.5, -0.81], [0.6, 0, 0], [-0.2, 0.4, 0.89], [2.1, -3.5, 4.2]):
        x = np.array(x, float)
        v, beta = rref.householder(x)
        nx = np.linalg.norm(x)
        assert np.abs((np.eye(3) - beta * np.outer(v, v)) @ x - [0, 0, nx]).max() <= 1e-15 * nx
        assert np.array_equal(rref.sphere_plus(x, np.zeros(2)), x)
        for d in ([0.3, -0.2], [1e-3, 2e-3], [-1.4, 2.5]):
            assert abs(np.linalg.norm(rref.sphere_plus(x, np.array(d))) - nx) <= 4e-16 * nx
        h = 1e-6
        fd = np.stack([(rref.sphere_plus(x, h * e) - rref.sphere_plus(x, -h * e)) / (2 * h) for e in np.eye(2)], 1)
        assert np.abs(fd - rref.sphere_plus_jacobian(x)).max() <= 1e-7 * nx


# --------------------------------------------------------------------------- CPU: the reference against itself
def test_reference_jacobian_matches_central_differences():
    """The autograd tangent Jacobian against central differences of the
    residual along Plus."""
    for pr in (block_problem(), rc.make_problem(9, 5, "neg_axis")):
        p = rc.reference_problem(pr, normalize=False)
        r, J = p.evaluate()
        h = 1e-6
        for k in range(5):
            d = np.zeros(5)
            d[k] = h
            qp, tp = p.plus(d)
            qm, tm = p.plus(-d)
            fd = (p._eval(qp, tp, False)[0] - p._eval(qm, tm, False)[0]) / (2 * h)
            assert np.abs(fd - J[:, k]).max() <= 1e-6 * max(np.abs(J[:, k]).max(), 1e-300), k


def essential_distance(E, q, t):
    return float(np.linalg.norm(E - rref.essential_matrix(q, t)))


def test_reference_refines_the_essential_scene():
    """The restated scene of the reference's TestRefineEssentialMatrix
    (essential_matrix_test.cc:169-205): ||E - E_refined|| <= ||E - E_perturbed||."""
    pr, E, Ep = rc.essential_scene()
    s = rc.reference_solve(pr)
    print("reference:", s.num_successful_steps, s.num_unsuccessful_steps, s.termination_type, s.initial_cost,
          s.final_cost, essential_distance(E, s.qvec, s.tvec), np.linalg.norm(E - Ep))
    assert s.termination_type == rref.CONVERGENCE and s.num_successful_steps >= 1
    assert essential_distance(E, s.qvec, s.tvec) <= np.linalg.norm(E - Ep)


def test_reference_cases_are_stable():
    """At most one parity case in ten may have a reference stop that rounding
    decides; the cases cover every count, both loss scales, both special
    baselines, and steps that are rejected."""
    cases = rc.parity_cases()
    assert sum(not c.stable for c in cases) * 10 <= len(cases)
    assert sum(not c.stable for c in rc.fixed_iteration_cases()) == 0
    assert sorted({c.count for c in cases}) == sorted(rc.counts())
    assert {c.scale == 1.0 for c in cases} == {True, False}
    by_name = {c.name: c for c in cases}
    start = by_name["n65-unit"].problem.tvec
    assert start[0] == 0 and start[1] == 0 and start[2] < 0
    assert by_name["n64-unit"].problem.tvec[2] > 0
    assert any((1, 0, 0) in c.result.trace for c in cases)
    assert all(c.result.termination_type == rref.CONVERGENCE for c in cases)


# --------------------------------------------------------------------------- CPU: facade
def test_relative_pose_facade_host():
    """Defaults, Check(), the size check and EssentialMatrixFromPose against hand values."""
    assert run_program("relative_pose_refinement_test", "host").count("PASS") == 3


# --------------------------------------------------------------------------- GPU
def run(problems, trace_cap=0, **kw):
    tr = np.zeros((len(problems), trace_cap), np.uint8) if trace_cap else None
    res = M.refine_relative_pose_batch(opts(**kw), problems, trace=tr)
    return (res, tr) if trace_cap else res


def same_bits(res_a, i, res_b, j):
    a, b = res_a.summaries[i], res_b.summaries[j]
    return (np.array_equal(res_a.qvec[i], res_b.qvec[j]) and np.array_equal(res_a.tvec[i], res_b.tvec[j])
            and a.final_cost == b.final_cost and a.initial_cost == b.initial_cost
            and a.num_successful_steps == b.num_successful_steps
            and a.num_unsuccessful_steps == b.num_unsuccessful_steps
            and a.termination_type == b.termination_type and res_a.usable[i] == res_b.usable[j])


@pytest.mark.gpu
def test_evaluate_parity(gpu):
    """relative_pose_evaluate on the count-65 and capacity + 1 cases against
    the reference's residuals and tangent Jacobians: scaled 1e-10."""
    by_name = {c.name: c for c in rc.parity_cases()}
    cases = [by_name["n65-unit"], by_name[f"n{rc.streaming_count()}-unit"]]
    got = M.relative_pose_evaluate(opts(), [c.problem for c in cases])
    for c, (r, J) in zip(cases, got):
        r_ref, J_ref = rc.reference_problem(c.problem, normalize=False).evaluate()
        dr, dj = scaled_difference(r[:, None], r_ref[:, None]), scaled_difference(J, J_ref)
        rel_r = np.abs(r / r_ref - 1).max()
        rel_j = (np.abs(J - J_ref).max(axis=1) / np.abs(J_ref).max(axis=1)).max()
        print(c.name, "dr", dr, "dJ", dj, "relative", rel_r, rel_j)
        assert dr <= 1e-10 and dj <= 1e-10, c.name
        assert rel_r <= 1e-9 and rel_j <= 1e-9, c.name


@pytest.mark.gpu
def test_trajectory_parity(gpu):
    """Every count at both loss scales: the reference's trace, termination
    and step counts, the initial cost within 1e-12 relative, the final cost
    within 1e-6 relative and q, t within 1e-5 (or ten times the reference's own
    spread).  The loss scale is an option of a call: one call per case."""
    cases = rc.parity_cases()
    assert sum(not c.stable for c in cases) * 10 <= len(cases)
    for c in cases:
        res, tr = run([c.problem], trace_cap=64, loss_function_scale=c.scale)
        g, s = res.summaries[0], c.result
        dq, dt = np.abs(res.qvec[0] - s.qvec).max(), np.abs(res.tvec[0] - s.tvec).max()
        print(c.name, "gpu", g.num_successful_steps, g.num_unsuccessful_steps, g.termination_type, "reference",
              s.num_successful_steps, s.num_unsuccessful_steps, s.termination_type, "dinitial",
              abs(g.initial_cost - s.initial_cost) / s.initial_cost, "dcost", abs(g.final_cost - s.final_cost),
              "bound", c.cost_bound(1e-6), "dq", dq, "dt", dt, "stable", c.stable)
        assert res.statuses[0] == M.OK and res.usable[0] == 1, c.name
        assert g.num_residuals_reduced == c.count and g.num_effective_parameters_reduced == 5, c.name
        assert np.all(np.isfinite(res.qvec[0])) and np.all(np.isfinite(res.tvec[0])) and np.isfinite(g.final_cost)
        assert abs(g.initial_cost - s.initial_cost) <= 1e-12 * s.initial_cost, c.name
        if not c.stable:
            continue
        assert gpu_sequence(tr[0]) == s.trace, c.name
        assert g.termination_type == s.termination_type, c.name
        assert (g.num_successful_steps, g.num_unsuccessful_steps) == \
            (s.num_successful_steps, s.num_unsuccessful_steps), c.name
        assert abs(g.final_cost - s.final_cost) <= c.cost_bound(1e-6), c.name
        assert dq <= c.qt_bound(1e-5) and dt <= c.qt_bound(1e-5), c.name


@pytest.mark.gpu
def test_known_answer(gpu):
    """The restated TestRefineEssentialMatrix scene through the GPU."""
    pr, E, Ep = rc.essential_scene()
    res = run([pr])
    assert res.usable[0] == 1 and res.summaries[0].num_successful_steps >= 1
    d = essential_distance(E, res.qvec[0], res.tvec[0])
    print("known answer:", d, np.linalg.norm(E - Ep))
    assert d <= np.linalg.norm(E - Ep)


@pytest.mark.gpu
def test_fixed_iteration_parity(gpu):
    """Every tolerance 0, three iterations, counts 5 and 65: parameters and
    cost within 1e-9 relative of the reference (or ten times its own spread)."""
    for c in rc.fixed_iteration_cases():
        res, tr = run([c.problem], trace_cap=8, max_num_iterations=3, function_tolerance=0.0, gradient_tolerance=0.0,
                      parameter_tolerance=0.0)
        g, s = res.summaries[0], c.result
        assert gpu_sequence(tr[0]) == s.trace and len(s.trace) == 3, c.name
        assert g.termination_type == s.termination_type == M.NO_CONVERGENCE
        dq, dt = np.abs(res.qvec[0] - s.qvec), np.abs(res.tvec[0] - s.tvec)
        print(c.name, "dq", dq.max(), "dt", dt.max(), "dcost", abs(g.final_cost - s.final_cost) / s.final_cost)
        assert np.all(dq <= np.maximum(1e-9 * np.abs(s.qvec), 10 * c.qt_spread)), c.name
        assert np.all(dt <= np.maximum(1e-9 * np.abs(s.tvec), 10 * c.qt_spread)), c.name
        assert abs(g.final_cost - s.final_cost) <= c.cost_bound(1e-9), c.name


@pytest.fixture(scope="module")
def batch70():
    probs = [rc.make_problem(10 + (37 * k) % 290, 2000 + k) for k in range(70)]
    probs[0] = rc.make_problem(200, 1999)
    probs[1] = probs[0].copy()
    probs[69] = probs[0].copy()
    probs[40] = rc.make_problem(rc.streaming_count() + 70, 1998)  # streams from device memory
    return probs


@pytest.mark.gpu
def test_batch_position_and_run_to_run_bitwise(gpu, batch70):
    """The same problem at positions 0, 1 and last of a 70-problem batch, two
    runs of the batch, and the problem alone (where the LDS arrays have another
    stride): bitwise identical; so is the streaming problem alone."""
    a = run(batch70)
    b = run(batch70)
    assert np.all(a.statuses == M.OK) and np.all(a.usable == 1)
    assert same_bits(a, 0, a, 1) and same_bits(a, 0, a, 69)
    for k in range(70):
        assert same_bits(a, k, b, k), k
    for k in (0, 7, 40):
        one = run([batch70[k]])
        assert same_bits(one, 0, a, k), k
    assert a.summaries[0].num_successful_steps >= 2 and a.summaries[40].num_successful_steps >= 2


@pytest.mark.gpu
def test_inlier_mask(gpu):
    """A masked call gives the bits of the compacted call; an all-zero mask
    does nothing."""
    masked, compact = [], []
    for k, n in enumerate((70, 300)):
        pr = rc.make_problem(n, 3000 + k, outlier_fraction=0.0)
        rng = np.random.default_rng(k)
        bad = rng.choice(n, n // 10, replace=False)
        pr.points2[bad] += rc.OUTLIER
        pr.inlier_mask = np.ones(n, np.uint8)
        pr.inlier_mask[bad] = 0
        masked.append(pr)
        keep = pr.inlier_mask != 0
        c = pr.copy()
        c.points1, c.points2, c.inlier_mask = pr.points1[keep], pr.points2[keep], None
        compact.append(c)
    empty = rc.make_problem(12, 5)
    empty.inlier_mask = np.zeros(12, np.uint8)
    empty.qvec = empty.qvec * 1.3
    a = run(masked + [empty])
    b = run(compact)
    for k in range(2):
        assert a.usable[k] == 1 and same_bits(a, k, b, k)
        assert a.summaries[k].num_residuals_reduced == int((masked[k].inlier_mask != 0).sum())
    s = a.summaries[2]
    assert a.usable[2] == 1 and a.statuses[2] == M.OK and s.termination_type == M.CONVERGENCE
    assert s.num_residuals_reduced == 0 and s.num_successful_steps == 0 and s.num_effective_parameters_reduced == 0
    assert np.array_equal(a.qvec[2], empty.qvec) and np.array_equal(a.tvec[2], empty.tvec)


@pytest.mark.gpu
def test_invariants(gpu):
    """|t| is kept to 1e-14 relative for |t| in {1, 0.1, 7}, |q| stays 1 within
    1e-14, and a q that is not of unit length is normalised first."""
    lengths = (1.0, 0.1, 7.0)
    probs = [rc.make_problem(120, 4000 + k, baseline=b) for k, b in enumerate(lengths)]
    scaled = probs[0].copy()
    scaled.qvec = scaled.qvec * 1.7
    res = run(probs + [scaled])
    assert np.all(res.usable == 1)
    for k, b in enumerate(lengths):
        assert res.summaries[k].num_successful_steps >= 2
        n0 = np.linalg.norm(probs[k].tvec)
        assert abs(n0 - b) <= 1e-15 * b
        assert abs(np.linalg.norm(res.tvec[k]) - n0) <= 1e-14 * n0, b
        assert abs(np.linalg.norm(res.qvec[k]) - 1.0) <= 1e-14, b
    # 1.7 q is normalised first: the path of q itself up to the rounding of the division
    assert res.summaries[3].num_successful_steps == res.summaries[0].num_successful_steps
    assert abs(np.linalg.norm(res.qvec[3]) - 1.0) <= 1e-14
    assert np.abs(res.qvec[3] - res.qvec[0]).max() <= 1e-9 and np.abs(res.tvec[3] - res.tvec[0]).max() <= 1e-9


@pytest.mark.gpu
def test_edge_semantics(gpu):
    good = [rc.make_problem(80, 5000 + k) for k in range(2)]
    # max_num_iterations 0: only the initial cost; q comes back normalised
    first = good[0].copy()
    first.qvec = first.qvec * 2.0
    res = run([first], max_num_iterations=0)
    s = res.summaries[0]
    assert s.termination_type == M.NO_CONVERGENCE and res.usable[0] == 1
    assert s.num_successful_steps == 0 and s.num_unsuccessful_steps == 0
    assert s.initial_cost == s.final_cost > 0
    assert np.array_equal(res.tvec[0], first.tvec)
    assert np.abs(res.qvec[0] - good[0].qvec).max() <= 4e-16 and abs(np.linalg.norm(res.qvec[0]) - 1) <= 4e-16
    # t = 0 and a NaN coordinate between solvable neighbours: FAILURE, usable 0, untouched
    ref = run(good)
    zero = good[0].copy()
    zero.tvec[:] = 0.0
    zero.qvec = zero.qvec * 1.5
    nan = good[1].copy()
    nan.points2[3, 0] = np.nan
    res, tr = run([good[0], zero, nan, good[1]], trace_cap=64)
    assert list(res.statuses) == [M.OK] * 4 and list(res.usable) == [1, 0, 0, 1]
    for k, pr in ((1, zero), (2, nan)):
        assert res.summaries[k].termination_type == M.FAILURE
        assert np.array_equal(res.qvec[k], pr.qvec) and np.array_equal(res.tvec[k], pr.tvec)
        assert gpu_sequence(tr[k]) == []
    assert same_bits(res, 0, ref, 0) and same_bits(res, 3, ref, 1)


@pytest.mark.gpu
def test_rank_deficient_counts(gpu):
    """One and four correspondences against five unknowns: no NaN, the
    reference's trace."""
    by_name = {c.name: c for c in rc.parity_cases()}
    for name in ("n1-unit", "n4-unit", "n1-knee", "n4-knee"):
        c = by_name[name]
        res, tr = run([c.problem], trace_cap=64, loss_function_scale=c.scale)
        assert res.usable[0] == 1
        assert np.all(np.isfinite(res.qvec[0])) and np.all(np.isfinite(res.tvec[0]))
        assert np.isfinite(res.summaries[0].final_cost)
        if c.stable:
            assert gpu_sequence(tr[0]) == c.result.trace, name


@pytest.mark.gpu
def test_relative_pose_facade_gpu(gpu, tmp_path):
    """RefineRelativePose and RefineRelativePoses on a problem written out as
    hex floats: the bits of the Python call."""
    pr = rc.make_problem(150, 9700)
    path = str(tmp_path / "problem.txt")
    write_problem(pr, path)
    out = run_program("relative_pose_refinement_test", "gpu", path)
    assert out.count("PASS") == 2
    res = run([pr])
    line = [l for l in out.splitlines() if l.startswith("RESULT")][0].split()
    vals = np.array([float.fromhex(v) for v in line[2:]])
    mine = np.concatenate([res.qvec[0], res.tvec[0]])
    assert int(line[1]) == res.usable[0] == 1
    assert np.array_equal(vals[:7], mine) and np.array_equal(vals[7:], mine)
