"""CPU checks of the independent rig reference (tests/rig_reference.py) itself:
the reference's known residuals (tests/golden/rig_known_answers.json, from
src/base/cost_functions_test.cc:101-132, compared exactly), its complex-step
Jacobian against central finite differences along the manifold, the counts of
src/optim/bundle_adjustment_test.cc:755-969 through its own set-up rules, and
its LM on a scene that satisfies the rig constraint exactly."""
import json
import os

import numpy as np
import pytest

import mi_ba
import rig_reference as ref
import rig_scenes
from test_rig_setup import build_case

GOLD = json.load(open(os.path.join(os.path.dirname(__file__), "golden", "rig_known_answers.json")))


def test_rig_cost_function_known_answers():
    g = GOLD["cost_function"]
    for case in g["cases"]:
        prm = np.zeros((1, 8))
        prm[0, :3] = case["camera"]
        # SIMPLE_PINHOLE (f, cx, cy) is SIMPLE_RADIAL with k = 0: (f, cx, cy, 0)
        r = ref.rig_residual(np.array([ref.SIMPLE_RADIAL]), np.array([g["rig_qvec"]], float),
                             np.array([g["rig_tvec"]], float), np.array([g["rel_qvec"]], float),
                             np.array([g["rel_tvec"]], float), np.array([case["point3D"]], float), prm,
                             np.array([g["observed"]], float))
        assert r[0].tolist() == [float(v) for v in case["residual"]], case  # BOOST_CHECK_EQUAL: exact


@pytest.mark.parametrize("case", GOLD["bundle_adjustment"]["cases"], ids=lambda c: c["name"])
def test_reference_counts(case):
    sc, rig = build_case(case)
    prob = rig_scenes.reference_problem(mi_ba.default_options(), sc, rig)
    assert prob.num_residuals_reduced == case["num_residuals_reduced"]
    assert prob.num_effective_parameters_reduced == case["num_effective_parameters_reduced"]


def test_reference_counts_match_product_setup_on_the_base_scene():
    for kw in (dict(), dict(refine=0), dict(const_cam=2), dict(const_pts=True)):
        sc, rig = rig_scenes.base_scene(seed=3)
        sc.point_config = (np.arange(sc.num_points) % 6 == 0).astype(np.uint8)
        if kw.get("const_pts"):
            sc.point_config[np.arange(sc.num_points) % 5 == 1] = 2
        if "const_cam" in kw:
            sc.camera_constant = np.zeros(sc.num_cameras, np.uint8)
            sc.camera_constant[kw["const_cam"]] = 1
        rig.refine_relative_poses = kw.get("refine", 1)
        opts = mi_ba.default_options()
        info = mi_ba.rig_setup_stats(opts, sc, rig)
        prob = rig_scenes.reference_problem(opts, sc, rig)
        assert info.num_residuals_reduced == prob.num_residuals_reduced
        assert info.num_effective_parameters_reduced == prob.num_effective_parameters_reduced


def test_reference_jacobian_matches_finite_differences():
    """Central differences along the manifold, h = 1e-6: truncation ~h^2 |f'''|,
    rounding ~eps |f| / h ~ 1e-7 on pixel residuals of a few hundred; 1e-5
    relative to the block's largest entry covers both."""
    sc, rig = rig_scenes.base_scene(seed=1)
    prob = rig_scenes.reference_problem(mi_ba.default_options(), sc, rig)
    _, J = prob.block_jacobians()
    m, rq, rt, lq, lt, X, prm = prob._gather(prob.blk, prob.poses, prob.points, prob.cams)
    base = [rq, rt, lq, lt, X, prm]
    h, col = 1e-6, 0
    for which, dim in ((0, 3), (1, 3), (2, 3), (3, 3), (4, 3), (5, 8)):
        for k in range(dim):
            out = []
            for sgn in (1, -1):
                args = [a.copy() for a in base]
                d = np.zeros((len(prob.blk), dim))
                d[:, k] = sgn * h
                args[which] = ref.quat_plus(args[which], d) if which in (0, 2) else args[which] + d
                out.append(ref.rig_residual(m, *args, prob.xy))
            fd = (out[0] - out[1]) / (2 * h)
            scale = np.maximum(1.0, np.abs(J).reshape(len(J), -1).max(1))[:, None]
            assert np.abs(fd - J[:, :, col]).max() <= 1e-5 * scale.max(), (which, k)
            assert np.all(np.abs(fd - J[:, :, col]) <= 1e-5 * scale)
            col += 1


def test_reference_lm_converges_on_an_exact_rig_scene():
    """Noise-free observations of a scene that satisfies the rig constraint:
    the rig problem has a zero-cost solution and the LM finds it."""
    sc, rig = rig_scenes.base_scene(seed=2, noise=0.0)
    # every track the outside image sees is a variable point (AddVariablePoint):
    # no perturbed point stays constant, so the truth is reachable
    sc.point_config = (np.arange(sc.num_points) % 3 == 0).astype(np.uint8)
    prob = rig_scenes.reference_problem(mi_ba.default_options(), sc, rig)
    out = prob.solve(max_num_iterations=30)
    assert out["initial_cost"] > 1.0
    assert out["final_cost"] <= 1e-16 * out["initial_cost"]
    assert out["num_successful_steps"] >= 3


def test_reference_converged_cost_is_no_higher_than_the_free_image_oracle():
    """On a scene that satisfies the rig constraint exactly (no noise, every
    image in the config, every point variable) the rig problem's minimum is
    the free-image problem's, zero: the rig reference's converged cost is no
    higher than the oracle's free-image solve, up to the rounding floor of a
    cost evaluated from residuals of ~1e-13 px (1e-14 of the initial cost)."""
    import oracle
    sc, rig = rig_scenes.base_scene(seed=5, noise=0.0, num_outside=0)
    opts = mi_ba.default_options(max_num_iterations=40)
    prob = rig_scenes.reference_problem(opts, sc, rig)
    out = prob.solve(max_num_iterations=40)
    free = sc.copy()
    s = oracle.solve(opts, free)
    print(f"rig reference {out['final_cost']:.3g}, free-image oracle {s.final_cost:.3g}, initial {s.initial_cost:.3g}")
    assert out["final_cost"] <= s.final_cost + 1e-14 * out["initial_cost"]
    assert s.final_cost <= 1e-14 * s.initial_cost  # the free solve did converge
