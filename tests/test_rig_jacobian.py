"""Rig Jacobian parity: mi_ba_rig_evaluate (the reprojection kernel's per-image
Jacobian times the device records A_i, B_i the solver's projection uses)
against the independent reference's complex-step Jacobian over the cost
function's six parameter blocks (tests/rig_reference.py), block by block, on
the base scene and with the reference camera last.

Bound: the one tests/test_gpu_parity.py applies to the analytic-vs-Jet
Jacobian, max|dJ| <= 1e-10 * max(1, max|J|) per block, on every column (rig
pose, relative pose, point, refined intrinsics); the rig columns did not need
more (measured 2e-13, printed below).  Residuals: 1e-9 as there."""
import numpy as np
import pytest

import mi_ba
import rig_scenes

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("ref_pos", [0, 2])
@pytest.mark.parametrize("refine", [1, 0])
def test_rig_jacobian_matches_reference(gpu, ref_pos, refine):
    sc, rig = rig_scenes.base_scene(seed=11, ref_pos=ref_pos)
    sc.point_config = (np.arange(sc.num_points) % 6 == 0).astype(np.uint8)
    sc.point_config[np.arange(sc.num_points) % 5 == 1] = 2
    rig.refine_relative_poses = refine
    opts = mi_ba.default_options()
    prob = rig_scenes.reference_problem(opts, sc, rig)
    r_ref, J_ref = prob.block_jacobians()
    bo, r, J = mi_ba.rig_evaluate(opts, sc, rig)
    ct = J.shape[2] - 15
    assert sorted(bo.tolist()) == sorted(prob.obs.tolist())
    pos = {int(k): i for i, k in enumerate(prob.obs)}
    sel = np.array([pos[int(k)] for k in bo])
    # the reference's Jacobian in the download's layout: columns of constant
    # blocks zero, the refined intrinsics in their tangent slots
    want = np.zeros((len(bo), 2, 15 + ct))
    structural_zero = np.ones(want.shape, bool)
    n_rig = n_rel = n_free = 0
    for g, b in enumerate(sel):
        ip, il, ipt, ic = prob.blk[b]
        if prob.pose_off[ip] >= 0:
            want[g, :, 0:6] = J_ref[b, :, 0:6]
            structural_zero[g, :, 0:6] = False
        if prob.pose_off[il] >= 0:
            want[g, :, 6:12] = J_ref[b, :, 6:12]
            structural_zero[g, :, 6:12] = False
            n_rel += 1
        n_rig += ip < prob.layout["nsnap"]
        n_free += ip > prob.layout["ident"] and prob.pose_off[ip] >= 0
        if prob.pt_off[ipt] >= 0:
            want[g, :, 12:15] = J_ref[b, :, 12:15]
            structural_zero[g, :, 12:15] = False
        if prob.cam_off[ic] >= 0:
            for j, idx in enumerate(prob.cam_idx[ic]):
                want[g, :, 15 + j] = J_ref[b, :, 15 + idx]
                structural_zero[g, :, 15 + j] = False
    assert n_rig > 100 and n_free > 20 and (n_rel > 50) == bool(refine)
    assert np.abs(r - r_ref[sel]).max() <= 1e-9
    scale = np.maximum(1.0, np.abs(want).reshape(len(bo), -1).max(axis=1))[:, None, None]
    err = np.abs(J - want) / scale
    print(f"ref_pos {ref_pos} refine {refine}: max scaled |dJ| rig pose {err[:, :, 0:6].max():.3g}, "
          f"relative pose {err[:, :, 6:12].max():.3g}, point {err[:, :, 12:15].max():.3g}, "
          f"intrinsics {err[:, :, 15:].max():.3g}")
    assert err.max() <= 1e-10
    # the zero pattern is exact: constant blocks, images of no rig, padding slots
    assert np.all(J[structural_zero] == 0)
