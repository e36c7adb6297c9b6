"""CPU tests of the rig problem assembly (mi_ba_rig_setup_stats, csrc/setup.cpp
build_rig_setup) against the reference's known answers
(tests/golden/rig_known_answers.json, transcribed from
src/optim/bundle_adjustment_test.cc:755-969) and of every validation error
where the reference CHECKs (RigBundleAdjuster::Solve :800-817,
AddImageToProblem :927-930, CameraRig::Check camera_rig.cc:86-110)."""
import json
import os

import numpy as np
import pytest

import mi_ba

GOLD = json.load(open(os.path.join(os.path.dirname(__file__), "golden", "rig_known_answers.json")))


def quat_mul(a, b):
    """Hamilton product a * b, (w, x, y, z)."""
    aw, ax, ay, az = a
    bw, bx, by, bz = b
    return np.array([aw * bw - ax * bx - ay * by - az * bz, aw * bx + ax * bw + ay * bz - az * by,
                     aw * by - ax * bz + ay * bw + az * bx, aw * bz + ax * by - ay * bx + az * bw])


def quat_rotate(q, p):
    q = np.asarray(q, float) / np.linalg.norm(q)
    return quat_mul(quat_mul(q, np.concatenate([[0.0], p])), q * np.array([1, -1, -1, -1]))[1:]


def concatenate_poses(q1, t1, q2, t2):
    """ConcatenatePoses (src/base/pose.cc:183-190)."""
    q = quat_mul(np.asarray(q2, float) / np.linalg.norm(q2), np.asarray(q1, float) / np.linalg.norm(q1))
    return q / np.linalg.norm(q), np.asarray(t2, float) + quat_rotate(q2, np.asarray(t1, float))


def compute_absolute_pose(sc, images, rel_q, rel_t):
    """CameraRig::ComputeAbsolutePose (camera_rig.cc:230-258) in numpy: the
    average (AverageQuaternions: dominant eigenvector) of the images' poses
    taken back through their cameras' relative poses."""
    qs, t = [], np.zeros(3)
    for i in images:
        rq, rt = rel_q[int(sc.image_camera[i])], rel_t[int(sc.image_camera[i])]
        inv = np.asarray(rq, float) * np.array([1, -1, -1, -1])
        q = quat_mul(inv / np.linalg.norm(inv), sc.qvec[i] / np.linalg.norm(sc.qvec[i]))
        qs.append(q / np.linalg.norm(q))
        t += quat_rotate(inv, sc.tvec[i] - rt)
    if len(qs) == 1:
        return qs[0], t
    A = sum(np.outer(q, q) for q in qs) / len(qs)
    w, v = np.linalg.eigh(A)
    return v[:, 3], t / len(qs)


def build_case(case):
    g = GOLD["bundle_adjustment"]
    sc = mi_ba.generate_scene(mi_ba.synth_config(mi_ba.MODEL_NAMES[g["model"]], case["images"], case["points"]))
    sc.image_camera = np.asarray(case["image_camera"], np.int32)
    cfg = np.zeros(case["images"], np.uint8)
    cfg[case["config_images"]] = 1
    sc.image_in_config = cfg
    cams = case["rig_cameras"]
    rel_q = {c: np.array(g["rel_qvec"], float) for c in cams}
    rel_t = {c: np.array(g["rel_tvec"], float) for c in cams}
    poses = [compute_absolute_pose(sc, sn, rel_q, rel_t) for sn in case["snapshots"]]
    rig = mi_ba.RigInput(
        rigs=[dict(cameras=cams, ref_camera=case["ref_camera"], rel_qvec=[rel_q[c] for c in cams],
                   rel_tvec=[rel_t[c] for c in cams], snapshots=case["snapshots"])],
        snapshot_qvec=np.array([p[0] for p in poses]), snapshot_tvec=np.array([p[1] for p in poses]),
        refine_relative_poses=case["refine_relative_poses"])
    return sc, rig


def test_default_rig():
    r = mi_ba.Rig()
    mi_ba.load().mi_ba_default_rig(r)
    assert r.num_rigs == 0 and r.refine_relative_poses == 1 and r.max_reproj_error == 1000.0


@pytest.mark.parametrize("case", GOLD["bundle_adjustment"]["cases"], ids=lambda c: c["name"])
def test_rig_counts(case):
    sc, rig = build_case(case)
    info = mi_ba.rig_setup_stats(mi_ba.default_options(), sc, rig)
    assert info.num_residuals_reduced == case["num_residuals_reduced"]
    assert info.num_effective_parameters_reduced == case["num_effective_parameters_reduced"]
    assert info.camera_tangent_size == 2
    # the images of no rig keep their own pose
    in_rig = {i for sn in case["snapshots"] for i in sn}
    assert info.num_variable_images == len(set(case["config_images"]) - in_rig)


def four_view():
    return build_case([c for c in GOLD["bundle_adjustment"]["cases"] if c["name"] == "TestRigFourView"][0])


def test_rig_filter_drops_an_observation():
    """An observation beyond max_reproj_error at the concatenated pose is not
    added (bundle_adjustment.cc:970-975): two residuals fewer; its point has a
    track longer than its observations and turns constant
    (ParameterizePoints, :518-530): three parameters fewer."""
    sc, rig = four_view()
    base = mi_ba.rig_setup_stats(mi_ba.default_options(), sc, rig)
    k = int(np.flatnonzero(sc.obs_image == 2)[5])
    sc.obs_xy[k] += 5000.0
    info = mi_ba.rig_setup_stats(mi_ba.default_options(), sc, rig)
    assert info.num_residuals_reduced == base.num_residuals_reduced - 2
    assert info.num_effective_parameters_reduced == base.num_effective_parameters_reduced - 3
    # with a bound that admits it nothing is dropped
    rig.max_reproj_error = 1e5
    info = mi_ba.rig_setup_stats(mi_ba.default_options(), sc, rig)
    assert info.num_residuals_reduced == base.num_residuals_reduced
    # a free image's observations are never filtered
    sc2, rig2 = build_case([c for c in GOLD["bundle_adjustment"]["cases"] if c["name"] == "TestRigFourViewPartial"][0])
    k = int(np.flatnonzero(sc2.obs_image == 3)[5])
    sc2.obs_xy[k] += 5000.0
    assert mi_ba.rig_setup_stats(mi_ba.default_options(), sc2, rig2).num_residuals_reduced == 800


def test_rig_point_behind_the_camera_is_dropped():
    """DBL_MAX behind the camera (projection.cc:137-140) exceeds every bound."""
    sc, rig = four_view()
    k = int(np.flatnonzero(sc.obs_image == 0)[0])
    # the only observation moved: give it a point of its own behind the rig
    sc.xyz = np.vstack([sc.xyz, [[0.0, 0.0, -50.0]]])
    sc.obs_point = sc.obs_point.copy()
    sc.obs_point[k] = sc.num_points - 1
    rig.max_reproj_error = 1e150
    info = mi_ba.rig_setup_stats(mi_ba.default_options(), sc, rig)
    assert info.num_residuals_reduced == 800 - 2


def invalid(sc, rig):
    with pytest.raises(mi_ba.MiBaError) as e:
        mi_ba.rig_setup_stats(mi_ba.default_options(), sc, rig)
    assert e.value.status == mi_ba.ERR_INVALID_ARGUMENT


def two_rigs(sc, rig, cameras_b, snapshots_b, ref_b):
    a = rig.rigs[0]
    b = dict(cameras=cameras_b, ref_camera=ref_b, rel_qvec=[[1, 0, 0, 0]] * len(cameras_b),
             rel_tvec=[[0, 0, 0]] * len(cameras_b), snapshots=snapshots_b)
    n = sum(len(r["snapshots"]) for r in (a, b))
    return mi_ba.RigInput(rigs=[a, b], snapshot_qvec=np.tile([1.0, 0, 0, 0], (n, 1)), snapshot_tvec=np.zeros((n, 3)))


def test_rig_validation_errors():
    sc, rig = four_view()
    mi_ba.rig_setup_stats(mi_ba.default_options(), sc, rig)  # the base case is valid
    # a camera in two rigs
    sc, rig = four_view()
    rig.rigs[0]["snapshots"] = [[0, 1]]
    invalid(sc, two_rigs(sc, rig, [1, 2], [], 1))
    # an image in two snapshots
    sc, rig = four_view()
    rig.rigs[0]["snapshots"] = [[0, 1], [0, 3]]
    invalid(sc, rig)
    # an image in two rigs: cameras 2, 3 form a second rig, image 0 listed in both
    sc, rig = four_view()
    sc.image_camera = np.array([0, 1, 2, 3], np.int32)
    rig.rigs[0]["snapshots"] = [[0, 1]]
    mi_ba.rig_setup_stats(mi_ba.default_options(), sc, two_rigs(sc, rig, [2, 3], [[2, 3]], 2))  # valid
    invalid(sc, two_rigs(sc, rig, [2, 3], [[2, 0]], 2))
    # a snapshot image whose camera is not in the rig
    sc, rig = four_view()
    sc.image_camera = np.array([0, 1, 0, 2], np.int32)
    invalid(sc, rig)
    # two images of one snapshot with the same camera
    sc, rig = four_view()
    rig.rigs[0]["snapshots"] = [[0, 2], [1, 3]]
    invalid(sc, rig)
    # a rig image with a constant pose / a constant tvec
    sc, rig = four_view()
    sc.image_constant_pose = np.array([0, 1, 0, 0], np.uint8)
    invalid(sc, rig)
    sc, rig = four_view()
    sc.image_constant_tvec = np.array([0, 0, 1, 0], np.uint8)
    invalid(sc, rig)
    # ... which an image of no rig may have
    sc, rig = build_case([c for c in GOLD["bundle_adjustment"]["cases"] if c["name"] == "TestRigFourViewPartial"][0])
    sc.image_constant_pose = np.array([0, 0, 0, 1], np.uint8)
    assert mi_ba.rig_setup_stats(mi_ba.default_options(), sc, rig).num_effective_parameters_reduced == 328 - 6
    # no reference camera: unset, not a camera of the rig, or a snapshot without its image
    for ref in (-1, 2):
        sc, rig = four_view()
        rig.rigs[0]["ref_camera"] = ref
        invalid(sc, rig)
    sc, rig = four_view()
    rig.rigs[0]["snapshots"] = [[0, 1], [3]]
    invalid(sc, rig)
    # an empty snapshot, an image that does not exist
    sc, rig = four_view()
    rig.rigs[0]["snapshots"] = [[0, 1], []]
    invalid(sc, rig)
    sc, rig = four_view()
    rig.rigs[0]["snapshots"] = [[0, 1], [2, 7]]
    invalid(sc, rig)
