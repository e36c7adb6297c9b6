"""Small rig scenes for the rig tests, and their translation into the
independent reference's problem (tests/rig_reference.py) by the set-up rules
of RigBundleAdjuster::SetUp (src/optim/bundle_adjustment.cc:871-1058)."""
import numpy as np

import mi_ba
import rig_reference as ref


def small_quat(rng, scale):
    v = rng.uniform(-scale, scale, 3)
    q = np.concatenate([[1.0], v])
    return q / np.linalg.norm(q)


def concat(rig_q, rig_t, rel_q, rel_t):
    q = ref.quat_product(np.asarray(rel_q, float), np.asarray(rig_q, float))
    return q, ref.unit_quat_rotate(np.asarray(rel_q, float), np.asarray(rig_t, float)) + np.asarray(rel_t, float)


def base_scene(seed=0, num_cameras=3, num_snapshots=4, num_free=2, num_outside=1, num_points=60, noise=0.3,
               perturb=1.0, opencv_camera=1, ref_pos=0):
    """num_cameras x num_snapshots rig images (snapshot-major), num_free images
    of no rig, num_outside images outside the config seen by some tracks;
    SIMPLE_RADIAL cameras with one OPENCV camera in the rig.  The
    observations satisfy the rig constraint (plus pixel noise); the returned
    parameters are perturbed from the truth by `perturb`."""
    rng = np.random.default_rng(seed)
    C = num_cameras + num_free + num_outside
    models = np.full(C, mi_ba.SIMPLE_RADIAL, np.int32)
    if opencv_camera is not None:
        models[opencv_camera] = mi_ba.OPENCV
    cams = []
    for c in range(C):
        if models[c] == mi_ba.SIMPLE_RADIAL:
            cams.append([500.0 + 10 * c, 250.0, 250.0, 0.02])
        else:
            cams.append([510.0, 505.0, 250.0, 250.0, 0.02, -0.01, 1e-3, -1e-3])
    rel_q = [np.array([1.0, 0, 0, 0]) if c == ref_pos else small_quat(rng, 0.05) for c in range(num_cameras)]
    rel_t = [np.zeros(3) if c == ref_pos else np.array([0.3 * (c - ref_pos), 0.05 * c, 0.0]) for c in range(num_cameras)]
    snap_q = [small_quat(rng, 0.05) for _ in range(num_snapshots)]
    snap_t = [rng.uniform(-0.3, 0.3, 3) for _ in range(num_snapshots)]
    qv, tv, icam, snaps = [], [], [], []
    for s in range(num_snapshots):
        snaps.append([])
        for c in range(num_cameras):
            q, t = concat(snap_q[s], snap_t[s], rel_q[c], rel_t[c])
            snaps[-1].append(len(qv))
            qv.append(q), tv.append(t), icam.append(c)
    for f in range(num_free + num_outside):
        qv.append(small_quat(rng, 0.05)), tv.append(rng.uniform(-0.3, 0.3, 3)), icam.append(num_cameras + f)
    I = len(qv)
    qv, tv, icam = np.array(qv), np.array(tv), np.array(icam, np.int32)
    X = rng.uniform(-1, 1, (num_points, 3)) + np.array([0, 0, 5.0])
    oi, op, oxy = [], [], []
    for p in range(num_points):
        seen = np.flatnonzero(rng.uniform(size=I) < 0.7)
        if len(seen) < 2:
            seen = np.array([0, 1])
        for i in seen:
            if i >= I - num_outside and p % 3:  # the outside images see some tracks only
                continue
            oi.append(i), op.append(p)
    oi, op = np.array(oi, np.int32), np.array(op, np.int32)
    prm = np.zeros((C, 8))
    for c in range(C):
        prm[c, :len(cams[c])] = cams[c]
    ident_q, ident_t = np.tile([1.0, 0, 0, 0], (len(oi), 1)), np.zeros((len(oi), 3))
    oxy = ref.rig_residual(models[icam[oi]], qv[oi], tv[oi], ident_q, ident_t, X[op], prm[icam[oi]],
                           np.zeros((len(oi), 2)))
    oxy = oxy + noise * rng.standard_normal(oxy.shape)
    # perturbed start
    e = perturb
    snap_q = [ref.quat_plus(q, e * rng.uniform(-0.005, 0.005, 3)) for q in snap_q]
    snap_t = [t + e * rng.uniform(-0.02, 0.02, 3) for t in snap_t]
    for c in range(num_cameras):
        if c != ref_pos:
            rel_q[c] = ref.quat_plus(rel_q[c], e * rng.uniform(-0.005, 0.005, 3))
            rel_t[c] = rel_t[c] + e * rng.uniform(-0.02, 0.02, 3)
    for i in range(num_cameras * num_snapshots, I - num_outside):
        qv[i] = ref.quat_plus(qv[i], e * rng.uniform(-0.005, 0.005, 3))
        tv[i] = tv[i] + e * rng.uniform(-0.02, 0.02, 3)
    X = X + e * rng.uniform(-0.02, 0.02, X.shape)
    in_cfg = np.ones(I, np.uint8)
    in_cfg[I - num_outside:] = 0
    sc = mi_ba.Scene(mi_ba.SIMPLE_RADIAL, np.concatenate([np.asarray(c, float) for c in cams]), qv, tv, icam, X, oxy,
                     oi, op, image_in_config=in_cfg, camera_models=models)
    rig = mi_ba.RigInput(rigs=[dict(cameras=list(range(num_cameras)), ref_camera=ref_pos, rel_qvec=np.array(rel_q),
                                    rel_tvec=np.array(rel_t), snapshots=snaps)],
                         snapshot_qvec=np.array(snap_q), snapshot_tvec=np.array(snap_t))
    return sc, rig


def reference_problem(opts, sc, rig):
    """The scene as the independent reference's problem.  Pose table: the
    snapshots' rig poses, the rig cameras' relative poses (rigs back to back),
    one identity, then every image's own pose."""
    r = rig.struct()  # flattens rel_qvec / rel_tvec / snapshot poses
    I = sc.num_images
    in_cfg = np.ones(I, bool) if sc.image_in_config is None else sc.image_in_config.astype(bool)
    const_pose = np.zeros(I, bool) if sc.image_constant_pose is None else sc.image_constant_pose.astype(bool)
    nsnap, ncam = len(rig.snapshot_qvec), len(rig.rel_qvec)
    ident = nsnap + ncam
    poses = np.vstack([np.hstack([rig.snapshot_qvec, rig.snapshot_tvec]), np.hstack([rig.rel_qvec, rig.rel_tvec]),
                       [[1.0, 0, 0, 0, 0, 0, 0]], np.hstack([sc.qvec, sc.tvec])])
    pose_var = np.zeros(len(poses), bool)
    img_snap, img_rel = np.full(I, -1), np.full(I, -1)
    refine_rel = 1 if rig.refine_relative_poses is None else rig.refine_relative_poses
    max_err = 1000.0 if rig.max_reproj_error is None else rig.max_reproj_error
    k0 = s0 = 0
    for g in rig.rigs:
        for si, snap in enumerate(g["snapshots"]):
            for i in snap:
                img_snap[i] = s0 + si
                img_rel[i] = k0 + list(g["cameras"]).index(int(sc.image_camera[i]))
        for ci, c in enumerate(g["cameras"]):
            pose_var[nsnap + k0 + ci] = bool(refine_rel) and c != g["ref_camera"]
        k0 += len(g["cameras"])
        s0 += len(g["snapshots"])
    pose_var[:nsnap] = True
    off = sc.camera_param_offsets()
    C = sc.num_cameras
    models = sc.camera_models if sc.camera_models is not None else np.full(C, sc.camera_model)
    cams = np.zeros((C, 8))
    for c in range(C):
        cams[c, :off[c + 1] - off[c]] = sc.camera_params.reshape(-1)[off[c]:off[c + 1]]
    P = sc.num_points
    track = np.bincount(sc.obs_point, minlength=P)
    nobs = np.zeros(P, int)
    cam_in = np.zeros(C, bool)
    cam_const = np.zeros(C, bool) if sc.camera_constant is None else sc.camera_constant.astype(bool).copy()
    blk, xy, obs = [], [], []
    # AddImageToProblem
    for i in range(I):
        if not in_cfg[i]:
            continue
        ks = np.flatnonzero(sc.obs_image == i)
        added = 0
        for k in ks:
            p, c = int(sc.obs_point[k]), int(sc.image_camera[i])
            if img_snap[i] >= 0:
                ip, il = img_snap[i], nsnap + img_rel[i]
                q, t = concat(poses[ip, :4] / np.linalg.norm(poses[ip, :4]), poses[ip, 4:],
                              poses[il, :4] / np.linalg.norm(poses[il, :4]), poses[il, 4:])
                Pc = ref.unit_quat_rotate(q / np.linalg.norm(q), sc.xyz[p]) + t
                if Pc[2] < np.finfo(float).eps:
                    continue
                x, y = ref.world_to_image(models[c:c + 1], cams[c:c + 1], Pc[0:1] / Pc[2], Pc[1:2] / Pc[2])
                if (x[0] - sc.obs_xy[k, 0]) ** 2 + (y[0] - sc.obs_xy[k, 1]) ** 2 > max_err * max_err:
                    continue
            else:
                ip, il = ident + 1 + i, ident
            blk.append((ip, il, p, c)), xy.append(sc.obs_xy[k]), obs.append(int(k))
            added += 1
            nobs[p] += 1
        if added:
            cam_in[sc.image_camera[i]] = True
            if img_snap[i] < 0:
                pose_var[ident + 1 + i] = not const_pose[i]
    # AddPointToProblem
    pc = np.zeros(P, np.uint8) if sc.point_config is None else sc.point_config
    for want in (1, 2):
        for p in np.flatnonzero(pc == want):
            if nobs[p] == track[p]:
                continue
            for k in np.flatnonzero(sc.obs_point == p):
                i = int(sc.obs_image[k])
                if in_cfg[i]:
                    continue
                nobs[p] += 1
                c = int(sc.image_camera[i])
                if not cam_in[c]:
                    cam_in[c] = True
                    cam_const[c] = True
                blk.append((ident + 1 + i, ident, int(p), c)), xy.append(sc.obs_xy[k]), obs.append(int(k))
    point_var = (nobs > 0) & (track <= nobs) & (pc != 2)
    cam_idx = []
    for c in range(C):
        f, pp, ex = ref.GROUPS[int(models[c])]
        idx = sorted((f if opts.refine_focal_length else []) + (pp if opts.refine_principal_point else [])
                     + (ex if opts.refine_extra_params else []))
        cam_idx.append(idx if cam_in[c] and not cam_const[c] else [])
    prob = ref.RigProblem(poses, pose_var, sc.xyz, point_var, cams, models, cam_idx, blk, xy,
                          loss=opts.loss_function_type, loss_scale=opts.loss_function_scale)
    prob.layout = dict(nsnap=nsnap, ncam=ncam, ident=ident)
    prob.obs = np.array(obs, int)[prob.keep]  # the problem observation of every reduced block
    return prob
