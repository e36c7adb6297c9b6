"""Independent checker for the reprojection residual of all nine camera
models (test helper, CPU, float64).

The oracle has no fisheye or FOV model, so the tests of those models compare
the product with this restatement instead:

  * the residual is the reference's (cost_functions.h): rotate the point by
    the quaternion as it is (no normalisation), add t, divide by z, apply the
    camera model, subtract the observation;
  * derivatives come from torch autograd, not from hand-derived formulas;
  * branches of a model are selected with masks over inputs made safe for the
    branch not taken, so an untaken branch never puts NaN into a gradient;
  * `reproj_eval` maps the ambient derivatives onto the product's tangent
    layout: rotation (J_q times the quaternion manifold's plus-Jacobian),
    translation, point, refined intrinsics in parameter order; columns of
    constant blocks are zero and a robust loss scales r and J by sqrt(rho').

test_fisheye_models.py first pins this helper to the oracle on the models the
oracle has.
"""
import numpy as np
import torch

SIMPLE_PINHOLE, PINHOLE, SIMPLE_RADIAL, RADIAL, OPENCV = range(5)
OPENCV_FISHEYE, FOV, SIMPLE_RADIAL_FISHEYE, RADIAL_FISHEYE = 5, 7, 8, 9
NUM_PARAMS = {0: 3, 1: 4, 2: 4, 3: 5, 4: 8, 5: 8, 7: 5, 8: 4, 9: 5}
# (focal idxs, principal point idxs, extra idxs)
GROUPS = {0: ([0], [1, 2], []), 1: ([0, 1], [2, 3], []), 2: ([0], [1, 2], [3]), 3: ([0], [1, 2], [3, 4]),
          4: ([0, 1], [2, 3], [4, 5, 6, 7]), 5: ([0, 1], [2, 3], [4, 5, 6, 7]), 7: ([0, 1], [2, 3], [4]),
          8: ([0], [1, 2], [3]), 9: ([0], [1, 2], [3, 4])}
EPS = float(np.finfo(np.float64).eps)
F64 = torch.float64


def _fisheye(u, v, ks):
    """Equidistant fisheye distortion offsets (du, dv); ks: list of [n] tensors."""
    r2 = u * u + v * v
    big = torch.sqrt(r2) > EPS
    r = torch.sqrt(torch.where(big, r2, torch.ones_like(r2)))
    theta = torch.atan(r)
    poly = torch.ones_like(theta)
    tp = theta * theta
    for k in ks:
        poly = poly + k * tp
        tp = tp * theta * theta
    thetad = theta * poly
    zero = torch.zeros_like(u)
    return torch.where(big, u * thetad / r - u, zero), torch.where(big, v * thetad / r - v, zero)


def _fov_factor(u, v, omega):
    r2 = u * u + v * v
    w2 = omega * omega
    m1 = w2 < 1e-4
    m2 = (~m1) & (r2 < 1e-4)
    m3 = (~m1) & (~m2)
    one = torch.ones_like(r2)
    f1 = (w2 * r2) / 3.0 - w2 / 12.0 + 1.0
    w_s = torch.where(m1, one, omega)
    th = torch.tan(w_s / 2.0)
    f2 = (-2.0 * th * (4.0 * r2 * th * th - 3.0)) / (3.0 * w_s)
    r_s = torch.sqrt(torch.where(m3, r2, one))
    f3 = torch.atan(r_s * 2.0 * th) / (r_s * w_s)
    return torch.where(m1, f1, torch.where(m2, f2, f3))


def project(model, prm, u, v):
    """World (normalized) -> image for [n] points; prm [n][num_params] tensor."""
    p = [prm[:, k] for k in range(prm.shape[1])]
    if model == SIMPLE_PINHOLE:
        return p[0] * u + p[1], p[0] * v + p[2]
    if model == PINHOLE:
        return p[0] * u + p[2], p[1] * v + p[3]
    if model in (SIMPLE_RADIAL, RADIAL):
        r2 = u * u + v * v
        radial = p[3] * r2 + (p[4] * r2 * r2 if model == RADIAL else 0.0)
        return p[0] * (u + u * radial) + p[1], p[0] * (v + v * radial) + p[2]
    if model == OPENCV:
        k1, k2, p1, p2 = p[4:8]
        u2, uv, v2 = u * u, u * v, v * v
        r2 = u2 + v2
        radial = k1 * r2 + k2 * r2 * r2
        du = u * radial + 2.0 * p1 * uv + p2 * (r2 + 2.0 * u2)
        dv = v * radial + 2.0 * p2 * uv + p1 * (r2 + 2.0 * v2)
        return p[0] * (u + du) + p[2], p[1] * (v + dv) + p[3]
    if model == OPENCV_FISHEYE:
        du, dv = _fisheye(u, v, p[4:8])
        return p[0] * (u + du) + p[2], p[1] * (v + dv) + p[3]
    if model == FOV:
        f = _fov_factor(u, v, p[4])
        return p[0] * (u * f) + p[2], p[1] * (v * f) + p[3]
    if model in (SIMPLE_RADIAL_FISHEYE, RADIAL_FISHEYE):
        du, dv = _fisheye(u, v, p[3:])
        return p[0] * (u + du) + p[1], p[0] * (v + dv) + p[2]
    raise ValueError(model)


def world_to_image(model, params, u, v):
    """numpy front end of `project`: params [num_params], u, v scalars or [n]."""
    u = torch.as_tensor(np.atleast_1d(np.asarray(u, np.float64)))
    v = torch.as_tensor(np.atleast_1d(np.asarray(v, np.float64)))
    prm = torch.as_tensor(np.asarray(params, np.float64)).expand(len(u), -1)
    x, y = project(model, prm, u, v)
    return x.numpy().copy(), y.numpy().copy()


def _rotate(q, X):
    """Rotation by the quaternion (w, x, y, z) as it is: X + 2 w (qv x X) + 2 qv x (qv x X)."""
    w, qv = q[:, :1], q[:, 1:]
    c1 = torch.cross(qv, X, dim=1)
    return X + 2.0 * (w * c1 + torch.cross(qv, c1, dim=1))


def _plus_jacobian(q):
    """d(q_delta * q)/d(delta) at delta = 0, q_delta = (1, delta) to first order: [n][4][3]."""
    n = q.shape[0]
    d = torch.zeros((n, 3), dtype=F64, requires_grad=True)
    w, qv = q[:, :1], q[:, 1:]
    out = torch.cat([w - (d * qv).sum(1, keepdim=True), qv + w * d + torch.cross(d, qv, dim=1)], dim=1)
    cols = [torch.autograd.grad(out[:, k].sum(), d, retain_graph=True)[0] for k in range(4)]
    return torch.stack(cols, dim=1)


def camera_of(sc):
    """Per-camera model ids and [C][8] zero-padded parameters of a Scene."""
    C = sc.num_cameras
    models = np.full(C, sc.camera_model, np.int64) if sc.camera_models is None else np.asarray(sc.camera_models, np.int64)
    off = sc.camera_param_offsets()
    flat = np.asarray(sc.camera_params, np.float64).reshape(-1)
    prm = np.zeros((C, 8))
    for c in range(C):
        prm[c, :off[c + 1] - off[c]] = flat[off[c]:off[c + 1]]
    return models, prm


def residuals(sc, with_jacobian=False):
    """Residual [N][2] of every observation of a Scene (quaternions as they
    are); with_jacobian: also the ambient derivatives by q [N][2][4],
    t [N][2][3], X [N][2][3], params [N][2][8], and the depth [N]."""
    models, prm_c = camera_of(sc)
    img = np.asarray(sc.obs_image, np.int64)
    cam = np.asarray(sc.image_camera, np.int64)[img]
    q = torch.tensor(np.asarray(sc.qvec, np.float64)[img], requires_grad=with_jacobian)
    t = torch.tensor(np.asarray(sc.tvec, np.float64)[img], requires_grad=with_jacobian)
    X = torch.tensor(np.asarray(sc.xyz, np.float64)[np.asarray(sc.obs_point, np.int64)], requires_grad=with_jacobian)
    prm = torch.tensor(prm_c[cam], requires_grad=with_jacobian)
    obs = torch.tensor(np.asarray(sc.obs_xy, np.float64).reshape(-1, 2))
    P = _rotate(q, X) + t
    u, v = P[:, 0] / P[:, 2], P[:, 1] / P[:, 2]
    x, y = torch.zeros_like(u), torch.zeros_like(u)
    mo = torch.as_tensor(models[cam])
    for m in np.unique(models[cam]):
        sel = torch.nonzero(mo == int(m))[:, 0]
        xm, ym = project(int(m), prm[sel][:, :NUM_PARAMS[int(m)]], u[sel], v[sel])
        x = x.index_add(0, sel, xm)
        y = y.index_add(0, sel, ym)
    r = torch.stack([x - obs[:, 0], y - obs[:, 1]], dim=1)
    if not with_jacobian:
        return r.detach().numpy()
    rows = [torch.autograd.grad(r[:, k].sum(), (q, t, X, prm), retain_graph=True) for k in range(2)]
    Jq, Jt, JX, Jp = (torch.stack([rows[0][a], rows[1][a]], dim=1) for a in range(4))
    Jrot = torch.einsum("nij,njk->nik", Jq, _plus_jacobian(q.detach()))
    return (r.detach().numpy(), Jrot.numpy(), Jt.numpy(), JX.numpy(), Jp.numpy(), P[:, 2].detach().numpy(),
            np.sqrt((u * u + v * v).detach().numpy()))


def loss_rho(opts, s):
    """rho(s) and rho'(s) of the options' loss (Trivial / SoftL1 / Cauchy)."""
    b = opts.loss_function_scale ** 2
    if opts.loss_function_type == 1:
        return 2.0 * b * (np.sqrt(1.0 + s / b) - 1.0), 1.0 / np.sqrt(1.0 + s / b)
    if opts.loss_function_type == 2:
        return b * np.log1p(s / b), 1.0 / (1.0 + s / b)
    return s, np.ones_like(s)


def tangent_indices(model, opts):
    f, pp, ex = GROUPS[int(model)]
    const = set()
    if not opts.refine_focal_length:
        const |= set(f)
    if not opts.refine_principal_point:
        const |= set(pp)
    if not opts.refine_extra_params:
        const |= set(ex)
    return [k for k in range(NUM_PARAMS[int(model)]) if k not in const]


def problem_flags(opts, sc):
    """Which blocks the problem holds and which parameter blocks vary
    (BundleAdjuster::SetUp: AddImageToProblem, AddPointToProblem,
    ParameterizeCameras, ParameterizePoints), restated."""
    I, C, Pn, N = sc.num_images, sc.num_cameras, sc.num_points, sc.num_obs
    models, _ = camera_of(sc)
    in_cfg = np.ones(I, bool) if sc.image_in_config is None else np.asarray(sc.image_in_config) != 0
    cpose = np.zeros(I, bool) if sc.image_constant_pose is None else np.asarray(sc.image_constant_pose) != 0
    if not opts.refine_extrinsics:
        cpose[:] = True
    tmask = np.zeros(I, np.int64) if sc.image_constant_tvec is None else np.asarray(sc.image_constant_tvec, np.int64)
    cam_const = np.zeros(C, bool) if sc.camera_constant is None else np.asarray(sc.camera_constant) != 0
    oi, op = np.asarray(sc.obs_image, np.int64), np.asarray(sc.obs_point, np.int64)
    in_problem = in_cfg[oi].copy()
    nobs_img = np.bincount(oi, minlength=I)
    img_var = in_cfg & (nobs_img > 0) & ~cpose
    cam_in = np.zeros(C, bool)
    cam_in[np.asarray(sc.image_camera)[in_cfg & (nobs_img > 0)]] = True
    pt_total = np.bincount(op, minlength=Pn)
    pt_nobs = np.bincount(op[in_problem], minlength=Pn)
    if sc.point_config is not None:
        pc = np.asarray(sc.point_config)
        for mode in (1, 2):
            for pt in np.nonzero(pc == mode)[0]:
                if pt_nobs[pt] == pt_total[pt]:
                    continue
                for k in np.nonzero((op == pt) & ~in_cfg[oi])[0]:
                    pt_nobs[pt] += 1
                    c = sc.image_camera[oi[k]]
                    if not cam_in[c]:
                        cam_in[c] = True
                        cam_const[c] = True
                    in_problem[k] = True
    ct = np.array([len(tangent_indices(m, opts)) for m in models])
    cam_var = cam_in & ~cam_const & (ct > 0)
    pt_var = (pt_nobs > 0) & ~(pt_total > pt_nobs)
    if sc.point_config is not None:
        pt_var &= np.asarray(sc.point_config) != 2
    return in_problem, img_var, np.where(img_var, tmask, 0), cam_var, pt_var, int(ct.max()) if C else 0


def normalized(sc):
    """A copy of the Scene with the quaternions of the images in the config
    normalised, as AddImageToProblem does before it adds their blocks."""
    out = sc.copy()
    in_cfg = np.ones(sc.num_images, bool) if sc.image_in_config is None else np.asarray(sc.image_in_config) != 0
    q = np.asarray(out.qvec, np.float64).copy()
    n = np.sqrt((q * q).sum(axis=1))
    unit = np.where(n[:, None] == 0, np.array([1.0, 0, 0, 0]), q / np.where(n == 0, 1.0, n)[:, None])
    out.qvec = np.where(in_cfg[:, None], unit, q)
    return out


def reproj_eval(opts, sc):
    """(r [N][2], J [N][2][9 + ct], in_problem [N], depth [N], radius [N]) in
    the product's tangent layout, one row pair per observation of the Scene."""
    sc = normalized(sc)
    r, Jrot, Jt, JX, Jp, depth, radius = residuals(sc, with_jacobian=True)
    in_problem, img_var, tmask, cam_var, pt_var, ct = problem_flags(opts, sc)
    models, _ = camera_of(sc)
    N = len(r)
    J = np.zeros((N, 2, 9 + ct))
    img = np.asarray(sc.obs_image, np.int64)
    cam = np.asarray(sc.image_camera, np.int64)[img]
    pt = np.asarray(sc.obs_point, np.int64)
    pv = img_var[img]
    J[:, :, 0:3] = np.where(pv[:, None, None], Jrot, 0.0)
    for b in range(3):
        J[:, :, 3 + b] = np.where((pv & (((tmask[img] >> b) & 1) == 0))[:, None], Jt[:, :, b], 0.0)
    J[:, :, 6:9] = np.where(pt_var[pt][:, None, None], JX, 0.0)
    for c in range(sc.num_cameras):
        if not cam_var[c]:
            continue
        sel = cam == c
        for slot, k in enumerate(tangent_indices(models[c], opts)):
            J[sel, :, 9 + slot] = Jp[sel, :, k]
    _, rho1 = loss_rho(opts, (r * r).sum(axis=1))
    sc_ = np.sqrt(rho1)
    return r * sc_[:, None], J * sc_[:, None, None], in_problem, depth, radius


def cost(opts, sc):
    """1/2 sum rho(|r|^2) over the problem's blocks."""
    sc = normalized(sc)
    r = residuals(sc)
    in_problem = problem_flags(opts, sc)[0]
    rho0, _ = loss_rho(opts, (r * r).sum(axis=1))
    return 0.5 * float(rho0[in_problem].sum())


def squared_reprojection_errors(sc):
    """CalculateSquaredReprojectionError per observation: the quaternion is
    normalised first; a point with depth below DBL_EPSILON gets DBL_MAX."""
    out = sc.copy()
    out.image_in_config = None
    out = normalized(out)
    r, _, _, _, _, depth, _ = residuals(out, with_jacobian=True)
    sq = (r * r).sum(axis=1)
    return np.where(depth < EPS, np.finfo(np.float64).max, sq)
