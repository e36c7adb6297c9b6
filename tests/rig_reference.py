"""An independent CPU reference for rig bundle adjustment (numpy, small
problems only), written from the reference's sources and sharing no code
with the product:

  * RigBundleAdjustmentCostFunction (src/base/cost_functions.h:160-214)
    restated literally over its six parameter blocks; its Jacobian by
    complex-step differentiation along Ceres' manifolds (every operation of
    the functor and of SIMPLE_RADIAL / OPENCV is analytic, so the derivative
    is exact to rounding, like a Jet's);
  * the set-up rules of RigBundleAdjuster::SetUp / AddImageToProblem /
    AddPointToProblem (src/optim/bundle_adjustment.cc:871-1140) and Ceres'
    reduced-program rule;
  * a dense Levenberg-Marquardt with Ceres 2.1's TrustRegionMinimizer /
    LevenbergMarquardtStrategy semantics over the full tangent Jacobian (no
    Schur complement, no projection matrix T), solved by dense Cholesky,
    returning the per-iteration trace (valid, successful, cost, model cost
    change, relative decrease).

An image of no rig is a rig pose with a constant identity relative pose (the
concatenation with (1, 0, 0, 0), (0, 0, 0) is exact in floating point), an
image outside the config a constant one.
"""
import numpy as np

SIMPLE_RADIAL, OPENCV = 2, 4
NUM_PARAMS = {SIMPLE_RADIAL: 4, OPENCV: 8}
# focal length / principal point / extra parameter indices (camera_models.h)
GROUPS = {SIMPLE_RADIAL: ([0], [1, 2], [3]), OPENCV: ([0, 1], [2, 3], [4, 5, 6, 7])}


# --- the cost function -----------------------------------------------------
def quat_product(z, w):
    """ceres::QuaternionProduct, arrays [..., 4]."""
    return np.stack([z[..., 0] * w[..., 0] - z[..., 1] * w[..., 1] - z[..., 2] * w[..., 2] - z[..., 3] * w[..., 3],
                     z[..., 0] * w[..., 1] + z[..., 1] * w[..., 0] + z[..., 2] * w[..., 3] - z[..., 3] * w[..., 2],
                     z[..., 0] * w[..., 2] - z[..., 1] * w[..., 3] + z[..., 2] * w[..., 0] + z[..., 3] * w[..., 1],
                     z[..., 0] * w[..., 3] + z[..., 1] * w[..., 2] - z[..., 2] * w[..., 1] + z[..., 3] * w[..., 0]], -1)


def unit_quat_rotate(q, p):
    """ceres::UnitQuaternionRotatePoint."""
    t2, t3, t4 = q[..., 0] * q[..., 1], q[..., 0] * q[..., 2], q[..., 0] * q[..., 3]
    t5, t6, t7 = -q[..., 1] * q[..., 1], q[..., 1] * q[..., 2], q[..., 1] * q[..., 3]
    t8, t9, t1 = -q[..., 2] * q[..., 2], q[..., 2] * q[..., 3], -q[..., 3] * q[..., 3]
    return np.stack([2 * ((t8 + t1) * p[..., 0] + (t6 - t4) * p[..., 1] + (t3 + t7) * p[..., 2]) + p[..., 0],
                     2 * ((t4 + t6) * p[..., 0] + (t5 + t1) * p[..., 1] + (t9 - t2) * p[..., 2]) + p[..., 1],
                     2 * ((t7 - t3) * p[..., 0] + (t2 + t9) * p[..., 1] + (t5 + t8) * p[..., 2]) + p[..., 2]], -1)


def world_to_image(model, prm, u, v):
    """SimpleRadialCameraModel / OpenCVCameraModel::WorldToImage; model [n], prm [n, 8]."""
    sr = model == SIMPLE_RADIAL
    r2 = u * u + v * v
    # SIMPLE_RADIAL
    rad = prm[:, 3] * r2
    xs = prm[:, 0] * (u + u * rad) + prm[:, 1]
    ys = prm[:, 0] * (v + v * rad) + prm[:, 2]
    # OPENCV
    k1, k2, p1, p2 = prm[:, 4], prm[:, 5], prm[:, 6], prm[:, 7]
    uv = u * v
    radial = k1 * r2 + k2 * r2 * r2
    du = u * radial + 2 * p1 * uv + p2 * (r2 + 2 * u * u)
    dv = v * radial + 2 * p2 * uv + p1 * (r2 + 2 * v * v)
    xo = prm[:, 0] * (u + du) + prm[:, 2]
    yo = prm[:, 1] * (v + dv) + prm[:, 3]
    return np.where(sr, xs, xo), np.where(sr, ys, yo)


def rig_residual(model, rig_q, rig_t, rel_q, rel_t, X, prm, xy):
    """RigBundleAdjustmentCostFunction::operator(), one row per block."""
    q = quat_product(rel_q, rig_q)
    t = unit_quat_rotate(rel_q, rig_t) + rel_t
    P = unit_quat_rotate(q, X) + t
    x, y = world_to_image(model, prm, P[:, 0] / P[:, 2], P[:, 1] / P[:, 2])
    return np.stack([x - xy[:, 0], y - xy[:, 1]], -1)


def quat_plus(x, d):
    """ceres::QuaternionManifold::Plus, arrays; complex deltas allowed."""
    nd = np.sqrt((d * d).sum(-1))
    safe = np.where(nd == 0, 1.0, nd)
    s = np.where(nd == 0, 1.0, np.sin(safe) / safe)
    a = np.concatenate([np.cos(nd)[..., None], s[..., None] * d], -1)
    return quat_product(a, x)


# --- the problem -------------------------------------------------------------
class RigProblem:
    """poses [n][7] (q, t): every rig pose, relative pose and free image pose
    in one table; pose_var [n].  Blocks: (rig pose, relative pose, point,
    camera, observation).  cam_idx: refined parameter indices per camera
    (empty: constant).  Parameters are updated in place by solve()."""

    def __init__(self, poses, pose_var, points, point_var, cams, cam_model, cam_idx, blk, xy,
                 loss=0, loss_scale=1.0):
        self.poses = np.array(poses, float)
        self.pose_var = np.asarray(pose_var, bool)
        self.points = np.array(points, float)
        self.point_var = np.asarray(point_var, bool)
        self.cams = np.array(cams, float)  # [C, 8] padded
        self.cam_model = np.asarray(cam_model)
        self.cam_idx = [list(i) for i in cam_idx]
        blk = np.asarray(blk, int).reshape(-1, 4)
        xy = np.asarray(xy, float).reshape(-1, 2)
        # Ceres' reduced program: blocks with no variable parameter block are dropped
        keep = np.array([self.pose_var[b[0]] or self.pose_var[b[1]] or self.point_var[b[2]]
                         or len(self.cam_idx[b[3]]) > 0 for b in blk], bool)
        self.keep = keep
        self.fixed_blk, self.fixed_xy = blk[~keep], xy[~keep]
        self.blk, self.xy = blk[keep], xy[keep]
        self.loss, self.loss_scale = loss, loss_scale
        # tangent layout over the parameter blocks used by the reduced program
        used_pose = np.zeros(len(self.poses), bool)
        used_pose[self.blk[:, 0]] = True
        used_pose[self.blk[:, 1]] = True
        used_pt = np.zeros(len(self.points), bool)
        used_pt[self.blk[:, 2]] = True
        used_cam = np.zeros(len(self.cams), bool)
        used_cam[self.blk[:, 3]] = True
        self.pose_off = np.full(len(self.poses), -1)
        n = 0
        for k in range(len(self.poses)):
            if self.pose_var[k] and used_pose[k]:
                self.pose_off[k] = n
                n += 6
        self.cam_off = np.full(len(self.cams), -1)
        for c in range(len(self.cams)):
            if self.cam_idx[c] and used_cam[c]:
                self.cam_off[c] = n
                n += len(self.cam_idx[c])
        self.pt_off = np.full(len(self.points), -1)
        for k in range(len(self.points)):
            if self.point_var[k] and used_pt[k]:
                self.pt_off[k] = n
                n += 3
        self.n = n
        self.num_residuals_reduced = 2 * len(self.blk)
        self.num_effective_parameters_reduced = n

    # -- evaluation ------------------------------------------------------
    def _gather(self, blk, poses, points, cams):
        return (self.cam_model[blk[:, 3]], poses[blk[:, 0], :4], poses[blk[:, 0], 4:], poses[blk[:, 1], :4],
                poses[blk[:, 1], 4:], points[blk[:, 2]], cams[blk[:, 3]])

    def residuals(self, poses=None, points=None, cams=None, blk=None, xy=None):
        poses = self.poses if poses is None else poses
        points = self.points if points is None else points
        cams = self.cams if cams is None else cams
        blk = self.blk if blk is None else blk
        xy = self.xy if xy is None else xy
        if len(blk) == 0:
            return np.zeros((0, 2))
        return rig_residual(*self._gather(blk, poses, points, cams), xy)

    def rho(self, s):
        """(rho, rho') of TrivialLoss / SoftLOneLoss(scale)."""
        if self.loss == 0:
            return s, np.ones_like(s)
        b = self.loss_scale * self.loss_scale
        tmp = np.sqrt(1 + s / b)
        return 2 * b * (tmp - 1), 1 / tmp

    def cost(self, poses=None, points=None, cams=None):
        r = self.residuals(poses, points, cams)
        return 0.5 * self.rho((r * r).sum(-1))[0].sum()

    def fixed_cost(self):
        r = self.residuals(blk=self.fixed_blk, xy=self.fixed_xy)
        return 0.5 * self.rho((r * r).sum(-1))[0].sum()

    def block_jacobians(self, h=1e-30):
        """Per block: residual [nb, 2] and the 2 x (6 + 6 + 3 + 8) tangent
        Jacobian w.r.t. rig pose, relative pose, point, camera parameters
        (ambient for point and camera), uncorrected, by complex step."""
        m, rq, rt, lq, lt, X, prm = self._gather(self.blk, self.poses, self.points, self.cams)
        base = [rq, rt, lq, lt, X, prm]
        r0 = rig_residual(m, *base, self.xy)
        J = np.zeros((len(self.blk), 2, 23))
        col = 0
        for which, dim in ((0, 3), (1, 3), (2, 3), (3, 3), (4, 3), (5, 8)):
            for k in range(dim):
                args = [a.astype(complex) for a in base]
                d = np.zeros(args[which].shape[:1] + (dim,), complex)
                d[:, k] = 1j * h
                args[which] = quat_plus(args[which], d) if which in (0, 2) else args[which] + d
                J[:, :, col] = rig_residual(m, *args, self.xy).imag / h
                col += 1
        return r0, J

    def jacobian(self):
        """Corrected residual vector and the dense tangent Jacobian of the reduced program."""
        r, Jb = self.block_jacobians()
        _, rho1 = self.rho((r * r).sum(-1))
        sq = np.sqrt(rho1)  # Corrector with rho'' <= 0: residual and Jacobian scaled by sqrt(rho')
        nb = len(self.blk)
        J = np.zeros((2 * nb, self.n))
        for b in range(nb):
            ip, il, ipt, ic = self.blk[b]
            rows = slice(2 * b, 2 * b + 2)
            if self.pose_off[ip] >= 0:
                J[rows, self.pose_off[ip]:self.pose_off[ip] + 6] = sq[b] * Jb[b, :, 0:6]
            if self.pose_off[il] >= 0:
                J[rows, self.pose_off[il]:self.pose_off[il] + 6] = sq[b] * Jb[b, :, 6:12]
            if self.pt_off[ipt] >= 0:
                J[rows, self.pt_off[ipt]:self.pt_off[ipt] + 3] = sq[b] * Jb[b, :, 12:15]
            if self.cam_off[ic] >= 0:
                idx = self.cam_idx[ic]
                J[rows, self.cam_off[ic]:self.cam_off[ic] + len(idx)] = sq[b] * Jb[b][:, [15 + k for k in idx]]
        return (sq[:, None] * r).reshape(-1), J

    def plus(self, delta):
        poses, points, cams = self.poses.copy(), self.points.copy(), self.cams.copy()
        for k in np.flatnonzero(self.pose_off >= 0):
            o = self.pose_off[k]
            poses[k, :4] = quat_plus(poses[k, :4], delta[o:o + 3])
            poses[k, 4:] = poses[k, 4:] + delta[o + 3:o + 6]
        for c in np.flatnonzero(self.cam_off >= 0):
            o = self.cam_off[c]
            for j, idx in enumerate(self.cam_idx[c]):
                cams[c, idx] += delta[o + j]
        for k in np.flatnonzero(self.pt_off >= 0):
            o = self.pt_off[k]
            points[k] = points[k] + delta[o:o + 3]
        return poses, points, cams

    # -- Ceres 2.1 TrustRegionMinimizer + LevenbergMarquardtStrategy -----------
    def solve(self, max_num_iterations=100, initial_trust_region_radius=1e4, min_relative_decrease=1e-3,
              max_num_consecutive_invalid_steps=10):
        fixed = self.fixed_cost()
        x_cost = self.cost()
        trace = []
        out = dict(initial_cost=x_cost + fixed, num_successful_steps=0, num_unsuccessful_steps=0)
        radius, decrease_factor = initial_trust_region_radius, 2.0
        r, J = self.jacobian()
        scale = 1.0 / (1.0 + np.sqrt((J * J).sum(0)))  # Jacobi scaling, fixed at iteration 0
        reuse_diag, invalid, iteration, diag = False, 0, 0, None
        while iteration < max_num_iterations and radius > 1e-32:
            iteration += 1
            Js = J * scale
            if not reuse_diag:
                diag = np.clip((Js * Js).sum(0), 1e-6, 1e32)
            reuse_diag = True
            A = Js.T @ Js + np.diag(diag / radius)
            ok = True
            try:
                L = np.linalg.cholesky(A)
                y = np.linalg.solve(L.T, np.linalg.solve(L, -(Js.T @ r)))
            except np.linalg.LinAlgError:
                ok = False
            model_change = 0.0
            if ok:
                delta = y * scale
                mr = J @ delta
                model_change = -mr @ (r + mr / 2)
                ok = np.isfinite(model_change) and model_change > 0
            if not ok:
                trace.append((0, 0, x_cost + fixed, 0.0, 0.0))
                invalid += 1
                out["num_unsuccessful_steps"] += 1
                if invalid > max_num_consecutive_invalid_steps:
                    break
                radius /= decrease_factor
                decrease_factor *= 2
                continue
            invalid = 0
            cand = self.plus(delta)
            cand_cost = self.cost(*cand)
            rel = (x_cost - cand_cost) / model_change
            if np.isfinite(cand_cost) and rel > min_relative_decrease:
                out["num_successful_steps"] += 1
                x_cost = cand_cost
                self.poses, self.points, self.cams = cand
                radius = min(1e16, radius / max(1.0 / 3.0, 1.0 - (2.0 * rel - 1.0) ** 3))
                decrease_factor = 2.0
                reuse_diag = False
                r, J = self.jacobian()
                trace.append((1, 1, x_cost + fixed, model_change, rel))
            else:
                out["num_unsuccessful_steps"] += 1
                radius /= decrease_factor
                decrease_factor *= 2
                trace.append((1, 0, x_cost + fixed, model_change, rel))
        out["final_cost"] = x_cost + fixed
        out["trace"] = trace
        return out
