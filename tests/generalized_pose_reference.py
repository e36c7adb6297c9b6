"""An independent CPU reference for RefineGeneralizedAbsolutePose
(src/estimators/pose.cc:354-520), torch float64, sharing no code with the
product:

  * the residual is RigBundleAdjustmentCostFunction's (cost_functions.h:
    160-214): q = q_rel * q_rig, t = R(q_rel) t_rig + t_rel, rotate the point
    by q, add t, divide by z, apply the camera model (camera_model_ref.project,
    all nine models), subtract the observation;
  * Jacobians come from torch autograd in ambient coordinates, times the plus
    Jacobian of Ceres' QuaternionManifold; refined intrinsics are a subset;
  * CauchyLoss rho and rho'; the Corrector takes the rho'' <= 0 branch, so r
    and J are scaled by sqrt(rho');
  * the dense Levenberg-Marquardt of lm_reference (Ceres 2.1
    TrustRegionMinimizer semantics, the gradient, parameter and function
    tolerance stops, 5 consecutive invalid steps); it returns the (valid,
    successful, ended) trace.

quat_product and unit_quat_rotate are restated here over torch tensors (the
numpy ones of rig_reference cannot carry a gradient); test_generalized_pose
pins them to rig_reference's, whose quat_plus takes the steps.
"""
from dataclasses import dataclass, field

import numpy as np
import torch

import camera_model_ref as cm
import lm_reference as lm
import rig_reference as rr
from lm_reference import CONVERGENCE, FAILURE, NO_CONVERGENCE  # noqa: F401

F64 = torch.float64


def quat_product(z, w):
    """ceres::QuaternionProduct over tensors [..., 4]."""
    return torch.stack([z[..., 0] * w[..., 0] - z[..., 1] * w[..., 1] - z[..., 2] * w[..., 2] - z[..., 3] * w[..., 3],
                        z[..., 0] * w[..., 1] + z[..., 1] * w[..., 0] + z[..., 2] * w[..., 3] - z[..., 3] * w[..., 2],
                        z[..., 0] * w[..., 2] - z[..., 1] * w[..., 3] + z[..., 2] * w[..., 0] + z[..., 3] * w[..., 1],
                        z[..., 0] * w[..., 3] + z[..., 1] * w[..., 2] - z[..., 2] * w[..., 1] + z[..., 3] * w[..., 0]], -1)


def unit_quat_rotate(q, p):
    """ceres::UnitQuaternionRotatePoint over tensors."""
    t2, t3, t4 = q[..., 0] * q[..., 1], q[..., 0] * q[..., 2], q[..., 0] * q[..., 3]
    t5, t6, t7 = -q[..., 1] * q[..., 1], q[..., 1] * q[..., 2], q[..., 1] * q[..., 3]
    t8, t9, t1 = -q[..., 2] * q[..., 2], q[..., 2] * q[..., 3], -q[..., 3] * q[..., 3]
    return torch.stack([2 * ((t8 + t1) * p[..., 0] + (t6 - t4) * p[..., 1] + (t3 + t7) * p[..., 2]) + p[..., 0],
                        2 * ((t4 + t6) * p[..., 0] + (t5 + t1) * p[..., 1] + (t9 - t2) * p[..., 2]) + p[..., 1],
                        2 * ((t7 - t3) * p[..., 0] + (t2 + t9) * p[..., 1] + (t5 + t8) * p[..., 2]) + p[..., 2]], -1)


def plus_jacobian(q):
    """QuaternionManifold::PlusJacobian (4 x 3)."""
    return np.array([[-q[1], -q[2], -q[3]], [q[0], q[3], -q[2]], [-q[3], q[0], q[1]], [q[2], -q[1], q[0]]])


def refined_indices(model, refine_focal_length, refine_extra_params):
    """Focal length and extra parameter indices, the principal point never."""
    f, _, e = cm.GROUPS[model]
    return sorted((list(f) if refine_focal_length else []) + (list(e) if refine_extra_params else []))


@dataclass
class Result:
    qvec: np.ndarray
    tvec: np.ndarray
    camera_params: list
    initial_cost: float
    final_cost: float
    num_successful_steps: int
    num_unsuccessful_steps: int
    termination_type: int
    trace: list = field(default_factory=list)  # (valid, successful, ended) per iteration
    num_residuals: int = 0
    num_effective_parameters: int = 0


class Problem:
    """The reduced program of one RefineGeneralizedAbsolutePose call."""

    def __init__(self, camera_models, camera_params, rig_qvecs, rig_tvecs, qvec, tvec, points2D, points3D,
                 camera_idxs, inlier_mask=None, refine_focal_length=True, refine_extra_params=True,
                 loss_function_scale=1.0):
        keep = np.ones(len(points2D), bool) if inlier_mask is None else np.asarray(inlier_mask) != 0
        self.xy = np.asarray(points2D, np.float64).reshape(-1, 2)[keep]
        self.X = np.asarray(points3D, np.float64).reshape(-1, 3)[keep]
        self.cidx = np.asarray(camera_idxs).reshape(-1)[keep]
        self.models = list(camera_models)
        self.cams = [np.array(c, np.float64) for c in camera_params]
        self.rq = np.asarray(rig_qvecs, np.float64).reshape(-1, 4)
        self.rt = np.asarray(rig_tvecs, np.float64).reshape(-1, 3)
        self.q = np.array(qvec, np.float64)
        self.t = np.array(tvec, np.float64)
        self.b = float(loss_function_scale) ** 2
        # cameras with inliers, in camera order; their refined sets and tangent offsets
        self.used = [c for c in range(len(self.models)) if np.any(self.cidx == c)]
        self.rows = {c: np.flatnonzero(self.cidx == c) for c in self.used}
        self.idx, self.off = {}, {}
        n = 6
        for c in self.used:
            self.idx[c] = refined_indices(self.models[c], refine_focal_length, refine_extra_params)
            self.off[c] = n
            n += len(self.idx[c])
        self.n = n

    # residuals [N][2] and, with jac, the ambient derivatives per observation
    def _camera_block(self, c, q, t, prm, jac):
        rows = self.rows[c]
        m = len(rows)
        Q = torch.as_tensor(q).expand(m, 4).clone().requires_grad_(jac)
        T = torch.as_tensor(t).expand(m, 3).clone().requires_grad_(jac)
        P = torch.as_tensor(prm).expand(m, -1).clone().requires_grad_(jac)
        rel_q = torch.as_tensor(self.rq[c]).expand(m, 4)
        rel_t = torch.as_tensor(self.rt[c]).expand(m, 3)
        X = torch.as_tensor(self.X[rows])
        pc = unit_quat_rotate(quat_product(rel_q, Q), X) + unit_quat_rotate(rel_q, T) + rel_t
        x, y = cm.project(self.models[c], P, pc[:, 0] / pc[:, 2], pc[:, 1] / pc[:, 2])
        r = torch.stack([x - torch.as_tensor(self.xy[rows, 0]), y - torch.as_tensor(self.xy[rows, 1])], -1)
        if not jac:
            return r.detach().numpy(), None
        g = []
        for k in range(2):
            gq, gt, gp = torch.autograd.grad(r[:, k].sum(), [Q, T, P], retain_graph=k == 0, allow_unused=True)
            gp = torch.zeros_like(P) if gp is None else gp
            g.append((gq.numpy(), gt.numpy(), gp.numpy()))
        return r.detach().numpy(), g

    def rho(self, s):
        return self.b * np.log1p(s / self.b), 1.0 / (1.0 + s / self.b)

    def cost(self, q=None, t=None, cams=None):
        q = self.q if q is None else q
        t = self.t if t is None else t
        cams = self.cams if cams is None else cams
        total = 0.0
        for c in self.used:
            r, _ = self._camera_block(c, q, t, cams[c], False)
            total += 0.5 * self.rho((r * r).sum(1))[0].sum()
        return total

    def jacobian(self):
        """Loss-corrected residual vector and tangent Jacobian (rows grouped by
        camera) and the cost at the current point."""
        N = len(self.xy)
        r_all, J = np.zeros(2 * N), np.zeros((2 * N, self.n))
        PJ = plus_jacobian(self.q)
        at, cost = 0, 0.0
        for c in self.used:
            r, g = self._camera_block(c, self.q, self.t, self.cams[c], True)
            rho, rho1 = self.rho((r * r).sum(1))
            cost += 0.5 * rho.sum()
            sq = np.sqrt(rho1)
            m = len(r)
            for k in range(2):
                rows = at + 2 * np.arange(m) + k
                gq, gt, gp = g[k]
                r_all[rows] = sq * r[:, k]
                J[rows, 0:3] = sq[:, None] * (gq @ PJ)
                J[rows, 3:6] = sq[:, None] * gt
                for j, i in enumerate(self.idx[c]):
                    J[rows, self.off[c] + j] = sq * gp[:, i]
            at += 2 * m
        return r_all, J, cost

    def plus(self, delta):
        q = rr.quat_plus(self.q, delta[0:3])
        t = self.t + delta[3:6]
        cams = [c.copy() for c in self.cams]
        for c in self.used:
            for j, i in enumerate(self.idx[c]):
                cams[c][i] += delta[self.off[c] + j]
        return q, t, cams

    def ambient(self, q=None, t=None, cams=None):
        q = self.q if q is None else q
        t = self.t if t is None else t
        cams = self.cams if cams is None else cams
        return np.concatenate([q, t] + [cams[c] for c in self.used if self.idx[c]])

    def accept(self, q, t, cams):
        self.q, self.t, self.cams = q, t, cams

    def solve(self, gradient_tolerance=1.0, max_num_iterations=100, function_tolerance=1e-6,
              parameter_tolerance=1e-8, **kw):
        """lm_reference.minimize with RefineAbsolutePose's defaults."""
        N = len(self.xy)

        def result(s):
            return Result(self.q.copy(), self.t.copy(), [c.copy() for c in self.cams], *s, 2 * N, self.n if N else 0)

        if N == 0:
            return result(lm.Solve(0.0, 0.0, 0, 0, CONVERGENCE, []))
        s = lm.minimize(self, gradient_tolerance, max_num_iterations, function_tolerance, parameter_tolerance, **kw)
        if s.termination_type == FAILURE and s.trace:  # after iterations; a non-finite initial cost is reported
            raise AssertionError("the reference does not restore parameters after FAILURE: unexpected here")
        return result(s)

    def covariance(self):
        """inv(J'J)[:6, :6] of the loss-corrected Jacobian at the current point."""
        _, J, _ = self.jacobian()
        return np.linalg.inv(J.T @ J)[:6, :6]
