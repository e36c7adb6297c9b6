"""An independent CPU reference for RefineRelativePose
(src/estimators/pose.cc:324-352), torch float64, sharing no code with the
product:

  * the residual is RelativePoseCostFunction's (cost_functions.h:216-268):
    R = ceres::QuaternionToRotation(q), E = [t]x R, a = E x1h, b = E' x2h,
    s = x2h . a, r = s^2 / (a0^2 + a1^2 + b0^2 + b1^2).  r is already the
    squared Sampson error and Ceres squares it again: cost = 0.5 sum rho(r^2);
  * Jacobians come from torch autograd in ambient coordinates (4 + 3), times
    the plus Jacobians of Ceres 2.1's QuaternionManifold (4 x 3) and
    SphereManifold<3> (3 x 2), both restated here;
  * CauchyLoss rho and rho'; the Corrector takes the rho'' <= 0 branch, so r
    and J are scaled by sqrt(rho');
  * the dense Levenberg-Marquardt of lm_reference (Ceres 2.1
    TrustRegionMinimizer semantics, the gradient, parameter and function
    tolerance stops, 5 consecutive invalid steps); it returns the (valid,
    successful, ended) trace.

The quaternion Plus is rig_reference.quat_plus, as in
generalized_pose_reference."""
from dataclasses import dataclass, field

import numpy as np
import torch

import lm_reference as lm
import rig_reference as rr
from lm_reference import CONVERGENCE, FAILURE, NO_CONVERGENCE  # noqa: F401

EPS = np.finfo(np.float64).eps


def quat_to_rotation(q):
    """ceres::QuaternionToRotation over tensors [..., 4] -> [..., 3, 3]: the
    scaled rotation divided by q.q (no normalisation of q itself)."""
    a, b, c, d = q[..., 0], q[..., 1], q[..., 2], q[..., 3]
    aa, ab, ac, ad, bb, bc, bd, cc, cd, dd = a * a, a * b, a * c, a * d, b * b, b * c, b * d, c * c, c * d, d * d
    n = aa + bb + cc + dd
    rows = [[aa + bb - cc - dd, 2 * (bc - ad), 2 * (ac + bd)],
            [2 * (ad + bc), aa - bb + cc - dd, 2 * (cd - ab)],
            [2 * (bd - ac), 2 * (ab + cd), aa - bb - cc + dd]]
    return torch.stack([torch.stack(r, -1) for r in rows], -2) / n[..., None, None]


def residuals(q, t, x1, x2):
    """r [N] over tensors q [N][4], t [N][3], x1, x2 [N][2]."""
    R = quat_to_rotation(q)
    z = torch.zeros_like(t[..., 0])
    tx = torch.stack([torch.stack([z, -t[..., 2], t[..., 1]], -1), torch.stack([t[..., 2], z, -t[..., 0]], -1),
                      torch.stack([-t[..., 1], t[..., 0], z], -1)], -2)
    E = tx @ R
    one = torch.ones_like(x1[..., :1])
    h1, h2 = torch.cat([x1, one], -1), torch.cat([x2, one], -1)
    a = (E @ h1[..., None])[..., 0]
    b = (E.transpose(-1, -2) @ h2[..., None])[..., 0]
    s = (h2 * a).sum(-1)
    return s * s / (a[..., 0] ** 2 + a[..., 1] ** 2 + b[..., 0] ** 2 + b[..., 1] ** 2)


def quat_plus_jacobian(q):
    """QuaternionManifold::PlusJacobian (4 x 3)."""
    return np.array([[-q[1], -q[2], -q[3]], [q[0], q[3], -q[2]], [-q[3], q[0], q[1]], [q[2], -q[1], q[0]]])


def householder(x):
    """(v, beta) of SphereManifold<3> at x: H = I - beta v v', H x = |x| e3."""
    sigma = x[0] * x[0] + x[1] * x[1]
    v = np.array([x[0], x[1], 1.0])
    beta = 0.0
    if sigma <= EPS:
        if x[2] < 0:
            beta = 2.0
    else:
        mu = np.sqrt(x[2] * x[2] + sigma)
        vp = x[2] - mu if x[2] <= 0 else -sigma / (x[2] + mu)
        beta = 2.0 * vp * vp / (sigma + vp * vp)
        v[:2] /= vp
    return v, beta


def sphere_plus(x, d):
    """SphereManifold<3>::Plus (no factor 1/2)."""
    x = np.asarray(x, np.float64)
    n = np.hypot(d[0], d[1])
    if n == 0:
        return x.copy()
    v, beta = householder(x)
    y = np.array([np.sin(n) / n * d[0], np.sin(n) / n * d[1], np.cos(n)])
    return np.linalg.norm(x) * (y - beta * v * (v @ y))


def sphere_plus_jacobian(x):
    """SphereManifold<3>::PlusJacobian (3 x 2)."""
    x = np.asarray(x, np.float64)
    v, beta = householder(x)
    return np.linalg.norm(x) * (np.eye(3)[:, :2] - beta * np.outer(v, v[:2]))


@dataclass
class Result:
    qvec: np.ndarray
    tvec: np.ndarray
    initial_cost: float
    final_cost: float
    num_successful_steps: int
    num_unsuccessful_steps: int
    termination_type: int
    trace: list = field(default_factory=list)  # (valid, successful, ended) per iteration
    num_residuals: int = 0
    num_effective_parameters: int = 0


class Problem:
    """The program of one RefineRelativePose call."""

    def __init__(self, qvec, tvec, points1, points2, inlier_mask=None, loss_function_scale=1.0, normalize=True):
        keep = np.ones(len(points1), bool) if inlier_mask is None else np.asarray(inlier_mask) != 0
        self.x1 = np.asarray(points1, np.float64).reshape(-1, 2)[keep]
        self.x2 = np.asarray(points2, np.float64).reshape(-1, 2)[keep]
        self.q = np.array(qvec, np.float64)
        if normalize:  # NormalizeQuaternion (pose.cc:331)
            n = np.linalg.norm(self.q)
            self.q = np.array([1.0, 0, 0, 0]) if n == 0 else self.q / n
        self.t = np.array(tvec, np.float64)
        self.b = float(loss_function_scale) ** 2

    def _eval(self, q, t, jac):
        m = len(self.x1)
        Q = torch.as_tensor(q).expand(m, 4).clone().requires_grad_(jac)
        T = torch.as_tensor(t).expand(m, 3).clone().requires_grad_(jac)
        r = residuals(Q, T, torch.as_tensor(self.x1), torch.as_tensor(self.x2))
        if not jac:
            return r.detach().numpy(), None
        gq, gt = torch.autograd.grad(r.sum(), [Q, T])
        return r.detach().numpy(), (gq.numpy(), gt.numpy())

    def evaluate(self):
        """Residuals [N] and tangent Jacobians [N][5], not loss-corrected."""
        r, (gq, gt) = self._eval(self.q, self.t, True)
        return r, np.concatenate([gq @ quat_plus_jacobian(self.q), gt @ sphere_plus_jacobian(self.t)], 1)

    def rho(self, s):
        """ceres::CauchyLoss::Evaluate as written (loss_function.cc): sum = 1 +
        s * c with c = 1 / b, rho = b * log(sum), rho' = 1 / sum.  It is log,
        not log1p: for the tiny s = r^2 of this problem 1 + s rounds to a
        multiple of 2.2e-16, and that rounding is part of what Ceres computes."""
        total = 1.0 + s * (1.0 / self.b)
        return self.b * np.log(total), 1.0 / total

    def cost(self, q=None, t=None):
        r, _ = self._eval(self.q if q is None else q, self.t if t is None else t, False)
        return 0.5 * self.rho(r * r)[0].sum()

    def jacobian(self):
        """Loss-corrected residual vector, tangent Jacobian and the cost."""
        r, J = self.evaluate()
        rho, rho1 = self.rho(r * r)
        sq = np.sqrt(rho1)
        return sq * r, sq[:, None] * J, 0.5 * rho.sum()

    def plus(self, delta):
        return rr.quat_plus(self.q, delta[0:3]), sphere_plus(self.t, delta[3:5])

    def ambient(self, q=None, t=None):
        return np.concatenate([self.q if q is None else q, self.t if t is None else t])

    def accept(self, q, t):
        self.q, self.t = q, t

    def solve(self, max_num_iterations=50, function_tolerance=1e-6, gradient_tolerance=1e-10,
              parameter_tolerance=1e-8, **kw):
        """lm_reference.minimize with ceres::Solver::Options' defaults."""
        N = len(self.x1)

        def result(s):
            return Result(self.q.copy(), self.t.copy(), *s, N, 5 if N else 0)

        if N == 0:
            return result(lm.Solve(0.0, 0.0, 0, 0, CONVERGENCE, []))
        q0, t0 = self.q.copy(), self.t.copy()
        with np.errstate(all="ignore"):  # an evaluation may overflow on the way to a rejected step
            s = lm.minimize(self, gradient_tolerance, max_num_iterations, function_tolerance, parameter_tolerance, **kw)
        if s.termination_type == FAILURE:  # Ceres leaves the parameter blocks as they were given
            self.q, self.t = q0, t0
        return result(s)


def essential_matrix(q, t):
    """EssentialMatrixFromPose: [t / |t|]x R(q) (essential_matrix.cc:90-93)."""
    q = np.asarray(q, np.float64) / np.linalg.norm(q)
    t = np.asarray(t, np.float64) / np.linalg.norm(t)
    R = quat_to_rotation(torch.as_tensor(q)).numpy()
    tx = np.array([[0, -t[2], t[1]], [t[2], 0, -t[0]], [-t[1], t[0], 0]])
    return tx @ R
