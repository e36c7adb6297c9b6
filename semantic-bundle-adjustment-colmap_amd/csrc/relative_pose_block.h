// relative_pose_block.h — host/device math of the two-view refinement
// (RefineRelativePose, src/estimators/pose.cc:324-352): the residual of
// RelativePoseCostFunction (src/base/cost_functions.h:216-268), its analytic
// tangent Jacobian, and Ceres 2.1's SphereManifold<3> restated.  Included by
// relative_pose.hip and, compiled for the host, by
// tests/cpp/relative_pose_block_test.cc.
//
// The residual is the *squared* Sampson error r = s^2 / d (the reference
// returns it as the residual, and Ceres squares it once more: the cost is
// 0.5 sum rho(r^2)).  That is restated, not repaired.
//
// Tangent: rotation 3 (QuaternionManifold, q+ = exp(delta) * q with the
// half-angle delta, so R+ = (I + 2 [delta]x) R to first order: the rotation of
// ceres::QuaternionToRotation does not depend on |q|), translation 2
// (SphereManifold<3>).
#pragma once

#include "ba_math.h"

namespace miba {

constexpr double kSphereEpsilon = 2.220446049250313e-16;  // DBL_EPSILON

// ceres::QuaternionToRotation: the scaled rotation divided by q.q (row-major).
MI_HD void quat_to_rotation(const double q[4], double R[9]) {
  const double a = q[0], b = q[1], c = q[2], d = q[3];
  const double aa = a * a, ab = a * b, ac = a * c, ad = a * d, bb = b * b, bc = b * c, bd = b * d, cc = c * c,
               cd = c * d, dd = d * d;
  const double inv = 1.0 / (aa + bb + cc + dd);
  R[0] = (aa + bb - cc - dd) * inv; R[1] = 2.0 * (bc - ad) * inv;     R[2] = 2.0 * (ac + bd) * inv;
  R[3] = 2.0 * (ad + bc) * inv;     R[4] = (aa - bb + cc - dd) * inv; R[5] = 2.0 * (cd - ab) * inv;
  R[6] = 2.0 * (bd - ac) * inv;     R[7] = 2.0 * (ab + cd) * inv;     R[8] = (aa - bb - cc + dd) * inv;
}

// The Householder vector of SphereManifold<3> at x: H = I - beta v v', H x = |x| e3.
MI_HD void sphere_householder(const double x[3], double v[3], double* beta) {
  const double sigma = x[0] * x[0] + x[1] * x[1];
  v[0] = x[0];
  v[1] = x[1];
  v[2] = 1.0;
  *beta = 0.0;
  if (sigma <= kSphereEpsilon) {
    if (x[2] < 0.0) *beta = 2.0;
  } else {
    const double mu = sqrt(x[2] * x[2] + sigma);
    const double vp = x[2] <= 0.0 ? x[2] - mu : -sigma / (x[2] + mu);
    *beta = 2.0 * vp * vp / (sigma + vp * vp);
    v[0] /= vp;
    v[1] /= vp;
  }
}

// SphereManifold<3>::Plus: |out| = |x|.
MI_HD void sphere_plus(const double x[3], const double d[2], double out[3]) {
  const double n = sqrt(d[0] * d[0] + d[1] * d[1]);
  if (n == 0.0) {
    out[0] = x[0]; out[1] = x[1]; out[2] = x[2];
    return;
  }
  double v[3], beta;
  sphere_householder(x, v, &beta);
  const double nx = sqrt(x[0] * x[0] + x[1] * x[1] + x[2] * x[2]);
  const double sn = sin(n) / n;
  const double y[3] = {sn * d[0], sn * d[1], cos(n)};
  const double vy = beta * (v[0] * y[0] + v[1] * y[1] + v[2] * y[2]);
  out[0] = nx * (y[0] - vy * v[0]);
  out[1] = nx * (y[1] - vy * v[1]);
  out[2] = nx * (y[2] - vy * v[2]);
}

// SphereManifold<3>::PlusJacobian, 3 x 2 row-major: column i = |x| (e_i - beta v_i v).
MI_HD void sphere_plus_jacobian(const double x[3], double J[6]) {
  double v[3], beta;
  sphere_householder(x, v, &beta);
  const double nx = sqrt(x[0] * x[0] + x[1] * x[1] + x[2] * x[2]);
  MI_UNROLL
  for (int i = 0; i < 2; ++i) {
    MI_UNROLL
    for (int r = 0; r < 3; ++r) J[r * 2 + i] = nx * ((r == i ? 1.0 : 0.0) - beta * v[i] * v[r]);
  }
}

// What every correspondence of one problem shares at a point (q, t).
struct RelPoseFrame {
  double R[9];   // QuaternionToRotation(q)
  double E[9];   // [t]x R
  double t[3];
  double Jt[6];  // sphere_plus_jacobian(t)
};

MI_HD void relpose_frame(const double q[4], const double t[3], bool with_jacobian, RelPoseFrame* f) {
  quat_to_rotation(q, f->R);
  const double* R = f->R;
  MI_UNROLL
  for (int c = 0; c < 3; ++c) {
    f->E[c] = t[1] * R[6 + c] - t[2] * R[3 + c];
    f->E[3 + c] = t[2] * R[c] - t[0] * R[6 + c];
    f->E[6 + c] = t[0] * R[3 + c] - t[1] * R[c];
  }
  f->t[0] = t[0]; f->t[1] = t[1]; f->t[2] = t[2];
  if (with_jacobian) sphere_plus_jacobian(t, f->Jt);
}

// r = (x2' E x1)^2 / (a0^2 + a1^2 + b0^2 + b1^2), a = E x1, b = E' x2.
MI_HD double relpose_residual(const double E[9], double x1, double y1, double x2, double y2) {
  const double a0 = E[0] * x1 + E[1] * y1 + E[2];
  const double a1 = E[3] * x1 + E[4] * y1 + E[5];
  const double a2 = E[6] * x1 + E[7] * y1 + E[8];
  const double b0 = E[0] * x2 + E[3] * y2 + E[6];
  const double b1 = E[1] * x2 + E[4] * y2 + E[7];
  const double s = x2 * a0 + y2 * a1 + a2;
  return s * s / (a0 * a0 + a1 * a1 + b0 * b0 + b1 * b1);
}

// The residual and its derivative by the tangent (rotation 3, sphere 2).
// G = dr/dE; with K = G R': a translation change u gives dr = u . axial(K),
// axial(K) = (K21 - K12, K02 - K20, K10 - K01); a rotation delta gives
// dr = 2 delta . axial([t]x' K).
MI_HD double relpose_residual_jacobian(const RelPoseFrame& f, double x1, double y1, double x2, double y2, double J[5]) {
  const double* E = f.E;
  const double a0 = E[0] * x1 + E[1] * y1 + E[2];
  const double a1 = E[3] * x1 + E[4] * y1 + E[5];
  const double a2 = E[6] * x1 + E[7] * y1 + E[8];
  const double b0 = E[0] * x2 + E[3] * y2 + E[6];
  const double b1 = E[1] * x2 + E[4] * y2 + E[7];
  const double s = x2 * a0 + y2 * a1 + a2;
  const double d = a0 * a0 + a1 * a1 + b0 * b0 + b1 * b1;
  const double r = s * s / d;
  const double g1 = 2.0 * s / d, g2 = 2.0 * r / d;
  // G = g1 x2h x1h' - g2 ((a0, a1, 0)' x1h' + x2h (b0, b1, 0))
  const double X1[3] = {x1, y1, 1.0}, X2[3] = {x2, y2, 1.0}, A[3] = {a0, a1, 0.0}, B[3] = {b0, b1, 0.0};
  double G[9], K[9];
  MI_UNROLL
  for (int i = 0; i < 3; ++i) {
    MI_UNROLL
    for (int j = 0; j < 3; ++j) G[i * 3 + j] = (g1 * X2[i] - g2 * A[i]) * X1[j] - g2 * X2[i] * B[j];
  }
  const double* R = f.R;
  MI_UNROLL
  for (int i = 0; i < 3; ++i) {
    MI_UNROLL
    for (int j = 0; j < 3; ++j) K[i * 3 + j] = G[i * 3] * R[j * 3] + G[i * 3 + 1] * R[j * 3 + 1] + G[i * 3 + 2] * R[j * 3 + 2];
  }
  const double w[3] = {K[7] - K[5], K[2] - K[6], K[3] - K[1]};
  J[3] = w[0] * f.Jt[0] + w[1] * f.Jt[2] + w[2] * f.Jt[4];
  J[4] = w[0] * f.Jt[1] + w[1] * f.Jt[3] + w[2] * f.Jt[5];
  // H = [t]x' K = -[t]x K: column c of H is -(t x K[:, c])
  const double* t = f.t;
  double H[9];
  MI_UNROLL
  for (int c = 0; c < 3; ++c) {
    H[c] = -(t[1] * K[6 + c] - t[2] * K[3 + c]);
    H[3 + c] = -(t[2] * K[c] - t[0] * K[6 + c]);
    H[6 + c] = -(t[0] * K[3 + c] - t[1] * K[c]);
  }
  J[0] = 2.0 * (H[7] - H[5]);
  J[1] = 2.0 * (H[2] - H[6]);
  J[2] = 2.0 * (H[3] - H[1]);
  return r;
}

}  // namespace miba
