// reproj_block.h — the chain rule of one reprojection block
// (BundleAdjustmentCostFunction, src/base/cost_functions.h:57-81), shared by
// the kernels that evaluate its tangent Jacobian: reproj_jacobian_kernel
// (kernels.hip) and pose_refine_kernel (pose_refine.hip).  One implementation,
// so both compute the same arithmetic.
#pragma once

#include "ba_math.h"

namespace miba {

// Refined-intrinsics mask per model and refine flags (bit 0 focal, bit 1
// principal point, bit 2 extra params): camera_models.h *Idxs, and
// BundleAdjuster::ParameterizeCameras (bundle_adjustment.cc:480-516).
MI_HD constexpr unsigned cam_tangent_mask(int M, int RF) {
  unsigned f = 0, pp = 0, ex = 0;
  if (M == kSimplePinhole) { f = 0x1; pp = 0x6; ex = 0x0; }
  if (M == kPinhole) { f = 0x3; pp = 0xC; ex = 0x0; }
  if (M == kSimpleRadial) { f = 0x1; pp = 0x6; ex = 0x8; }
  if (M == kRadial) { f = 0x1; pp = 0x6; ex = 0x18; }
  if (M == kOpenCV) { f = 0x3; pp = 0xC; ex = 0xF0; }
  return ((RF & 1) ? f : 0u) | ((RF & 2) ? pp : 0u) | ((RF & 4) ? ex : 0u);
}
// The same over all nine models (camera_models.h: OPENCV_FISHEYE and FOV
// fx fy cx cy + extras, the RADIAL_FISHEYEs f cx cy + extras).  The run-time
// callers of the five-model kernels keep cam_tangent_mask.
MI_HD constexpr unsigned cam_tangent_mask_all(int M, int RF) {
  unsigned f = 0, pp = 0, ex = 0;
  if (M == kOpenCVFisheye) { f = 0x3; pp = 0xC; ex = 0xF0; }
  else if (M == kFOV) { f = 0x3; pp = 0xC; ex = 0x10; }
  else if (M == kSimpleRadialFisheye) { f = 0x1; pp = 0x6; ex = 0x8; }
  else if (M == kRadialFisheye) { f = 0x1; pp = 0x6; ex = 0x18; }
  else return cam_tangent_mask(M, RF);
  return ((RF & 1) ? f : 0u) | ((RF & 2) ? pp : 0u) | ((RF & 4) ? ex : 0u);
}
MI_HD constexpr int popcount8(unsigned m) {
  return (int)((m & 1) + ((m >> 1) & 1) + ((m >> 2) & 1) + ((m >> 3) & 1) + ((m >> 4) & 1) + ((m >> 5) & 1) +
               ((m >> 6) & 1) + ((m >> 7) & 1));
}

// B = d(x, y)/dP (2 x 3 row-major) of the pixel by the camera-frame point
// P = R X + t, from A = d(x, y)/d(u, v) of the camera model at (u, v) =
// (P0, P1) / P2 and iz = 1 / P2.
MI_HD void reproj_dpixel_dpoint(const double A[4], double iz, double u, double v, double B[6]) {
  B[0] = A[0] * iz; B[1] = A[1] * iz; B[2] = -(A[0] * u + A[1] * v) * iz;
  B[3] = A[2] * iz; B[4] = A[3] * iz; B[5] = -(A[2] * u + A[3] * v) * iz;
}

// |q|^2 is 1 within 1e-12: the closed-form rotation columns below apply.
MI_HD bool quat_is_unit(const double q[4]) {
  return fabs(q[0] * q[0] + q[1] * q[1] + q[2] * q[2] + q[3] * q[3] - 1.0) <= 1e-12;
}

// Mq = d(R X)/d(tangent) of QuaternionManifold (plus = q_delta * q, rotation
// angle 2|delta|), 3 x 3 row-major, a = R X.  For a unit q it is -2 [R X]x;
// the general product Dq * PlusJacobian serves a quaternion that is not
// normalised, as AutoDiff would (equal up to rounding for a unit q).  Mq is
// left as it is for a constant pose.
MI_HD void rotation_tangent_jacobian(const double q[4], const double X[3], double a0, double a1, double a2,
                                     bool pose_var, bool unit_q, double Mq[9]) {
  if (pose_var && unit_q) {
    Mq[0] = 0.0;       Mq[1] = 2.0 * a2;  Mq[2] = -2.0 * a1;
    Mq[3] = -2.0 * a2; Mq[4] = 0.0;       Mq[5] = 2.0 * a0;
    Mq[6] = 2.0 * a1;  Mq[7] = -2.0 * a0; Mq[8] = 0.0;
  } else if (pose_var) {
    double Dq[12], PJ[12];
    unit_quat_rotate_dq(q, X, Dq);
    quat_plus_jacobian(q, PJ);
    MI_UNROLL
    for (int a = 0; a < 3; ++a)
      MI_UNROLL
      for (int b = 0; b < 3; ++b)
        Mq[a * 3 + b] = Dq[a * 4 + 0] * PJ[0 * 3 + b] + Dq[a * 4 + 1] * PJ[1 * 3 + b] +
                        Dq[a * 4 + 2] * PJ[2 * 3 + b] + Dq[a * 4 + 3] * PJ[3 * 3 + b];
  }
}

// Pose columns of one block row (rw = 0: x, 1: y): rotation tangent (3) into
// dst[0..3), translation (3) into dst[3..6); flags bit 1 + b = tvec[b]
// constant.  B is loss-corrected by the caller.
MI_HD void emit_row_pose(int rw, double* dst, const double (&B)[6], const double (&Mq)[9], bool pose_var,
                         uint32_t flags) {
  MI_UNROLL
  for (int b = 0; b < 3; ++b)
    dst[b] = pose_var ? B[rw * 3 + 0] * Mq[b] + B[rw * 3 + 1] * Mq[3 + b] + B[rw * 3 + 2] * Mq[6 + b] : 0.0;
  MI_UNROLL
  for (int b = 0; b < 3; ++b) dst[3 + b] = (pose_var && !((flags >> (1 + b)) & 1u)) ? B[rw * 3 + b] : 0.0;
}

}  // namespace miba
