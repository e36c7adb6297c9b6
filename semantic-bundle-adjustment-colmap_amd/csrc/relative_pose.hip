// relative_pose.hip — batched two-view (relative) pose refinement (product
// code).
//
//   mi_ba_refine_relative_pose_batch
//       <- RefineRelativePose (src/estimators/pose.cc:324-352)
//
// The residual is RelativePoseCostFunction's squared Sampson error
// (cost_functions.h:216-268, relative_pose_block.h), one row per
// correspondence, under CauchyLoss; q lives on QuaternionManifold, t on
// SphereManifold<3>: a tangent of 3 + 2.
//
// One wavefront per problem, four problems per workgroup, the whole
// Levenberg-Marquardt loop on the device.  The waves of a workgroup share
// nothing: there is no workgroup barrier and no atomic.  Lane l takes the
// correspondences l, l + 64, ... in that order and keeps its 20 sums (the
// upper triangle of J'J and J'r) and its cost in registers; an xor tree then
// adds the 64 lanes.  Floating-point addition commutes, so after the tree every
// lane holds the same bits: the 5 x 5 system, its Cholesky, the step and the
// LM state live in registers of every lane, redundantly, and every branch on
// them is uniform across the wave.  Every sum has a fixed order that depends
// on the problem alone.
//
// Correspondences (x1, y1, x2, y2) stay resident in the wave's quarter of the
// LDS as a struct of arrays up to kRLdsObs of them; a problem with more
// streams them from device memory on every pass.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstring>
#include <vector>

#include "../../include/mi_ba.h"
#include "ba_math.h"
#include "pose_common.h"
#include "relative_pose_block.h"

namespace miba {
namespace {

// 4 waves x 4 arrays x 1024 doubles = 128 KiB of the 160 KiB; a launch sizes
// the arrays by its largest resident problem, so batches of a few hundred
// correspondences keep several workgroups on a CU.
constexpr int kRLdsObs = 1024;
constexpr int kRTangent = 5;
constexpr int kRSums = 20;  // upper triangle of the 5 x 6 [J'J | J'r]
static_assert(kPoseWaves * 4 * kRLdsObs * 8 <= 160 * 1024, "LDS budget of one workgroup");

struct RProblemDev {
  int64_t begin;  // first correspondence in the uploaded arrays
  int32_t count, index;
};

struct RPoseArgs {
  const RProblemDev* prob;
  const double2* p1;
  const double2* p2;
  double* pose;  // [n][8] q(4) t(3) pad, in/out
  double* out;   // [n][kOutStride]
  double function_tolerance, gradient_tolerance, parameter_tolerance, loss_scale;
  int32_t max_num_iterations;
  int32_t num_listed;
  int32_t lds_obs;
  uint8_t* trace;
  int32_t trace_cap;
};

struct RObsSource {
  const double* sx;   // LDS, struct of arrays (resident) ...
  const double2* p1;  // ... or device memory
  const double2* p2;
  int lds_obs;
  bool resident;
  __device__ __forceinline__ void load(int i, double* x1, double* y1, double* x2, double* y2) const {
    if (resident) {
      *x1 = sx[i];
      *y1 = sx[lds_obs + i];
      *x2 = sx[2 * lds_obs + i];
      *y2 = sx[3 * lds_obs + i];
    } else {
      const double2 a = p1[i], b = p2[i];
      *x1 = a.x;
      *y1 = a.y;
      *x2 = b.x;
      *y2 = b.y;
    }
  }
};

// [J'J | J'r] (upper triangle, row major: S[0..5] row 0, S[6..10] row 1, ...)
// of the loss-corrected rows and the cost 0.5 sum rho(r^2) at (q, t); every
// lane returns the same bits.
__device__ inline void rpose_linearize(const RObsSource& src, int count, int lane, const double q[4], const double t[3],
                                       double loss_scale, double (&S)[kRSums], double* cost) {
  RelPoseFrame f;
  relpose_frame(q, t, true, &f);
  double c = 0.0;
#pragma unroll
  for (int e = 0; e < kRSums; ++e) S[e] = 0.0;
#pragma unroll 1
  for (int i = lane; i < count; i += 64) {
    double x1, y1, x2, y2, row[kRTangent + 1], rho[3];
    src.load(i, &x1, &y1, &x2, &y2);
    const double r = relpose_residual_jacobian(f, x1, y1, x2, y2, row);
    loss_eval(kLossCauchy, loss_scale, r * r, rho);
    c += 0.5 * rho[0];
    // Ceres Corrector, rho'' <= 0 branch: r, J *= sqrt(rho')
    const double sc = sqrt(rho[1]);
#pragma unroll
    for (int k = 0; k < kRTangent; ++k) row[k] *= sc;
    row[kRTangent] = r * sc;
    int e = 0;
#pragma unroll
    for (int a = 0; a < kRTangent; ++a)
#pragma unroll
      for (int b = a; b <= kRTangent; ++b) S[e++] += row[a] * row[b];
  }
#pragma unroll
  for (int e = 0; e < kRSums; ++e) S[e] = wave_sum_fixed(S[e]);
  *cost = wave_sum_fixed(c);
}

__device__ inline double rpose_cost(const RObsSource& src, int count, int lane, const double q[4], const double t[3],
                                    double loss_scale) {
  RelPoseFrame f;
  relpose_frame(q, t, false, &f);
  double c = 0.0;
#pragma unroll 1
  for (int i = lane; i < count; i += 64) {
    double x1, y1, x2, y2, rho[3];
    src.load(i, &x1, &y1, &x2, &y2);
    const double r = relpose_residual(f.E, x1, y1, x2, y2);
    loss_eval(kLossCauchy, loss_scale, r * r, rho);
    c += 0.5 * rho[0];
  }
  return wave_sum_fixed(c);
}

// In-register Cholesky of the 5 x 5 lower triangle A (in place) and the solve
// of L L' x = b.  false if a pivot is not positive.
__device__ __forceinline__ bool chol5_solve(double (&A)[kRTangent][kRTangent], const double (&b)[kRTangent],
                                            double (&x)[kRTangent]) {
  bool ok = true;
#pragma unroll
  for (int k = 0; k < kRTangent; ++k) {
    const double akk = A[k][k];
    if (!(akk > 0.0)) ok = false;
    const double lkk = sqrt(akk);
    A[k][k] = lkk;
#pragma unroll
    for (int i = k + 1; i < kRTangent; ++i) A[i][k] = A[i][k] / lkk;
#pragma unroll
    for (int i = k + 1; i < kRTangent; ++i)
#pragma unroll
      for (int j = k + 1; j <= i; ++j) A[i][j] -= A[i][k] * A[j][k];
  }
#pragma unroll
  for (int k = 0; k < kRTangent; ++k) {
    double v = b[k];
#pragma unroll
    for (int j = 0; j < k; ++j) v -= A[k][j] * x[j];
    x[k] = v / A[k][k];
  }
#pragma unroll
  for (int k = kRTangent - 1; k >= 0; --k) {
    double v = x[k];
#pragma unroll
    for (int j = k + 1; j < kRTangent; ++j) v -= A[j][k] * x[j];
    x[k] = v / A[k][k];
  }
  return ok;
}

__global__ __launch_bounds__(kPoseTB) void relative_pose_kernel(RPoseArgs a) {
  extern __shared__ double lds[];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int slot = blockIdx.x * kPoseWaves + wave;
  if (slot >= a.num_listed) return;
  const RProblemDev pb = a.prob[slot];
  const int count = pb.count, index = pb.index;
  double* sObs = lds + (size_t)wave * 4 * a.lds_obs;
  RObsSource src;
  src.sx = sObs;
  src.p1 = a.p1 + pb.begin;
  src.p2 = a.p2 + pb.begin;
  src.lds_obs = a.lds_obs;
  src.resident = count <= a.lds_obs;
  if (src.resident) {
    // lane l reads back only what lane l wrote
    for (int i = lane; i < count; i += 64) {
      const double2 u = src.p1[i], v = src.p2[i];
      sObs[i] = u.x;
      sObs[a.lds_obs + i] = u.y;
      sObs[2 * a.lds_obs + i] = v.x;
      sObs[3 * a.lds_obs + i] = v.y;
    }
    wave_sync();
  }
  double q[4], t[3];
#pragma unroll
  for (int m = 0; m < 4; ++m) q[m] = a.pose[(size_t)index * 8 + m];
#pragma unroll
  for (int m = 0; m < 3; ++m) t[m] = a.pose[(size_t)index * 8 + 4 + m];

  double S[kRSums], x_cost;
  rpose_linearize(src, count, lane, q, t, a.loss_scale, S, &x_cost);
  const double initial_cost = x_cost;
  // Jacobi scaling from the first Jacobian
  double scale[kRTangent];
  {
    int e = 0;
#pragma unroll
    for (int k = 0; k < kRTangent; ++k) {
      scale[k] = lm_jacobi_scale(S[e]);
      e += kRTangent + 1 - k;
    }
  }
  double radius = kInitialRadius, decrease_factor = 2.0;
  int iteration = 0, consecutive_invalid = 0, n_successful = 0, n_unsuccessful = 0;
  int termination = MI_BA_NO_CONVERGENCE;
  bool last_successful = true;  // iteration 0 counts as successful (IterationZero)
  // a non-finite initial cost: FAILURE, parameters untouched
  bool go = isfinite(x_cost);
  if (!go) termination = MI_BA_FAILURE;
#pragma unroll 1
  while (go) {
    // FinalizeIterationAndCheckIfMinimizerCanContinue
    if (iteration >= a.max_num_iterations) {
      termination = MI_BA_NO_CONVERGENCE;
      break;
    }
    // M: the symmetric 5 x 5 J'J, g = J'r
    double M[kRTangent][kRTangent], g[kRTangent];
    {
      int e = 0;
#pragma unroll
      for (int i = 0; i < kRTangent; ++i) {
#pragma unroll
        for (int j = i; j < kRTangent; ++j) {
          M[i][j] = S[e];
          M[j][i] = S[e];
          ++e;
        }
        g[i] = S[e++];
      }
    }
    if (last_successful) {
      // GradientToleranceReached: |x - Plus(x, -g)|_inf
      const double dq[3] = {-g[0], -g[1], -g[2]}, dt[2] = {-g[3], -g[4]};
      double qn[4], tn[3], gmax = 0.0;
      quat_plus(q, dq, qn);
      sphere_plus(t, dt, tn);
#pragma unroll
      for (int m = 0; m < 4; ++m) gmax = fmax(gmax, fabs(q[m] - qn[m]));
#pragma unroll
      for (int m = 0; m < 3; ++m) gmax = fmax(gmax, fabs(t[m] - tn[m]));
      if (gmax <= a.gradient_tolerance) {
        termination = MI_BA_CONVERGENCE;
        break;
      }
    }
    if (radius <= kMinRadius) {
      termination = MI_BA_CONVERGENCE;
      break;
    }
    iteration += 1;
    // the scaled, damped system; LM diagonal: the clipped scaled column norm over the radius
    double A[kRTangent][kRTangent], gs[kRTangent], y[kRTangent];
#pragma unroll
    for (int i = 0; i < kRTangent; ++i) {
#pragma unroll
      for (int j = 0; j <= i; ++j) {
        double v = M[i][j] * scale[i] * scale[j];
        if (j == i) v = lm_damped_diagonal(v, radius);
        A[i][j] = v;
      }
      gs[i] = g[i] * scale[i];
    }
    bool ok = chol5_solve(A, gs, y);
    double step[kRTangent], model = 0.0;
    if (ok) {
      // Ceres solves (J'J + D'D) x = J'r, step = -x
#pragma unroll
      for (int i = 0; i < kRTangent; ++i) step[i] = -y[i];
      double total = 0.0;
#pragma unroll
      for (int i = 0; i < kRTangent; ++i) {
        double hstep = 0.0;
#pragma unroll
        for (int j = 0; j < kRTangent; ++j) hstep += M[i][j] * scale[i] * scale[j] * step[j];
        total += step[i] * (gs[i] + 0.5 * hstep);
      }
      model = -total;
      ok = isfinite(model) && model > 0.0;
    }
    if (!ok) {
      consecutive_invalid += 1;
      last_successful = false;
      n_unsuccessful += 1;
      lm_radius_reject(radius, decrease_factor);
      const bool end = consecutive_invalid > kMaxConsecutiveInvalid;
      if (lane == 0) pose_trace(a.trace, a.trace_cap, index, iteration, 0, 0, end ? 1 : 0);
      if (end) {
        termination = MI_BA_FAILURE;
        break;
      }
      continue;
    }
    consecutive_invalid = 0;
    // candidate = Plus(x, step * scale)
    double qc[4], tc[3];
    {
      const double dq[3] = {step[0] * scale[0], step[1] * scale[1], step[2] * scale[2]};
      const double dt[2] = {step[3] * scale[3], step[4] * scale[4]};
      quat_plus(q, dq, qc);
      sphere_plus(t, dt, tc);
    }
    // |x|, |x - candidate| over qvec and tvec in ambient coordinates
    double xn2 = 0.0, sn2 = 0.0;
#pragma unroll
    for (int m = 0; m < 4; ++m) {
      const double dv = q[m] - qc[m];
      xn2 += q[m] * q[m];
      sn2 += dv * dv;
    }
#pragma unroll
    for (int m = 0; m < 3; ++m) {
      const double dv = t[m] - tc[m];
      xn2 += t[m] * t[m];
      sn2 += dv * dv;
    }
    const double x_norm = sqrt(xn2), step_norm = sqrt(sn2);
    const double cand_cost = rpose_cost(src, count, lane, qc, tc, a.loss_scale);
    const double cost_change = x_cost - cand_cost;
    const double relative_decrease = cost_change / model;
    const bool success = lm_step_successful(cand_cost, relative_decrease);
    // Ceres returns before accepting the candidate
    const bool tol = lm_tolerance_reached(step_norm, x_norm, cost_change, x_cost, a.parameter_tolerance,
                                          a.function_tolerance);
    if (tol) {
      n_unsuccessful += 1;
      termination = MI_BA_CONVERGENCE;
      if (lane == 0) pose_trace(a.trace, a.trace_cap, index, iteration, 1, 0, 1);
      break;
    }
    if (success) {
#pragma unroll
      for (int m = 0; m < 4; ++m) q[m] = qc[m];
#pragma unroll
      for (int m = 0; m < 3; ++m) t[m] = tc[m];
      n_successful += 1;
      last_successful = true;
      lm_radius_accept(radius, decrease_factor, relative_decrease);
      if (lane == 0) pose_trace(a.trace, a.trace_cap, index, iteration, 1, 1, 0);
      double ignored;
      rpose_linearize(src, count, lane, q, t, a.loss_scale, S, &ignored);
      x_cost = cand_cost;
    } else {
      n_unsuccessful += 1;
      last_successful = false;
      lm_radius_reject(radius, decrease_factor);
      if (lane == 0) pose_trace(a.trace, a.trace_cap, index, iteration, 1, 0, 0);
    }
  }

  if (lane != 0) return;
  if (termination != MI_BA_FAILURE) {
#pragma unroll
    for (int m = 0; m < 4; ++m) a.pose[(size_t)index * 8 + m] = q[m];
#pragma unroll
    for (int m = 0; m < 3; ++m) a.pose[(size_t)index * 8 + 4 + m] = t[m];
  }
  double* out = a.out + (size_t)index * kOutStride;
  out[0] = initial_cost;
  out[1] = x_cost;
  out[2] = n_successful;
  out[3] = n_unsuccessful;
  out[4] = termination;
}

// Residuals and tangent Jacobians, not loss-corrected: one workgroup of one
// wave per problem.
__global__ __launch_bounds__(64) void relative_pose_evaluate_kernel(const RProblemDev* prob, const double2* p1,
                                                                    const double2* p2, const double* pose,
                                                                    double* residuals, double* jacobians) {
  const RProblemDev pb = prob[blockIdx.x];
  double q[4], t[3];
#pragma unroll
  for (int m = 0; m < 4; ++m) q[m] = pose[(size_t)pb.index * 8 + m];
#pragma unroll
  for (int m = 0; m < 3; ++m) t[m] = pose[(size_t)pb.index * 8 + 4 + m];
  RelPoseFrame f;
  relpose_frame(q, t, true, &f);
  for (int i = threadIdx.x; i < pb.count; i += 64) {
    const double2 u = p1[pb.begin + i], v = p2[pb.begin + i];
    double J[kRTangent];
    residuals[pb.begin + i] = relpose_residual_jacobian(f, u.x, u.y, v.x, v.y, J);
#pragma unroll
    for (int k = 0; k < kRTangent; ++k) jacobians[(size_t)(pb.begin + i) * kRTangent + k] = J[k];
  }
}

// The argument checks of both entry points.  Host only.
mi_ba_status relative_pose_check(const mi_ba_relative_pose_options* o, const mi_ba_relative_pose_batch* b) {
  if (!o || !b || b->num_problems < 0) return MI_BA_ERR_INVALID_ARGUMENT;
  if (!pose_options_check(o->gradient_tolerance, o->max_num_iterations, o->loss_function_scale, o->function_tolerance,
                          o->parameter_tolerance))
    return MI_BA_ERR_INVALID_ARGUMENT;
  const int n = b->num_problems;
  if (n == 0) return MI_BA_OK;
  if (!b->obs_offsets || !b->qvec || !b->tvec || b->obs_offsets[0] < 0) return MI_BA_ERR_INVALID_ARGUMENT;
  for (int k = 0; k < n; ++k) {
    const int64_t c = b->obs_offsets[k + 1] - b->obs_offsets[k];
    if (c < 0 || c > INT32_MAX) return MI_BA_ERR_INVALID_ARGUMENT;
  }
  if (b->obs_offsets[n] > b->obs_offsets[0] && (!b->points1 || !b->points2)) return MI_BA_ERR_INVALID_ARGUMENT;
  return MI_BA_OK;
}

// NormalizeQuaternion (src/base/pose.cc): q / |q|, the identity for |q| = 0.
void relative_pose_unit_quat(const double* q, double* dst) {
  const double nq = std::sqrt(q[0] * q[0] + q[1] * q[1] + q[2] * q[2] + q[3] * q[3]);
  for (int m = 0; m < 4; ++m) dst[m] = nq == 0.0 ? (m == 0 ? 1.0 : 0.0) : q[m] / nq;
}

}  // namespace
}  // namespace miba

using namespace miba;

extern "C" void mi_ba_default_relative_pose_options(mi_ba_relative_pose_options* o) {
  if (!o) return;
  std::memset(o, 0, sizeof(*o));
  // ceres::Solver::Options' defaults (solver.h)
  o->max_num_iterations = 50;
  o->function_tolerance = 1e-6;
  o->gradient_tolerance = 1e-10;
  o->parameter_tolerance = 1e-8;
  o->loss_function_scale = 1.0;
  o->device = 0;
}

extern "C" int32_t mi_ba_relative_pose_lds_capacity(void) { return kRLdsObs; }

extern "C" mi_ba_status mi_ba_refine_relative_pose_batch(const mi_ba_relative_pose_options* o,
                                                         const mi_ba_relative_pose_batch* b, int32_t* statuses,
                                                         mi_ba_summary* summaries, int32_t* usable) {
  mi_ba_status st = relative_pose_check(o, b);
  if (st != MI_BA_OK) return st;
  const int n = b->num_problems;
  if (n == 0) return MI_BA_OK;
  if (!statuses || !summaries || !usable) return MI_BA_ERR_INVALID_ARGUMENT;
  st = pose_select_device(o->device);
  if (st != MI_BA_OK) return st;

  // Host assembly: without a mask the caller's arrays are uploaded as they
  // are; with one the inliers are compacted, so a masked call runs the
  // arithmetic of the compacted call.
  const int64_t raw0 = b->obs_offsets[0];
  const bool masked = b->inlier_mask != nullptr;
  std::vector<double> c1, c2, pose(8 * (size_t)n, 0.0);
  std::vector<RProblemDev> list;
  int64_t at = 0;
  int most_resident = 0;
  for (int k = 0; k < n; ++k) {
    std::memset(&summaries[k], 0, sizeof(mi_ba_summary));
    statuses[k] = MI_BA_OK;
    usable[k] = 0;
    const int64_t i0 = b->obs_offsets[k], i1 = b->obs_offsets[k + 1];
    int64_t inliers = i1 - i0;
    const int64_t begin = masked ? at : i0 - raw0;
    if (masked) {
      inliers = 0;
      for (int64_t i = i0; i < i1; ++i) {
        if (!b->inlier_mask[i]) continue;
        c1.push_back(b->points1[2 * i]);
        c1.push_back(b->points1[2 * i + 1]);
        c2.push_back(b->points2[2 * i]);
        c2.push_back(b->points2[2 * i + 1]);
        ++inliers;
      }
      at += inliers;
    }
    summaries[k].num_residuals_reduced = inliers;
    summaries[k].num_effective_parameters_reduced = inliers ? kRTangent : 0;
    if (inliers == 0) {  // no residuals: nothing to do
      summaries[k].termination_type = MI_BA_CONVERGENCE;
      usable[k] = 1;
      continue;
    }
    relative_pose_unit_quat(b->qvec + 4 * (size_t)k, &pose[8 * (size_t)k]);
    for (int m = 0; m < 3; ++m) pose[8 * (size_t)k + 4 + m] = b->tvec[3 * (size_t)k + m];
    list.push_back(RProblemDev{begin, (int32_t)inliers, k});
    if (inliers <= kRLdsObs && inliers > most_resident) most_resident = (int)inliers;
  }
  if (list.empty()) return MI_BA_OK;

  const int64_t N = masked ? at : b->obs_offsets[n] - raw0;
  const double* h1 = masked ? c1.data() : b->points1 + 2 * raw0;
  const double* h2 = masked ? c2.data() : b->points2 + 2 * raw0;
  Buf bufs[5];
  double2* d1 = bufs[0].alloc<double2>(N);
  double2* d2 = bufs[1].alloc<double2>(N);
  double* dpose = bufs[2].alloc<double>(pose.size());
  double* dout = bufs[3].alloc<double>(kOutStride * (size_t)n);
  RProblemDev* dprob = bufs[4].alloc<RProblemDev>(list.size());
  if (!d1 || !d2 || !dpose || !dout || !dprob) return MI_BA_ERR_OUT_OF_MEMORY;
  if (hipMemcpy(d1, h1, (size_t)N * 16, hipMemcpyHostToDevice) != hipSuccess ||
      hipMemcpy(d2, h2, (size_t)N * 16, hipMemcpyHostToDevice) != hipSuccess ||
      hipMemcpy(dpose, pose.data(), pose.size() * 8, hipMemcpyHostToDevice) != hipSuccess ||
      hipMemcpy(dprob, list.data(), list.size() * sizeof(RProblemDev), hipMemcpyHostToDevice) != hipSuccess ||
      hipMemset(dout, 0, kOutStride * (size_t)n * 8) != hipSuccess)
    return MI_BA_ERR_HIP;
  RPoseArgs a{};
  a.prob = dprob;
  a.p1 = d1;
  a.p2 = d2;
  a.pose = dpose;
  a.out = dout;
  a.function_tolerance = o->function_tolerance;
  a.gradient_tolerance = o->gradient_tolerance;
  a.parameter_tolerance = o->parameter_tolerance;
  a.loss_scale = o->loss_function_scale;
  a.max_num_iterations = o->max_num_iterations;
  a.num_listed = (int32_t)list.size();
  // the arrays' stride only: a problem is resident exactly when its own count is at most kRLdsObs
  a.lds_obs = (most_resident + 63) / 64 * 64;
  PoseTraceBuf trace;
  st = trace.setup(n);
  if (st != MI_BA_OK) return st;
  a.trace = trace.dev;
  a.trace_cap = trace.cap;
  const size_t bytes = (size_t)kPoseWaves * 4 * a.lds_obs * 8;
  if (hipFuncSetAttribute(reinterpret_cast<const void*>(&relative_pose_kernel),
                          hipFuncAttributeMaxDynamicSharedMemorySize, (int)bytes) != hipSuccess)
    return MI_BA_ERR_HIP;
  const unsigned groups = (unsigned)((list.size() + kPoseWaves - 1) / kPoseWaves);
  hipLaunchKernelGGL(relative_pose_kernel, dim3(groups), dim3(kPoseTB), bytes, 0, a);
  if (hipGetLastError() != hipSuccess) return MI_BA_ERR_HIP;
  if (hipStreamSynchronize(0) != hipSuccess) return MI_BA_ERR_HIP;
  std::vector<double> out(kOutStride * (size_t)n);
  if (!pose_download(&pose, dpose) || !pose_download(&out, dout) || trace.download() != MI_BA_OK)
    return MI_BA_ERR_HIP;
  for (const RProblemDev& pb : list) {
    const int k = pb.index;
    const bool ok = pose_summary_fill(&out[kOutStride * (size_t)k], &summaries[k]);
    if (ok) {
      for (int m = 0; m < 4; ++m) b->qvec[4 * (size_t)k + m] = pose[8 * (size_t)k + m];
      for (int m = 0; m < 3; ++m) b->tvec[3 * (size_t)k + m] = pose[8 * (size_t)k + 4 + m];
    }
    usable[k] = ok ? 1 : 0;
  }
  return MI_BA_OK;
}

extern "C" mi_ba_status mi_ba_relative_pose_evaluate(const mi_ba_relative_pose_options* o,
                                                     const mi_ba_relative_pose_batch* b, double* residuals,
                                                     double* jacobians) {
  mi_ba_status st = relative_pose_check(o, b);
  if (st != MI_BA_OK) return st;
  const int n = b->num_problems;
  if (n == 0) return MI_BA_OK;
  const int64_t raw0 = b->obs_offsets[0], N = b->obs_offsets[n] - raw0;
  if (N == 0) return MI_BA_OK;
  if (!residuals || !jacobians) return MI_BA_ERR_INVALID_ARGUMENT;
  st = pose_select_device(o->device);
  if (st != MI_BA_OK) return st;
  std::vector<RProblemDev> list;
  std::vector<double> pose(8 * (size_t)n, 0.0);
  for (int k = 0; k < n; ++k) {
    for (int m = 0; m < 4; ++m) pose[8 * (size_t)k + m] = b->qvec[4 * (size_t)k + m];
    for (int m = 0; m < 3; ++m) pose[8 * (size_t)k + 4 + m] = b->tvec[3 * (size_t)k + m];
    list.push_back(RProblemDev{b->obs_offsets[k] - raw0, (int32_t)(b->obs_offsets[k + 1] - b->obs_offsets[k]), k});
  }
  Buf bufs[6];
  double2* d1 = bufs[0].alloc<double2>(N);
  double2* d2 = bufs[1].alloc<double2>(N);
  double* dpose = bufs[2].alloc<double>(pose.size());
  RProblemDev* dprob = bufs[3].alloc<RProblemDev>(list.size());
  double* dres = bufs[4].alloc<double>(N);
  double* djac = bufs[5].alloc<double>(kRTangent * (size_t)N);
  if (!d1 || !d2 || !dpose || !dprob || !dres || !djac) return MI_BA_ERR_OUT_OF_MEMORY;
  if (hipMemcpy(d1, b->points1 + 2 * raw0, (size_t)N * 16, hipMemcpyHostToDevice) != hipSuccess ||
      hipMemcpy(d2, b->points2 + 2 * raw0, (size_t)N * 16, hipMemcpyHostToDevice) != hipSuccess ||
      hipMemcpy(dpose, pose.data(), pose.size() * 8, hipMemcpyHostToDevice) != hipSuccess ||
      hipMemcpy(dprob, list.data(), list.size() * sizeof(RProblemDev), hipMemcpyHostToDevice) != hipSuccess)
    return MI_BA_ERR_HIP;
  hipLaunchKernelGGL(relative_pose_evaluate_kernel, dim3((unsigned)n), dim3(64), 0, 0, dprob, d1, d2, dpose, dres,
                     djac);
  if (hipGetLastError() != hipSuccess || hipStreamSynchronize(0) != hipSuccess) return MI_BA_ERR_HIP;
  // the outputs are indexed like the caller's arrays
  if (hipMemcpy(residuals + raw0, dres, (size_t)N * 8, hipMemcpyDeviceToHost) != hipSuccess ||
      hipMemcpy(jacobians + kRTangent * raw0, djac, kRTangent * (size_t)N * 8, hipMemcpyDeviceToHost) != hipSuccess)
    return MI_BA_ERR_HIP;
  return MI_BA_OK;
}
