// pose_common.h — what the pose-refinement kernels share.
//
// All three (pose_refine_kernel, generalized_pose_kernel, relative_pose_kernel):
// Ceres' default solver constants, the trust-region rules as functions of
// scalars, the trace byte, wave_sync / wave_sum_fixed, and the host side of an
// entry point (options check, device selection, trace buffer, summary fill).
//
// The two kernels that run one workgroup per problem with the LM state in LDS
// (pose_refine_kernel, generalized_pose_kernel) also share the wave Cholesky
// and solve over LDS rows, the triangle and tile helpers of the
// linearization, the resident-observation source, wave 0's part of the LM loop
// (PoseLmLds) and the launch.  How a camera-frame point is formed, the segment
// reduction and the in-register system of the relative kernel stay in their
// own files.
#pragma once

#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdint>
#include <vector>

#include "../../include/mi_ba.h"
#include "ba_math.h"
#include "reproj_block.h"

namespace miba {

constexpr int kPoseTB = 256;
constexpr int kPoseWaves = kPoseTB / 64;
constexpr int kColStride = 129;

// Ceres defaults RefineAbsolutePose leaves alone (solver.h).
constexpr double kFunctionTolerance = 1e-6;
constexpr double kParameterTolerance = 1e-8;
constexpr int kMaxConsecutiveInvalid = 5;
constexpr double kInitialRadius = 1e4;
constexpr double kMinRelativeDecrease = 1e-3;
constexpr double kMinRadius = 1e-32;
constexpr double kMaxRadius = 1e16;
// covariance: a pivot at or below this fraction of the column's own diagonal
// entry is rank deficiency
constexpr double kCovPivotTolerance = 1e-14;

constexpr int kOutStride = 8;  // initial cost, final cost, successful, unsuccessful, termination, covariance ok

enum { kActStop = 0, kActEval = 1, kActAccept = 2, kActReject = 3 };

__device__ __forceinline__ void wave_sync() {
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
  __builtin_amdgcn_wave_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

// xor tree: the same order on every run
__device__ __forceinline__ double wave_sum_fixed(double v) {
#pragma unroll
  for (int off = 1; off < 64; off <<= 1) v += __shfl_xor(v, off, 64);
  return v;
}

// Total of the per-thread costs in sCost (wave 0; every lane gets the sum).
__device__ inline double pose_cost_total(const double* sCost, int lane) {
  double c = sCost[lane];
#pragma unroll
  for (int w = 1; w < kPoseWaves; ++w) c += sCost[64 * w + lane];
  return wave_sum_fixed(c);
}

// trace byte of iteration it (1-based): bit 0 step valid, bit 1 successful,
// bit 2 the iteration ended the solve
__device__ __forceinline__ void pose_trace(uint8_t* trace, int cap, int index, int it, int valid, int successful,
                                           int end) {
  if (trace && it >= 1 && it <= cap) trace[(size_t)index * cap + it - 1] = (uint8_t)(valid | successful << 1 | end << 2);
}

// ---- Ceres' TrustRegionMinimizer / LevenbergMarquardtStrategy rules, on scalars ----

// Jacobi scaling of a column from its J'J diagonal entry
__device__ __forceinline__ double lm_jacobi_scale(double d) { return 1.0 / (1.0 + sqrt(d)); }

// LM diagonal: the clipped scaled column norm over the radius.  kContract: the
// sum may contract with the product that made v, as generalized_pose_kernel and
// relative_pose_kernel have always been compiled.  pose_refine_kernel's row
// build took v out of a select, which kept its sum unfused; it passes false
// and keeps those bits.
template <bool kContract = true>
__device__ __forceinline__ double lm_damped_diagonal(double v, double radius) {
  const double d = fmin(fmax(v, 1e-6), 1e32) / radius;
  if constexpr (kContract) {
    return v + d;
  } else {
#pragma clang fp contract(off)
    return v + d;
  }
}

// a non-finite candidate cost is an unsuccessful step
__device__ __forceinline__ bool lm_step_successful(double cand_cost, double relative_decrease) {
  return isfinite(cand_cost) && relative_decrease > kMinRelativeDecrease;
}

// ParameterToleranceReached / FunctionToleranceReached
__device__ __forceinline__ bool lm_tolerance_reached(double step_norm, double x_norm, double cost_change, double x_cost,
                                                     double parameter_tolerance, double function_tolerance) {
  return step_norm <= parameter_tolerance * (x_norm + parameter_tolerance) ||
         fabs(cost_change) <= function_tolerance * x_cost;
}

// StepAccepted
__device__ __forceinline__ void lm_radius_accept(double& radius, double& decrease_factor, double relative_decrease) {
  radius = fmin(kMaxRadius, radius / fmax(1.0 / 3.0, 1.0 - pow(2.0 * relative_decrease - 1.0, 3.0)));
  decrease_factor = 2.0;
}

// StepRejected / StepIsInvalid
__device__ __forceinline__ void lm_radius_reject(double& radius, double& decrease_factor) {
  radius = radius / decrease_factor;
  decrease_factor = decrease_factor * 2.0;
}

// ---- one workgroup per problem: the linearization's helpers ----

// The lane's entries (i, j), i <= j < NC, of the upper triangle of [J r]'[J r].
template <int NC, int EPL>
__device__ __forceinline__ void pose_triangle_entries(int lane, int (&ei)[EPL], int (&ej)[EPL]) {
  constexpr int NE = NC * (NC + 1) / 2;
  static_assert(EPL == (NE + 63) / 64, "entries per lane");
#pragma unroll
  for (int s = 0; s < EPL; ++s) {
    int e = lane + 64 * s, i = 0, w = NC;
    if (e >= NE) e = 0;  // idle slot: sums entry 0, never stored
    while (e >= w) { e -= w; --w; ++i; }
    ei[s] = i;
    ej[s] = i + e;
  }
}

// One tile of 64 observations: the lane's two rows go into the wave's slab as
// columns, then the lane adds the 128 products of each of its entries to acc.
template <int NC, int EPL>
__device__ __forceinline__ void pose_tile_products(double* slab, int lane, const double (&J0)[NC],
                                                   const double (&J1)[NC], const int (&ei)[EPL],
                                                   const int (&ej)[EPL], double (&acc)[EPL]) {
#pragma unroll
  for (int c = 0; c < NC; ++c) {
    slab[c * kColStride + lane] = J0[c];
    slab[c * kColStride + 64 + lane] = J1[c];
  }
  wave_sync();
#pragma unroll
  for (int s = 0; s < EPL; ++s) {
    const double* ci = slab + ei[s] * kColStride;
    const double* cj = slab + ej[s] * kColStride;
    double v = acc[s];
#pragma unroll 4
    for (int k = 0; k < 128; ++k) v += ci[k] * cj[k];
    acc[s] = v;
  }
  wave_sync();
}

// Correspondences (pixel, 3D point) of one problem: a struct of arrays in LDS
// when the problem fits, device memory otherwise.  kOrdered: correspondence i
// is number order[i] of the device arrays.
template <bool kOrdered>
struct PoseObsSource {
  double* sx;            // LDS, SoA (resident) ...
  const int32_t* order;  // ... or device memory
  const double2* p2;
  const double* p3;
  bool resident;
  int lds_obs;
  __device__ __forceinline__ size_t at(int i) const {
    if constexpr (kOrdered) return (size_t)order[i];
    else return (size_t)i;
  }
  __device__ __forceinline__ void fetch(int i, double* ox, double* oy, double X[3]) const {
    const size_t j = at(i);
    const double2 o = p2[j];
    *ox = o.x;
    *oy = o.y;
    X[0] = p3[3 * j];
    X[1] = p3[3 * j + 1];
    X[2] = p3[3 * j + 2];
  }
  // the whole workgroup, before a barrier
  __device__ __forceinline__ void stage(int tid, int count) const {
    if (!resident) return;
    for (int i = tid; i < count; i += kPoseTB) {
      double X[3];
      fetch(i, &sx[i], &sx[lds_obs + i], X);
      sx[2 * lds_obs + i] = X[0];
      sx[3 * lds_obs + i] = X[1];
      sx[4 * lds_obs + i] = X[2];
    }
  }
  __device__ __forceinline__ void load(int i, double* ox, double* oy, double X[3]) const {
    if (resident) {
      *ox = sx[i];
      *oy = sx[lds_obs + i];
      X[0] = sx[2 * lds_obs + i];
      X[1] = sx[3 * lds_obs + i];
      X[2] = sx[4 * lds_obs + i];
    } else {
      fetch(i, ox, oy, X);
    }
  }
};

// ---- one workgroup per problem: wave 0's solve ----

// Dense Cholesky by one wave, in LDS: lane i < n owns row i of the lower
// triangle in sA (row stride S); on return sA holds L.  A pivot k with
// !(pivot > tol * d0[k]) makes the result false.  Column k reaches the other
// rows through LDS.
template <int S>
__device__ inline bool wave_cholesky(double* sA, int n, int lane, double tol, const double* d0) {
  bool ok = true;
#pragma unroll 1
  for (int k = 0; k < n; ++k) {
    wave_sync();
    const double akk = sA[k * S + k];
    if (!(akk > tol * d0[k])) ok = false;
    const double lkk = sqrt(akk);
    const bool mine = lane < n && lane >= k;
    double lik = 0.0;
    if (mine) lik = lane == k ? lkk : sA[lane * S + k] / lkk;
    wave_sync();
    if (mine) sA[lane * S + k] = lik;
    wave_sync();
    if (mine)
      for (int j = k + 1; j <= lane; ++j) sA[lane * S + j] -= lik * sA[j * S + k];
  }
  wave_sync();
  return ok;
}

// Solves L L' x = b with L in sA: lane i < n passes b_i and receives x_i; sx
// (n doubles of LDS) carries each solved component to the other lanes.
template <int S>
__device__ inline double wave_chol_solve(const double* sA, int n, double b, int lane, double* sx) {
#pragma unroll 1
  for (int k = 0; k < n; ++k) {
    if (lane == k) sx[k] = b / sA[k * S + k];
    wave_sync();
    const double yk = sx[k];
    if (lane == k) b = yk;
    else if (lane > k && lane < n) b -= sA[lane * S + k] * yk;
  }
#pragma unroll 1
  for (int k = n - 1; k >= 0; --k) {
    if (lane == k) sx[k] = b / sA[k * S + k];
    wave_sync();
    const double xk = sx[k];
    if (lane == k) b = xk;
    else if (lane < k) b -= sA[k * S + lane] * xk;
  }
  wave_sync();
  return b;
}

// The lane index again, opaque to the compiler.  Wave 0's blocks below address
// LDS rows by lane; left visible, those loop-invariant addresses are hoisted
// out of the LM loop and stay in registers across the observation passes,
// where the kernels have none to spare.
__device__ __forceinline__ int wave0_lane(int lane) {
  asm volatile("" : "+v"(lane));
  return lane;
}

// LM state of one problem, in LDS: read and written by wave 0 only, so no
// register holds it across the observation passes.
struct PoseLm {
  double x_cost, initial_cost, radius, decrease_factor;
  double model_cost_change, x_norm, step_norm, pad;
  int iteration, consecutive_invalid, n_successful, n_unsuccessful;
  int termination, last_successful, action0, action1;
};

// What the kernel's arguments say about the solve.
struct PoseLmOptions {
  double gradient_tolerance;
  int32_t max_num_iterations;
  uint8_t* trace;  // nullable [n][trace_cap]: outcome of each LM iteration (mi_ba_pose_refine_set_trace)
  int32_t trace_cap;
  int32_t index;   // the problem's row of trace / out / cov
};

// Wave 0's part of the LM loop over the problem's LDS.  sM is the symmetric
// [J r]'[J r] with NC columns, r the last; sA the system / factor with row
// stride S; sScale, sStep and sD0 have W entries.  Lane i owns row i of the
// n <= min(NC - 1, W) active rows.  The state is q(4) t(3), then whatever the
// kernel keeps; tangent column m >= 6 belongs to state slot sTan[m].
// kContractDiag: see lm_damped_diagonal.
template <int NC, int S, int W, bool kContractDiag>
struct PoseLmLds {
  static constexpr int NTG = NC - 1;
  double *sM, *sA, *sScale, *sStep, *sD0;
  PoseLm* lm;
  const int* sTan;

  static __device__ __forceinline__ bool in_w(int lane) { return W >= 64 || lane < W; }

  __device__ __forceinline__ void init(int tid) const {
    if (tid != 0) return;
    lm->radius = kInitialRadius;
    lm->decrease_factor = 2.0;
    lm->iteration = 0;
    lm->consecutive_invalid = 0;
    lm->n_successful = 0;
    lm->n_unsuccessful = 0;
    lm->termination = MI_BA_NO_CONVERGENCE;
    lm->last_successful = 1;  // iteration 0 counts as successful (IterationZero)
  }

  // after the first linearization: Jacobi scaling and the initial cost
  __device__ __forceinline__ void first(int n, int lane, double total) const {
    if (in_w(lane)) sScale[lane] = lane < n ? lm_jacobi_scale(sM[lane * NC + lane]) : 1.0;
    if (lane == 0) {
      lm->x_cost = total;
      lm->initial_cost = total;
    }
    wave_sync();
  }

  // From the linearization in sM to a candidate: the exit tests, the scaled
  // and damped system, factor, solve and model cost change (an invalid step
  // shrinks the radius and tries again), then sCand = Plus(sState, step) over
  // ncopy state slots.  False: the solve ended, lm->termination says how.
  __device__ __forceinline__ bool propose(const double* sState, double* sCand, int ncopy, int n, int lane,
                                          const PoseLmOptions& o, double* model_cost_change) const {
    lane = wave0_lane(lane);
    // a non-finite initial cost: FAILURE, parameters untouched
    const bool go = isfinite(lm->x_cost);
    if (!go && lane == 0) lm->termination = MI_BA_FAILURE;
    while (go) {
      // FinalizeIterationAndCheckIfMinimizerCanContinue
      if (lm->iteration >= o.max_num_iterations) {
        if (lane == 0) lm->termination = MI_BA_NO_CONVERGENCE;
        break;
      }
      if (lm->last_successful) {
        // GradientToleranceReached: |x - Plus(x, -g)|_inf, g = J'r
        const double d[3] = {-sM[0 * NC + NTG], -sM[1 * NC + NTG], -sM[2 * NC + NTG]};
        const double q[4] = {sState[0], sState[1], sState[2], sState[3]};
        double qn[4], gmax = 0.0;
        quat_plus(q, d, qn);
#pragma unroll
        for (int m = 0; m < 4; ++m) gmax = fmax(gmax, fabs(q[m] - qn[m]));
        for (int m = 0; m < 3; ++m) gmax = fmax(gmax, fabs(sState[4 + m] - (sState[4 + m] + -sM[(3 + m) * NC + NTG])));
        for (int m = 6; m < n; ++m) {
          const double xv = sState[sTan[m]];
          gmax = fmax(gmax, fabs(xv - (xv + -sM[m * NC + NTG])));
        }
        if (gmax <= o.gradient_tolerance) {
          if (lane == 0) lm->termination = MI_BA_CONVERGENCE;
          break;
        }
      }
      const double radius = lm->radius;
      if (radius <= kMinRadius) {
        if (lane == 0) lm->termination = MI_BA_CONVERGENCE;
        break;
      }
      wave_sync();
      if (lane == 0) lm->iteration += 1;
      // row `lane` of the scaled, damped system
      const double scale = in_w(lane) ? sScale[lane] : 1.0;
      double gs = 0.0;
      if (lane < n) {
        for (int j = 0; j <= lane; ++j) {
          double v = sM[lane * NC + j] * scale * sScale[j];
          if (j == lane) v = lm_damped_diagonal<kContractDiag>(v, radius);
          sA[lane * S + j] = v;
        }
        sD0[lane] = 1.0;
        gs = sM[lane * NC + NTG] * scale;
      }
      bool ok = wave_cholesky<S>(sA, n, lane, 0.0, sD0);
      double step = 0.0, model = 0.0;
      if (ok) {
        // Ceres solves (J'J + D'D) x = J'r, step = -x
        step = -wave_chol_solve<S>(sA, n, gs, lane, sStep);
        if (in_w(lane)) sStep[lane] = lane < n ? step : 0.0;
        wave_sync();
        double term = 0.0;
        if (lane < n) {
          double hstep = 0.0;
          for (int j = 0; j < n; ++j) hstep += sM[lane * NC + j] * scale * sScale[j] * sStep[j];
          // gs + 0.5 * hstep, fused as both kernels have always been compiled
          term = step * fma(0.5, hstep, gs);
        }
        model = -wave_sum_fixed(term);
        ok = isfinite(model) && model > 0.0;
      }
      if (!ok) {
        const int inv = lm->consecutive_invalid + 1;
        wave_sync();
        if (lane == 0) {
          lm->last_successful = 0;
          lm->consecutive_invalid = inv;
          lm->n_unsuccessful += 1;
          lm_radius_reject(lm->radius, lm->decrease_factor);
          if (inv > kMaxConsecutiveInvalid) lm->termination = MI_BA_FAILURE;
          pose_trace(o.trace, o.trace_cap, o.index, lm->iteration, 0, 0, inv > kMaxConsecutiveInvalid ? 1 : 0);
        }
        wave_sync();
        if (inv > kMaxConsecutiveInvalid) break;
        continue;
      }
      // candidate = Plus(x, step * scale)
      const double delta = step * scale;
      for (int m = lane; m < ncopy; m += 64) sCand[m] = sState[m];
      if (in_w(lane)) sStep[lane] = lane < n ? delta : 0.0;
      wave_sync();
      const double dq[3] = {sStep[0], sStep[1], sStep[2]};
      const double q[4] = {sState[0], sState[1], sState[2], sState[3]};
      double qn[4];
      quat_plus(q, dq, qn);
      if (lane < 4) sCand[lane] = lane == 0 ? qn[0] : lane == 1 ? qn[1] : lane == 2 ? qn[2] : qn[3];
      if (lane >= 3 && lane < 6) sCand[1 + lane] = sState[1 + lane] + delta;
      if (lane >= 6 && lane < n) sCand[sTan[lane]] = sState[sTan[lane]] + delta;
      wave_sync();
      *model_cost_change = model;
      return true;
    }
    return false;
  }

  // the candidate's model cost change, |x|^2 and |x - candidate|^2
  __device__ __forceinline__ void candidate_ready(int lane, double model_cost_change, double xn2, double sn2) const {
    if (lane != 0) return;
    lm->consecutive_invalid = 0;
    lm->model_cost_change = model_cost_change;
    lm->x_norm = sqrt(xn2);
    lm->step_norm = sqrt(sn2);
  }

  // The candidate's per-thread costs are in sCost: converged (kActStop),
  // accepted (kActAccept: the caller copies the candidate into the state) or
  // rejected (kActReject).
  __device__ __forceinline__ int judge(const double* sCost, int lane, const PoseLmOptions& o) const {
    const double cand_cost = pose_cost_total(sCost, lane);
    const double x_cost = lm->x_cost;
    const double cost_change = x_cost - cand_cost;
    const double relative_decrease = cost_change / lm->model_cost_change;
    const bool success = lm_step_successful(cand_cost, relative_decrease);
    // Ceres returns before accepting the candidate
    const bool tol = lm_tolerance_reached(lm->step_norm, lm->x_norm, cost_change, x_cost, kParameterTolerance,
                                          kFunctionTolerance);
    wave_sync();
    const int action = tol ? kActStop : success ? kActAccept : kActReject;
    if (lane == 0) {
      lm->action1 = action;
      if (tol) {
        lm->n_unsuccessful += 1;
        lm->termination = MI_BA_CONVERGENCE;
      } else if (success) {
        lm->n_successful += 1;
        lm->last_successful = 1;
        lm->x_cost = cand_cost;
        lm_radius_accept(lm->radius, lm->decrease_factor, relative_decrease);
      } else {
        lm->n_unsuccessful += 1;
        lm->last_successful = 0;
        lm_radius_reject(lm->radius, lm->decrease_factor);
      }
      pose_trace(o.trace, o.trace_cap, o.index, lm->iteration, 1, success && !tol, tol);
    }
    return action;
  }

  // After the loop: the pose block of inv(J'J) at the final point (sM) into
  // cov (nullable, [n][36]) and the problem's row of out.
  __device__ __forceinline__ void finish(int n, int lane, double* cov, double* out, int index) const {
    lane = wave0_lane(lane);
    const int termination = lm->termination;
    double cov_ok = 0.0;
    if (cov && termination != MI_BA_FAILURE) {
      if (lane < n) {
        for (int j = 0; j <= lane; ++j) sA[lane * S + j] = sM[lane * NC + j];
        sD0[lane] = sM[lane * NC + lane];
      }
      if (wave_cholesky<S>(sA, n, lane, kCovPivotTolerance, sD0)) {
        cov_ok = 1.0;
        cov += (size_t)index * 36;
#pragma unroll 1
        for (int c = 0; c < 6; ++c) {
          const double x = wave_chol_solve<S>(sA, n, lane == c ? 1.0 : 0.0, lane, sStep);
          if (lane < 6) cov[lane * 6 + c] = x;
        }
      }
    }
    if (lane == 0) {
      out += (size_t)index * kOutStride;
      out[0] = lm->initial_cost;
      out[1] = lm->x_cost;
      out[2] = lm->n_successful;
      out[3] = lm->n_unsuccessful;
      out[4] = termination;
      out[5] = cov_ok;
    }
  }
};

// ---- host side of an entry point ----

struct Buf {
  void* p = nullptr;
  ~Buf() {
    if (p) (void)hipFree(p);
  }
  template <typename T>
  T* alloc(size_t n) {
    if (hipMalloc(&p, n == 0 ? 8 : n * sizeof(T)) != hipSuccess) p = nullptr;
    return static_cast<T*>(p);
  }
};

// The buffer of mi_ba_pose_refine_set_trace (pose_refine.hip).
void pose_trace_target(uint8_t** trace, int32_t* capacity);

// AbsolutePoseRefinementOptions::Check (pose.h:119-123); the relative entry
// points add Ceres' two other tolerances.
inline bool pose_options_check(double gradient_tolerance, int32_t max_num_iterations, double loss_function_scale,
                               double function_tolerance = 0.0, double parameter_tolerance = 0.0) {
  return gradient_tolerance >= 0.0 && max_num_iterations >= 0 && loss_function_scale >= 0.0 &&
         function_tolerance >= 0.0 && parameter_tolerance >= 0.0;
}

inline mi_ba_status pose_select_device(int device) {
  int ndev = 0;
  if (hipGetDeviceCount(&ndev) != hipSuccess || ndev == 0) return MI_BA_ERR_NO_DEVICE;
  if (device < 0 || device >= ndev) return MI_BA_ERR_INVALID_ARGUMENT;
  return hipSetDevice(device) == hipSuccess ? MI_BA_OK : MI_BA_ERR_HIP;
}

// q / |q|; a unit quaternion is kept bit for bit (BundleAdjuster::SetUp normalises)
inline void pose_unit_quat_copy(const double* q, double* dst) {
  const double nq = std::sqrt(q[0] * q[0] + q[1] * q[1] + q[2] * q[2] + q[3] * q[3]);
  const bool unit = quat_is_unit(q);
  for (int m = 0; m < 4; ++m) dst[m] = unit ? q[m] : q[m] / nq;
}

// The device copy of the caller's trace buffer, if one is set: every byte
// 0xFF until an iteration writes it.
struct PoseTraceBuf {
  uint8_t* host = nullptr;
  uint8_t* dev = nullptr;
  int32_t cap = 0;
  size_t bytes = 0;
  Buf buf;
  mi_ba_status setup(int n) {
    pose_trace_target(&host, &cap);
    if (!host) return MI_BA_OK;
    bytes = (size_t)n * cap;
    dev = buf.alloc<uint8_t>(bytes);
    if (!dev) return MI_BA_ERR_OUT_OF_MEMORY;
    return hipMemset(dev, 0xFF, bytes) == hipSuccess ? MI_BA_OK : MI_BA_ERR_HIP;
  }
  mi_ba_status download() const {
    return !host || hipMemcpy(host, dev, bytes, hipMemcpyDeviceToHost) == hipSuccess ? MI_BA_OK : MI_BA_ERR_HIP;
  }
};

inline bool pose_download(std::vector<double>* host, const double* dev) {
  return hipMemcpy(host->data(), dev, host->size() * 8, hipMemcpyDeviceToHost) == hipSuccess;
}

// Fills the summary from the problem's row of out; true when the solve left
// usable parameters (Ceres leaves the user's parameter blocks untouched on
// FAILURE).
inline bool pose_summary_fill(const double* r, mi_ba_summary* s) {
  s->initial_cost = r[0];
  s->final_cost = r[1];
  s->num_successful_steps = (int32_t)r[2];
  s->num_unsuccessful_steps = (int32_t)r[3];
  s->termination_type = (int32_t)r[4];
  s->num_jacobian_evaluations = 1 + s->num_successful_steps;
  s->num_linear_solver_iterations = s->num_successful_steps + s->num_unsuccessful_steps;
  return s->termination_type == MI_BA_CONVERGENCE || s->termination_type == MI_BA_NO_CONVERGENCE ||
         s->termination_type == MI_BA_USER_SUCCESS;
}

// One workgroup per listed problem.  The LDS holds the launch's largest
// problem, up to lds_cap observations; lds_doubles gives its size.
template <typename Args, typename Problem>
mi_ba_status pose_launch(void (*kernel)(Args), int (*lds_doubles)(int), int lds_cap, Args a,
                         const std::vector<Problem>& list, Buf* buf) {
  if (list.empty()) return MI_BA_OK;
  int most = 0;
  for (const Problem& pb : list) most = pb.count > most ? pb.count : most;
  a.lds_obs = most > lds_cap ? lds_cap : (most + 63) / 64 * 64;
  Problem* d = buf->alloc<Problem>(list.size());
  if (!d) return MI_BA_ERR_OUT_OF_MEMORY;
  if (hipMemcpy(d, list.data(), list.size() * sizeof(Problem), hipMemcpyHostToDevice) != hipSuccess)
    return MI_BA_ERR_HIP;
  a.prob = d;
  const size_t bytes = (size_t)lds_doubles(a.lds_obs) * 8;
  if (hipFuncSetAttribute(reinterpret_cast<const void*>(kernel), hipFuncAttributeMaxDynamicSharedMemorySize,
                          (int)bytes) != hipSuccess)
    return MI_BA_ERR_HIP;
  hipLaunchKernelGGL(kernel, dim3((unsigned)list.size()), dim3(kPoseTB), bytes, 0, a);
  return hipGetLastError() == hipSuccess ? MI_BA_OK : MI_BA_ERR_HIP;
}

}  // namespace miba
