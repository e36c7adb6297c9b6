// pose_common.h — what the two pose-refinement kernels share: Ceres' default
// solver constants, the wave helpers, the LM state record and the device
// buffer holder.  pose_refine_kernel (pose_refine.hip) and
// generalized_pose_kernel (generalized_pose.hip) include it; the arithmetic of
// either is its own.
#pragma once

#include <hip/hip_runtime.h>

#include <cstdint>

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

// LM state of one problem, in LDS: read and written by wave 0 only, so no
// register holds it across the observation passes.
struct PoseLm {
  double x_cost, initial_cost, radius, decrease_factor;
  double model_cost_change, x_norm, step_norm, pad;
  int iteration, consecutive_invalid, n_successful, n_unsuccessful;
  int termination, last_successful, action0, action1;
};

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

}  // namespace miba
