// absolute_pose.hip — batched robust absolute pose (product code).
//
//   mi_ba_estimate_absolute_pose_batch
//       <- EstimateAbsolutePose's per-hypothesis kernel
//          (src/estimators/pose.cc:50-75) and the report handling of :126-155
//
// absolute_pose_kernel: one wavefront per problem, four problems per
// workgroup, the whole LO-RANSAC of src/optim/loransac.h:88-249 on the device.
// The waves of a workgroup share nothing: no workgroup barrier, no atomic.
//
// Prologue: the problem's pixels are normalised under its camera with the
// focal parameters scaled by its factor and staged as records (x, y, X, Y, Z)
// in the wave's share of the LDS; a problem of more than kApLdsObs
// correspondences keeps them in device memory instead.
//
// A round: lane l draws trial t0 + l with the counter-based sampler, solves
// P3P (up to four models, ascending in the root x, in registers) and scores
// each model over all correspondences in order: every lane reads the same
// record at the same time (an LDS broadcast) and keeps its own count and sum,
// so there is no cross-lane reduction and a sample model's support has the
// host build's summation order.  The round is then committed in trial order,
// model by model, uniformly across the wave: a model whose support compares
// better becomes the best and triggers the local optimisation, then the
// dynamic bound; the abort test follows every model.  Lanes past an abort are
// discarded.
//
// The local optimisation (EPnP on the inlier set, absolute_pose_block.h) is
// wave-cooperative: lane l takes the correspondences l, l + 64, ... and the
// sums go through an xor tree, after which every lane holds the same bits; the
// dense algebra between the sums runs on lane 0 over the wave's LDS
// workspace.  Every sum has a fixed order that depends on the problem alone.
//
// Built without FMA contraction: a residual has the same bits wherever the
// compiler inlines it, so the inlier set of a recursion, the inlier count of
// the best support and the final mask agree.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstring>
#include <vector>

#include "../../include/mi_ba.h"
#include "absolute_pose_block.h"
#include "ba_math.h"
#include "pose_common.h"

namespace miba {
namespace {

// Per wave: the workspace of the dense algebra and up to kApLdsObs records of
// 5 doubles (an odd stride: lanes that read different records spread over the
// banks).  4 x (544 + 5 x 896) x 8 B = 157 KiB of the 160 KiB.
constexpr int kApLdsObs = 896;
constexpr int kApWsLds = 544;
static_assert(kApWsLds >= kApWsSize, "workspace");
static_assert(kPoseWaves * (kApWsLds + kApRecord * kApLdsObs) * 8 <= 160 * 1024, "LDS budget of one workgroup");

struct ApLdsRecords {
  double* base;
  __device__ __forceinline__ double& at(int64_t i, int f) const { return base[(int)i * kApRecord + f]; }
};

struct ApProblemDev {
  int64_t begin;       // first correspondence of the set
  int64_t mask_begin;  // first mask entry
  int64_t stream;      // first record in the streamed buffer, -1: resident
  uint64_t seed;
  double factor;
  int32_t count, camera;
};

struct ApArgs {
  const ApProblemDev* prob;
  const double2* points2D;
  const double* points3D;
  const double* cam_params;  // [C][8]
  const int32_t* cam_model;  // [C]
  double* stream;            // records of the problems that are not resident
  ApResult* out;
  uint8_t* mask;
  double max_error, confidence, multiplier;
  int64_t max_num_trials, min_num_trials;
  int32_t num_listed, lds_obs;
};

__device__ __forceinline__ int ap_wave_sum_int(int v) {
#pragma unroll
  for (int off = 1; off < 64; off <<= 1) v += __shfl_xor(v, off, 64);
  return v;
}

template <typename T>
__device__ __forceinline__ T ap_pick(T a0, T a1, T a2, T a3, int m) {
  return m == 0 ? a0 : m == 1 ? a1 : m == 2 ? a2 : a3;
}

// The correspondences whose residual under `prev` is within max_residual,
// over the lanes of one wave.
template <typename Rec>
struct ApWaveSet {
  Rec rec;
  int n, lane;
  double prev[12];
  double max_residual;
  __device__ __forceinline__ bool in(int i) const { return ap_residual(rec, i, prev) <= max_residual; }
  __device__ __forceinline__ bool leader() const { return lane == 0; }
  __device__ __forceinline__ void sync() const { wave_sync(); }
  __device__ inline int64_t count() const {
    int c = 0;
#pragma unroll 1
    for (int i = lane; i < n; i += 64) c += in(i) ? 1 : 0;
    return ap_wave_sum_int(c);
  }
  template <typename F>
  __device__ inline double first(F f) const {
    int mine = INT32_MAX;
#pragma unroll 1
    for (int i = lane; i < n; i += 64)
      if (in(i)) {
        mine = i;
        break;
      }
    int lowest = mine;
#pragma unroll
    for (int off = 1; off < 64; off <<= 1) {
      const int other = __shfl_xor(lowest, off, 64);
      lowest = other < lowest ? other : lowest;
    }
    if (lowest == INT32_MAX) return 0.0;
    double v = 0.0;
    if (mine == lowest) {
      const double X[3] = {rec.at(mine, kApW), rec.at(mine, kApW + 1), rec.at(mine, kApW + 2)};
      v = f(rec.at(mine, kApX), rec.at(mine, kApY), X);
    }
    return __shfl(v, lowest & 63, 64);
  }
  template <int K, typename F>
  __device__ inline void sum(double (&out)[K], F f) const {
    double acc[K];
#pragma unroll
    for (int k = 0; k < K; ++k) acc[k] = 0.0;
#pragma unroll 1
    for (int i = lane; i < n; i += 64) {
      if (!in(i)) continue;
      const double X[3] = {rec.at(i, kApW), rec.at(i, kApW + 1), rec.at(i, kApW + 2)};
      f(rec.at(i, kApX), rec.at(i, kApY), X, acc);
    }
#pragma unroll
    for (int k = 0; k < K; ++k) out[k] = wave_sum_fixed(acc[k]);
  }
};

// The support of model P over the problem by the whole wave; the mask, if
// given, becomes the inlier set.  Every lane returns the same.
template <typename Rec>
__device__ inline void ap_wave_support(const Rec& rec, int n, int lane, const double P[12], double max_residual,
                                       uint8_t* mask, int* num_inliers, double* residual_sum) {
  int ni = 0;
  double sum = 0.0;
#pragma unroll 1
  for (int i = lane; i < n; i += 64) {
    const double r = ap_residual(rec, i, P);
    const bool in = r <= max_residual;
    if (mask) mask[i] = in ? 1 : 0;
    if (in) {
      ni += 1;
      sum += r;
    }
  }
  *num_inliers = ap_wave_sum_int(ni);
  *residual_sum = wave_sum_fixed(sum);
}

// The local optimisation on the improving model M (loransac.h:157-205), by
// the whole wave; best_* are uniform.
template <typename Rec>
__device__ inline void ap_wave_local(const Rec& rec, int n, int lane, double max_residual,
                                                        double* ws, const double M[12], int& best_n,
                                                        double& best_sum, int& best_local, double best[12]) {
  ApWaveSet<Rec> set;
  set.rec = rec;
  set.n = n;
  set.lane = lane;
  set.max_residual = max_residual;
#pragma unroll
  for (int m = 0; m < 12; ++m) set.prev[m] = M[m];
#pragma unroll 1
  for (int local = 0; local < kApMaxLocalTrials; ++local) {
    const int prev = best_n;
    double L[12];
    if (ap_epnp(set, ws, L)) {
      int ln;
      double lsum;
      ap_wave_support(rec, n, lane, L, max_residual, (uint8_t*)nullptr, &ln, &lsum);
      if (ap_better(ln, lsum, best_n, best_sum)) {
        best_n = ln;
        best_sum = lsum;
        best_local = 1;
#pragma unroll
        for (int m = 0; m < 12; ++m) best[m] = L[m];
      }
#pragma unroll
      for (int m = 0; m < 12; ++m) set.prev[m] = L[m];
    }
    if (best_n <= prev) break;
  }
}

// Trial t of the problem by one lane: up to four models and their supports.
template <typename Rec>
__device__ __forceinline__ int ap_lane_trial(const Rec& rec, int n, uint64_t seed, int64_t t,
                                                       double max_residual, double (&M)[4][12], int (&ni)[4],
                                                       double (&sum)[4]) {
  int64_t idx[3];
  ap_sample(seed, t, n, idx);
  ApP3P s;
  ap_p3p_roots(rec, idx[0], idx[1], idx[2], &s);
#pragma unroll
  for (int m = 0; m < 4; ++m) {
    if (m < s.count) {
      ap_p3p_model(s, s.x[m], M[m]);
      int64_t cnt;
      ap_support(rec, n, M[m], max_residual, &cnt, &sum[m]);
      ni[m] = (int)cnt;
    }
  }
  return s.count;
}

// One problem by one wave.
template <typename Rec>
__device__ __forceinline__ void ap_problem(const ApArgs& a, const ApProblemDev& pb, ApResult* out, const Rec& rec,
                                           double* ws, double max_residual, int lane) {
  const int n = pb.count;
  const int64_t max_trials = a.max_num_trials;
  int64_t dyn = max_trials, num_trials = max_trials;
  int best_n = 0, best_local = 0;
  double best_sum = DBL_MAX, best[12];
#pragma unroll
  for (int m = 0; m < 12; ++m) best[m] = 0.0;
  bool aborted = false;
#pragma unroll 1
  for (int64_t t0 = 0; t0 < max_trials && !aborted; t0 += 64) {
    const int64_t t = t0 + lane;
    double M[4][12], sum[4] = {0.0, 0.0, 0.0, 0.0};
    int ni[4] = {0, 0, 0, 0}, count = 0;
#pragma unroll
    for (int m = 0; m < 4; ++m) {
#pragma unroll
      for (int e = 0; e < 12; ++e) M[m][e] = 0.0;
    }
    if (t < max_trials) count = ap_lane_trial(rec, n, pb.seed, t, max_residual, M, ni, sum);
    // commit in trial order; only a trial with a model touches the state
    uint64_t models = __ballot(count > 0);
#pragma unroll 1
    while (models != 0 && !aborted) {
      const int l = __ffsll((unsigned long long)models) - 1;
      models &= models - 1;
      const int64_t tl = t0 + l;
      const int count_l = __shfl(count, l, 64);
      // The model index stays a run-time value and every access to the
      // models selects among the four with static indices, so that they stay
      // in registers (an array indexed at run time would live in scratch).
#pragma unroll 1
      for (int m = 0; m < count_l && !aborted; ++m) {
        const int ni_l = __shfl(ap_pick(ni[0], ni[1], ni[2], ni[3], m), l, 64);
        const double sum_l = __shfl(ap_pick(sum[0], sum[1], sum[2], sum[3], m), l, 64);
        if (ap_better(ni_l, sum_l, best_n, best_sum)) {
          double Ml[12];
#pragma unroll
          for (int e = 0; e < 12; ++e) Ml[e] = __shfl(ap_pick(M[0][e], M[1][e], M[2][e], M[3][e], m), l, 64);
          best_n = ni_l;
          best_sum = sum_l;
          best_local = 0;
#pragma unroll
          for (int e = 0; e < 12; ++e) best[e] = Ml[e];
          if (ni_l > 3 && ni_l >= 4) ap_wave_local(rec, n, lane, max_residual, ws, Ml, best_n, best_sum, best_local, best);
          dyn = ap_compute_num_trials(best_n, n, a.confidence, a.multiplier);
        }
        if (ap_abort(tl, dyn, a.min_num_trials)) {
          // the reference notices the abort at the top of the next trial and
          // counts that one too
          aborted = true;
          num_trials = tl + 1 < max_trials ? tl + 2 : tl + 1;
        }
      }
    }
  }

  if (best_n >= 3) {
    int ln;
    double lsum;
    ap_wave_support(rec, n, lane, best, max_residual, a.mask + pb.mask_begin, &ln, &lsum);
  }
  if (lane == 0) ap_finish(out, best, num_trials, best_n, best_local != 0);
}

__global__ __launch_bounds__(kPoseTB) void absolute_pose_kernel(ApArgs a) {
  extern __shared__ double lds[];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int slot = blockIdx.x * kPoseWaves + wave;
  if (slot >= a.num_listed) return;
  const ApProblemDev pb = a.prob[slot];
  const int n = pb.count;
  if (n < 3) return;  // loransac.h:103-105: failure, 0 trials (the outputs are zeroed)
  double* wave_lds = lds + (size_t)wave * (kApWsLds + kApRecord * a.lds_obs);
  double* ws = wave_lds;
  // EstimateAbsolutePoseKernel's preparation (pose.cc:56-72)
  double prm_in[8], prm[8];
#pragma unroll
  for (int m = 0; m < 8; ++m) prm_in[m] = a.cam_params[8 * (size_t)pb.camera + m];
  const int model = a.cam_model[pb.camera];
  const double max_residual = ap_scaled_camera(model, prm_in, pb.factor, a.max_error, prm);
  const bool resident = pb.stream < 0;
  double* dst = resident ? wave_lds + kApWsLds : a.stream + kApRecord * pb.stream;
#pragma unroll 1
  for (int i = lane; i < n; i += 64) {
    const double2 px = a.points2D[pb.begin + i];
    double u, v;
    image_to_world_all(model, prm, px.x, px.y, &u, &v);
    dst[kApRecord * i + kApX] = u;
    dst[kApRecord * i + kApY] = v;
#pragma unroll
    for (int m = 0; m < 3; ++m) dst[kApRecord * i + kApW + m] = a.points3D[3 * (pb.begin + i) + m];
  }
  __threadfence_block();
  wave_sync();
  if (resident) {
    ap_problem(a, pb, a.out + slot, ApLdsRecords{dst}, ws, max_residual, lane);
  } else {
    ap_problem(a, pb, a.out + slot, ApRecords{dst}, ws, max_residual, lane);
  }
}

// The argument checks of the batch entry point.  Host only.
mi_ba_status absolute_pose_check(const mi_ba_absolute_pose_estimation_options* o,
                                 const mi_ba_absolute_pose_estimation_batch* b) {
  if (!o || !b || b->num_problems < 0 || b->num_sets < 0 || b->num_cameras < 0) return MI_BA_ERR_INVALID_ARGUMENT;
  // RANSACOptions::Check (optim/ransac.h:68-75)
  if (!(o->max_error > 0.0) || !(o->max_error <= DBL_MAX) || !(o->min_inlier_ratio >= 0.0) ||
      !(o->min_inlier_ratio <= 1.0) || !(o->confidence >= 0.0) || !(o->confidence <= 1.0) || o->min_num_trials < 0 ||
      o->max_num_trials < 0 || o->min_num_trials > o->max_num_trials)
    return MI_BA_ERR_INVALID_ARGUMENT;
  // every device loop is bounded by max_num_trials after the constructor's cap
  if (ap_constructor_cap(o->max_num_trials, o->min_inlier_ratio, o->confidence, o->dyn_num_trials_multiplier) ==
      kApMaxTrials)
    return MI_BA_ERR_INVALID_ARGUMENT;
  const int n = b->num_problems;
  if (n == 0) return MI_BA_OK;
  if (!b->set_offsets || !b->points2D || !b->points3D || !b->camera_model_ids || !b->camera_param_offsets ||
      !b->camera_params || !b->set_index || !b->camera_index || b->set_offsets[0] < 0)
    return MI_BA_ERR_INVALID_ARGUMENT;
  for (int s = 0; s < b->num_sets; ++s) {
    const int64_t c = b->set_offsets[s + 1] - b->set_offsets[s];
    // a record's fields are indexed with int: kApRecord * count must fit
    if (c < 0 || c > INT32_MAX / kApRecord) return MI_BA_ERR_INVALID_ARGUMENT;
  }
  for (int c = 0; c < b->num_cameras; ++c) {
    const int np = num_params(b->camera_model_ids[c]);
    if (np < 0 || b->camera_param_offsets[c + 1] - b->camera_param_offsets[c] != np) return MI_BA_ERR_INVALID_ARGUMENT;
  }
  for (int k = 0; k < n; ++k) {
    if (b->set_index[k] < 0 || b->set_index[k] >= b->num_sets || b->camera_index[k] < 0 ||
        b->camera_index[k] >= b->num_cameras)
      return MI_BA_ERR_INVALID_ARGUMENT;
    if (b->focal_length_factor && (!(b->focal_length_factor[k] > 0.0) || !(b->focal_length_factor[k] <= DBL_MAX)))
      return MI_BA_ERR_INVALID_ARGUMENT;
  }
  return MI_BA_OK;
}

}  // namespace
}  // namespace miba

using namespace miba;

extern "C" void mi_ba_default_absolute_pose_estimation_options(mi_ba_absolute_pose_estimation_options* o) {
  if (!o) return;
  std::memset(o, 0, sizeof(*o));
  // RANSACOptions (optim/ransac.h:47-66)
  o->max_error = 0.0;
  o->min_inlier_ratio = 0.1;
  o->confidence = 0.99;
  o->dyn_num_trials_multiplier = 3.0;
  o->min_num_trials = 0;
  o->max_num_trials = INT64_MAX;
  o->seed = 0;
  o->device = 0;
}

extern "C" int32_t mi_ba_absolute_pose_lds_capacity(void) { return kApLdsObs; }

extern "C" mi_ba_status mi_ba_estimate_absolute_pose_batch(const mi_ba_absolute_pose_estimation_options* o,
                                                           const mi_ba_absolute_pose_estimation_batch* b,
                                                           double* proj_matrix, double* qvec, double* tvec,
                                                           uint8_t* inlier_mask, int32_t* success,
                                                           int64_t* num_trials, int32_t* num_inliers,
                                                           int32_t* best_is_local) {
  mi_ba_status st = absolute_pose_check(o, b);
  if (st != MI_BA_OK) return st;
  const int n = b->num_problems;
  if (n == 0) return MI_BA_OK;
  if (!success) return MI_BA_ERR_INVALID_ARGUMENT;
  st = pose_select_device(o->device);
  if (st != MI_BA_OK) return st;

  const int S = b->num_sets, C = b->num_cameras;
  const int64_t raw0 = b->set_offsets[0], N = b->set_offsets[S] - raw0;
  std::vector<ApProblemDev> list((size_t)n);
  int most_resident = 0;
  int64_t mask_total = 0, stream_total = 0;
  for (int k = 0; k < n; ++k) {
    const int s = b->set_index[k];
    const int64_t c = b->set_offsets[s + 1] - b->set_offsets[s];
    ApProblemDev& p = list[k];
    p.begin = b->set_offsets[s] - raw0;
    p.mask_begin = mask_total;
    p.stream = -1;
    p.seed = b->seed ? b->seed[k] : o->seed;
    p.factor = b->focal_length_factor ? b->focal_length_factor[k] : 1.0;
    p.count = (int32_t)c;
    p.camera = b->camera_index[k];
    if (c <= kApLdsObs) {
      if (c > most_resident) most_resident = (int)c;
    } else {
      p.stream = stream_total;
      stream_total += c;
    }
    mask_total += c;
  }
  // camera parameters in 8-wide slots
  std::vector<double> cam(8 * (size_t)C, 0.0);
  for (int c = 0; c < C; ++c)
    for (int64_t m = b->camera_param_offsets[c]; m < b->camera_param_offsets[c + 1]; ++m)
      cam[8 * (size_t)c + (m - b->camera_param_offsets[c])] = b->camera_params[m];

  Buf bufs[8];
  double2* d2 = bufs[0].alloc<double2>(N);
  double* d3 = bufs[1].alloc<double>(3 * (size_t)N);
  double* dcam = bufs[2].alloc<double>(cam.size());
  int32_t* dmodel = bufs[3].alloc<int32_t>(C);
  ApProblemDev* dprob = bufs[4].alloc<ApProblemDev>(list.size());
  ApResult* dout = bufs[5].alloc<ApResult>(n);
  uint8_t* dmask = bufs[6].alloc<uint8_t>(mask_total);
  double* dstream = bufs[7].alloc<double>(kApRecord * (size_t)stream_total);
  if (!d2 || !d3 || !dcam || !dmodel || !dprob || !dout || !dmask || !dstream) return MI_BA_ERR_OUT_OF_MEMORY;
  if (hipMemcpy(d2, b->points2D + 2 * raw0, (size_t)N * 16, hipMemcpyHostToDevice) != hipSuccess ||
      hipMemcpy(d3, b->points3D + 3 * raw0, (size_t)N * 24, hipMemcpyHostToDevice) != hipSuccess ||
      hipMemcpy(dcam, cam.data(), cam.size() * 8, hipMemcpyHostToDevice) != hipSuccess ||
      hipMemcpy(dmodel, b->camera_model_ids, (size_t)C * 4, hipMemcpyHostToDevice) != hipSuccess ||
      hipMemcpy(dprob, list.data(), list.size() * sizeof(ApProblemDev), hipMemcpyHostToDevice) != hipSuccess ||
      hipMemset(dmask, 0, (size_t)(mask_total ? mask_total : 8)) != hipSuccess ||
      hipMemset(dout, 0, (size_t)n * sizeof(ApResult)) != hipSuccess)
    return MI_BA_ERR_HIP;

  ApArgs a{};
  a.prob = dprob;
  a.points2D = d2;
  a.points3D = d3;
  a.cam_params = dcam;
  a.cam_model = dmodel;
  a.stream = dstream;
  a.out = dout;
  a.mask = dmask;
  a.max_error = o->max_error;
  a.confidence = o->confidence;
  a.multiplier = o->dyn_num_trials_multiplier;
  a.max_num_trials =
      ap_constructor_cap(o->max_num_trials, o->min_inlier_ratio, o->confidence, o->dyn_num_trials_multiplier);
  a.min_num_trials = o->min_num_trials;
  a.num_listed = n;
  // the arrays' stride only: a problem is resident exactly when its own count is at most kApLdsObs
  a.lds_obs = (most_resident + 1) / 2 * 2;
  const size_t bytes = (size_t)kPoseWaves * (kApWsLds + kApRecord * a.lds_obs) * 8;
  if (hipFuncSetAttribute(reinterpret_cast<const void*>(&absolute_pose_kernel),
                          hipFuncAttributeMaxDynamicSharedMemorySize, (int)bytes) != hipSuccess)
    return MI_BA_ERR_HIP;
  const unsigned groups = (unsigned)((list.size() + kPoseWaves - 1) / kPoseWaves);
  hipLaunchKernelGGL(absolute_pose_kernel, dim3(groups), dim3(kPoseTB), bytes, 0, a);
  if (hipGetLastError() != hipSuccess) return MI_BA_ERR_HIP;
  if (hipStreamSynchronize(0) != hipSuccess) return MI_BA_ERR_HIP;

  std::vector<ApResult> out((size_t)n);
  std::vector<uint8_t> hmask((size_t)mask_total);
  if (hipMemcpy(out.data(), dout, out.size() * sizeof(ApResult), hipMemcpyDeviceToHost) != hipSuccess ||
      (mask_total && hipMemcpy(hmask.data(), dmask, (size_t)mask_total, hipMemcpyDeviceToHost) != hipSuccess))
    return MI_BA_ERR_HIP;
  for (int k = 0; k < n; ++k) {
    const ApResult& r = out[k];
    success[k] = r.success;
    if (num_trials) num_trials[k] = r.num_trials;
    if (num_inliers) num_inliers[k] = r.num_inliers;
    if (best_is_local) best_is_local[k] = r.best_is_local;
    if (!r.success) continue;  // a failed problem leaves its other outputs untouched
    if (proj_matrix) std::memcpy(proj_matrix + 12 * (size_t)k, r.P, 12 * 8);
    if (qvec) std::memcpy(qvec + 4 * (size_t)k, r.qvec, 4 * 8);
    if (tvec) std::memcpy(tvec + 3 * (size_t)k, r.tvec, 3 * 8);
    if (inlier_mask) std::memcpy(inlier_mask + list[k].mask_begin, hmask.data() + list[k].mask_begin, (size_t)list[k].count);
  }
  return MI_BA_OK;
}
