// triangulation.hip — batched robust triangulation of tracks (product code).
//
//   mi_ba_estimate_triangulation_batch
//       <- EstimateTriangulation (src/estimators/triangulation.cc:132-160)
//   mi_ba_triangulate_points
//       <- TriangulatePoints, CalculateTriangulationAngles
//          (src/base/triangulation.cc:55-70, 147-181)
//
// triangulation_kernel: one wavefront per track, four tracks per workgroup,
// the whole LO-RANSAC of src/optim/loransac.h:88-249 on the device.  The waves
// of a workgroup share nothing: no workgroup barrier, no atomic.
//
// The sampler is CombinationSampler, which draws the pairs in lexicographic
// order without a random number, and a trial's model and support do not depend
// on the best-so-far state.  So a round evaluates 64 trials at once, lane l
// trial t0 + l: the two-view Estimate and, if it yields a model, the support
// over all observations, summed in observation order by that lane.  The round
// is then committed in trial order, uniformly across the wave: a lane whose
// support compares better becomes the best and triggers the local
// optimisation, which the wave runs cooperatively (lane l takes the
// observations l, l + 64, ...; sums go through an xor tree, after which every
// lane holds the same bits); then the dynamic bound and the abort test.
// Lanes past an abort are discarded.  Every sum has a fixed order that depends
// on the track alone.
//
// LORANSAC caps max_num_trials by the sampler's C(n, 2) (loransac.h:126-127),
// so the sampler never wraps; the wrap is not implemented.
//
// A record per observation (triangulation_block.h: projection matrix, centre,
// point_normalized, its unit ray, the pixel, the camera index) is built by
// triangulation_records_kernel, one lane per observation.  A track of up to
// kTriLdsObs observations keeps its records in the wave's quarter of the LDS
// (padded to 25 doubles, so lanes that read different observations spread over
// the banks); a longer one streams them from device memory.
//
// Built without FMA contraction: a residual then has the same bits wherever
// the compiler inlines it, so the inlier count of the best support and the
// mask computed from the best model at the end agree.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstring>
#include <vector>

#include "../../include/mi_ba.h"
#include "ba_math.h"
#include "pose_common.h"
#include "triangulation_block.h"

namespace miba {
namespace {

// 4 waves x 128 observations x 25 doubles x 8 B = 100 KiB of the 160 KiB; a
// launch sizes the arrays by its longest resident track.
constexpr int kTriLdsObs = 128;
constexpr int kTriLdsStride = kTriRecord + 1;
constexpr int kTriMaxLocalTrials = 10;  // loransac.h:160
static_assert(kPoseWaves * kTriLdsStride * kTriLdsObs * 8 <= 160 * 1024, "LDS budget of one workgroup");

struct TriLdsRecords {
  double* base;
  __device__ __forceinline__ double& at(int64_t i, int f) const { return base[(int)i * kTriLdsStride + f]; }
};

struct TriProblemDev {
  int64_t begin;       // first observation
  int64_t min_trials;  // RANSACOptions::min_num_trials of this track
  int32_t count, index;
};

struct TriArgs {
  const TriProblemDev* prob;
  double* rec;  // [N][kTriRecord]; field kTriFlag is the kernel's scratch
  TriCameras cams;
  TriOptions opt;
  TriResult* out;  // [n]; xyz is written on success only
  uint8_t* mask;   // [N]
  int32_t num_listed;
  int32_t lds_obs;
};

struct TriRecordArgs {
  const int32_t* view_index;
  const double2* points;             // nullable
  const double2* points_normalized;  // nullable
  const double* proj;                // [V][12]
  const double* centers;             // [V][3]
  const int32_t* view_cam;           // [V]
  TriCameras cams;
  double* rec;
  int64_t n;
};

__global__ __launch_bounds__(256) void triangulation_records_kernel(TriRecordArgs a) {
  const int64_t k = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (k >= a.n) return;
  const int view = a.view_index[k];
  const int cam = a.view_cam[view];
  double2 px = make_double2(0.0, 0.0), pn;
  if (a.points) px = a.points[k];
  if (a.points_normalized) {
    pn = a.points_normalized[k];
  } else {
    double prm[8];
#pragma unroll
    for (int m = 0; m < 8; ++m) prm[m] = a.cams.params[8 * (size_t)cam + m];
    image_to_world_all(a.cams.model[cam], prm, px.x, px.y, &pn.x, &pn.y);
  }
  tri_fill_record(a.rec + kTriRecord * k, a.proj + 12 * (size_t)view, a.centers + 3 * (size_t)view, px.x, px.y, pn.x,
                  pn.y, cam);
}

__device__ __forceinline__ int wave_sum_int(int v) {
#pragma unroll
  for (int off = 1; off < 64; off <<= 1) v += __shfl_xor(v, off, 64);
  return v;
}

// TriangulationEstimator::Estimate on the flagged observations
// (triangulation.cc:75-106) by the whole wave; every lane returns the same.
template <typename Rec>
__device__ inline bool tri_wave_estimate_flagged(const TriOptions& o, const Rec& rec, int n, int lane,
                                                 double X[3]) {
  double S[10];
#pragma unroll
  for (int e = 0; e < 10; ++e) S[e] = 0.0;
#pragma unroll 1
  for (int i = lane; i < n; i += 64) {
    if (rec.at(i, kTriFlag) == 0.0) continue;
    double P[12], ray[3];
#pragma unroll
    for (int m = 0; m < 12; ++m) P[m] = rec.at(i, kTriP + m);
#pragma unroll
    for (int m = 0; m < 3; ++m) ray[m] = rec.at(i, kTriRay + m);
    tri_multiview_accumulate(P, ray, S);
  }
#pragma unroll
  for (int e = 0; e < 10; ++e) S[e] = wave_sum_fixed(S[e]);
  tri_multiview_solve(S, X);
  // every cheirality
  bool behind = false;
#pragma unroll 1
  for (int i = lane; i < n; i += 64) {
    if (rec.at(i, kTriFlag) == 0.0) continue;
    double P[12];
#pragma unroll
    for (int m = 0; m < 12; ++m) P[m] = rec.at(i, kTriP + m);
    if (!tri_positive_depth(P, X)) behind = true;
  }
  if (__ballot(behind) != 0) return false;
  // any pair (i, j < i) with a sufficient angle: the order of the search does
  // not matter to the answer
#pragma unroll 1
  for (int i0 = 0; i0 < n; i0 += 64) {
    const int i = i0 + lane;
    bool found = false;
    if (i < n && rec.at(i, kTriFlag) != 0.0) {
      const double ci[3] = {rec.at(i, kTriCenter), rec.at(i, kTriCenter + 1), rec.at(i, kTriCenter + 2)};
#pragma unroll 1
      for (int j = 0; j < i && !found; ++j) {
        if (rec.at(j, kTriFlag) == 0.0) continue;
        const double cj[3] = {rec.at(j, kTriCenter), rec.at(j, kTriCenter + 1), rec.at(j, kTriCenter + 2)};
        found = tri_angle(ci, cj, X) >= o.min_tri_angle;
      }
    }
    if (__ballot(found) != 0) return true;
  }
  return false;
}

// The residuals of model X over the track by the whole wave: the flags (and
// mask, if given) become the inlier set, the support comes back in every lane.
template <typename Rec>
__device__ inline void tri_wave_support(const TriOptions& o, const Rec& rec, int n, int lane, const double X[3],
                                        const TriCameras& cams, uint8_t* mask, int* num_inliers,
                                        double* residual_sum) {
  int ni = 0;
  double sum = 0.0;
#pragma unroll 1
  for (int i = lane; i < n; i += 64) {
    const double r = tri_residual(o.residual_type, rec, i, X, cams);
    const bool in = r <= o.max_residual;
    rec.at(i, kTriFlag) = in ? 1.0 : 0.0;
    if (mask) mask[i] = in ? 1 : 0;
    if (in) {
      ni += 1;
      sum += r;
    }
  }
  *num_inliers = wave_sum_int(ni);
  *residual_sum = wave_sum_fixed(sum);
  wave_sync();
}

// One track by one wave.
template <typename Rec>
__device__ __forceinline__ void tri_track(const TriArgs& a, const TriProblemDev& pb, const Rec& rec, int lane) {
  const int n = pb.count;
  const TriOptions o = a.opt;
  const int64_t pairs = (int64_t)n * (n - 1) / 2;
  const int64_t max_trials = o.max_num_trials < pairs ? o.max_num_trials : pairs;
  int64_t dyn = max_trials, num_trials = max_trials;
  int best_n = 0, best_local = 0;
  double best_sum = DBL_MAX, best[3] = {0.0, 0.0, 0.0};
  bool aborted = false;
#pragma unroll 1
  for (int64_t t0 = 0; t0 < max_trials && !aborted; t0 += 64) {
    // speculate: lane l evaluates trial t0 + l
    const int64_t t = t0 + lane;
    bool has = false;
    double X[3] = {0.0, 0.0, 0.0}, sum = 0.0;
    int ni = 0;
    if (t < max_trials) {
      int64_t i, j, cnt;
      tri_unrank_pair(t, n, &i, &j);
      has = tri_estimate_two(o, rec, i, j, X);
      if (has) {
        tri_support(o, rec, n, X, a.cams, &cnt, &sum);
        ni = (int)cnt;
      }
    }
    // commit in trial order; only a trial with a model touches the state
    uint64_t models = __ballot(has);
#pragma unroll 1
    while (models != 0) {
      const int l = __ffsll((unsigned long long)models) - 1;
      models &= models - 1;
      const int64_t tl = t0 + l;
      const int ni_l = __shfl(ni, l, 64);
      const double sum_l = __shfl(sum, l, 64);
      if (tri_better(ni_l, sum_l, best_n, best_sum)) {
        double M[3];
#pragma unroll
        for (int m = 0; m < 3; ++m) M[m] = __shfl(X[m], l, 64);
        best_n = ni_l;
        best_sum = sum_l;
        best_local = 0;
#pragma unroll
        for (int m = 0; m < 3; ++m) best[m] = M[m];
        if (ni_l > 2) {
          // Local optimisation.  Pass 0 turns the sample model's residuals
          // into the flags; pass k >= 1 evaluates the k-th local model, which
          // Estimate made from the flags of the model evaluated before it (see
          // tri_loransac for the trace of the reference's residual-buffer
          // swaps).
          int prev = best_n;
#pragma unroll 1
          for (int local = 0; local <= kTriMaxLocalTrials; ++local) {
            int ln;
            double lsum;
            tri_wave_support(o, rec, n, lane, M, a.cams, (uint8_t*)nullptr, &ln, &lsum);
            if (local > 0) {
              if (tri_better(ln, lsum, best_n, best_sum)) {
                best_n = ln;
                best_sum = lsum;
                best_local = 1;
#pragma unroll
                for (int m = 0; m < 3; ++m) best[m] = M[m];
              }
              if (best_n <= prev) break;
            }
            if (local == kTriMaxLocalTrials) break;
            prev = best_n;
            if (!tri_wave_estimate_flagged(o, rec, n, lane, M)) break;
          }
        }
        dyn = tri_compute_num_trials(best_n, n, o.confidence, o.dyn_num_trials_multiplier);
      }
      if (tl >= dyn && tl >= pb.min_trials) {
        // the reference notices the abort at the top of the next trial and
        // counts that one too
        aborted = true;
        num_trials = tl + 1 < max_trials ? tl + 2 : tl + 1;
        break;
      }
    }
  }

  const bool success = best_n >= 2;
  if (success) {
    // the mask from the best model's residuals, computed again
    int ln;
    double lsum;
    tri_wave_support(o, rec, n, lane, best, a.cams, a.mask + pb.begin, &ln, &lsum);
  }
  if (lane != 0) return;
  TriResult* out = a.out + pb.index;
  out->success = success ? 1 : 0;
  out->num_trials = num_trials;
  out->num_inliers = best_n;
  out->best_is_local = best_local;
  if (success) {
#pragma unroll
    for (int m = 0; m < 3; ++m) out->xyz[m] = best[m];
  }
}

__global__ __launch_bounds__(kPoseTB) void triangulation_kernel(TriArgs a) {
  extern __shared__ double lds[];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int slot = blockIdx.x * kPoseWaves + wave;
  if (slot >= a.num_listed) return;
  const TriProblemDev pb = a.prob[slot];
  const int n = pb.count;
  double* grec = a.rec + kTriRecord * pb.begin;
  if (n <= a.lds_obs) {
    double* sObs = lds + (size_t)wave * kTriLdsStride * a.lds_obs;
    for (int e = lane; e < n * kTriRecord; e += 64) {
      const int i = e / kTriRecord, f = e - i * kTriRecord;
      sObs[i * kTriLdsStride + f] = grec[e];
    }
    wave_sync();
    tri_track(a, pb, TriLdsRecords{sObs}, lane);
  } else {
    tri_track(a, pb, TriRecords{grec}, lane);
  }
}

struct TriPointsArgs {
  double P1[12], P2[12], c1[3], c2[3];
  const double2* p1;
  const double2* p2;
  double* xyz;
  double* angles;
  int64_t m;
  int32_t triangulate, with_angles;
};

__global__ __launch_bounds__(256) void triangulate_points_kernel(TriPointsArgs a) {
  const int64_t k = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (k >= a.m) return;
  double X[3];
  if (a.triangulate) {
    const double2 u = a.p1[k], v = a.p2[k];
    tri_triangulate_point(a.P1, a.P2, u.x, u.y, v.x, v.y, X);
#pragma unroll
    for (int m = 0; m < 3; ++m) a.xyz[3 * k + m] = X[m];
  } else {
#pragma unroll
    for (int m = 0; m < 3; ++m) X[m] = a.xyz[3 * k + m];
  }
  if (a.with_angles) a.angles[k] = tri_angle(a.c1, a.c2, X);
}

// The argument checks of the batch entry point.  Host only.
mi_ba_status triangulation_check(const mi_ba_triangulation_options* o, const mi_ba_triangulation_batch* b) {
  if (!o || !b || b->num_problems < 0 || b->num_views < 0 || b->num_cameras < 0) return MI_BA_ERR_INVALID_ARGUMENT;
  // EstimateTriangulationOptions::Check, RANSACOptions::Check
  if (!(o->min_tri_angle >= 0.0) || !(o->max_error > 0.0) || !(o->min_inlier_ratio >= 0.0) ||
      !(o->min_inlier_ratio <= 1.0) || !(o->confidence >= 0.0) || !(o->confidence <= 1.0) || o->min_num_trials < 0 ||
      o->min_num_trials > o->max_num_trials)
    return MI_BA_ERR_INVALID_ARGUMENT;
  if (o->residual_type != MI_BA_TRIANGULATION_ANGULAR_ERROR && o->residual_type != MI_BA_TRIANGULATION_REPROJECTION_ERROR)
    return MI_BA_ERR_INVALID_ARGUMENT;
  const int n = b->num_problems;
  if (n == 0) return MI_BA_OK;
  if (!b->obs_offsets || !b->view_index || !b->proj_matrices || !b->proj_centers || !b->camera_index ||
      !b->camera_model_ids || !b->camera_param_offsets || !b->camera_params || b->obs_offsets[0] < 0)
    return MI_BA_ERR_INVALID_ARGUMENT;
  if (!b->points && (!b->points_normalized || o->residual_type == MI_BA_TRIANGULATION_REPROJECTION_ERROR))
    return MI_BA_ERR_INVALID_ARGUMENT;
  for (int k = 0; k < n; ++k) {
    const int64_t c = b->obs_offsets[k + 1] - b->obs_offsets[k];
    if (c < 2 || c > INT32_MAX) return MI_BA_ERR_INVALID_ARGUMENT;  // the reference CHECKs two observations
    if (b->min_num_trials && (b->min_num_trials[k] < 0 || b->min_num_trials[k] > o->max_num_trials))
      return MI_BA_ERR_INVALID_ARGUMENT;
  }
  for (int c = 0; c < b->num_cameras; ++c) {
    const int np = num_params(b->camera_model_ids[c]);
    if (np < 0 || b->camera_param_offsets[c + 1] - b->camera_param_offsets[c] != np) return MI_BA_ERR_INVALID_ARGUMENT;
  }
  for (int v = 0; v < b->num_views; ++v)
    if (b->camera_index[v] < 0 || b->camera_index[v] >= b->num_cameras) return MI_BA_ERR_INVALID_ARGUMENT;
  for (int64_t i = b->obs_offsets[0]; i < b->obs_offsets[n]; ++i)
    if (b->view_index[i] < 0 || b->view_index[i] >= b->num_views) return MI_BA_ERR_INVALID_ARGUMENT;
  return MI_BA_OK;
}

}  // namespace
}  // namespace miba

using namespace miba;

extern "C" void mi_ba_default_triangulation_options(mi_ba_triangulation_options* o) {
  if (!o) return;
  std::memset(o, 0, sizeof(*o));
  // EstimateTriangulationOptions (estimators/triangulation.h:123-138)
  o->min_tri_angle = 0.0;
  o->residual_type = MI_BA_TRIANGULATION_ANGULAR_ERROR;
  // RANSACOptions (optim/ransac.h:47-66)
  o->max_error = 0.0;
  o->min_inlier_ratio = 0.1;
  o->confidence = 0.99;
  o->dyn_num_trials_multiplier = 3.0;
  o->min_num_trials = 0;
  o->max_num_trials = INT64_MAX;
  o->device = 0;
}

extern "C" int32_t mi_ba_triangulation_lds_capacity(void) { return kTriLdsObs; }

extern "C" mi_ba_status mi_ba_estimate_triangulation_batch(const mi_ba_triangulation_options* o,
                                                           const mi_ba_triangulation_batch* b, double* xyz,
                                                           uint8_t* inlier_mask, int32_t* success,
                                                           int64_t* num_trials, int32_t* num_inliers,
                                                           int32_t* best_is_local) {
  mi_ba_status st = triangulation_check(o, b);
  if (st != MI_BA_OK) return st;
  const int n = b->num_problems;
  if (n == 0) return MI_BA_OK;
  if (!success) return MI_BA_ERR_INVALID_ARGUMENT;
  st = pose_select_device(o->device);
  if (st != MI_BA_OK) return st;

  const int64_t raw0 = b->obs_offsets[0], N = b->obs_offsets[n] - raw0;
  const int V = b->num_views, C = b->num_cameras;
  std::vector<TriProblemDev> list((size_t)n);
  int most_resident = 0;
  for (int k = 0; k < n; ++k) {
    const int64_t c = b->obs_offsets[k + 1] - b->obs_offsets[k];
    list[k] = TriProblemDev{b->obs_offsets[k] - raw0, b->min_num_trials ? b->min_num_trials[k] : o->min_num_trials,
                            (int32_t)c, k};
    if (c <= kTriLdsObs && c > most_resident) most_resident = (int)c;
  }
  // camera parameters in 8-wide slots
  std::vector<double> cam(8 * (size_t)(C ? C : 1), 0.0);
  for (int c = 0; c < C; ++c)
    for (int64_t m = b->camera_param_offsets[c]; m < b->camera_param_offsets[c + 1]; ++m)
      cam[8 * (size_t)c + (m - b->camera_param_offsets[c])] = b->camera_params[m];

  Buf bufs[12];
  int32_t* dview = bufs[0].alloc<int32_t>(N);
  double2* dpts = b->points ? bufs[1].alloc<double2>(N) : nullptr;
  double2* dpn = b->points_normalized ? bufs[2].alloc<double2>(N) : nullptr;
  double* dproj = bufs[3].alloc<double>(12 * (size_t)V);
  double* dcen = bufs[4].alloc<double>(3 * (size_t)V);
  int32_t* dvcam = bufs[5].alloc<int32_t>(V);
  double* dcam = bufs[6].alloc<double>(cam.size());
  int32_t* dmodel = bufs[7].alloc<int32_t>(C);
  double* drec = bufs[8].alloc<double>(kTriRecord * (size_t)N);
  TriProblemDev* dprob = bufs[9].alloc<TriProblemDev>(list.size());
  TriResult* dout = bufs[10].alloc<TriResult>(n);
  uint8_t* dmask = bufs[11].alloc<uint8_t>(N);
  if (!dview || (b->points && !dpts) || (b->points_normalized && !dpn) || !dproj || !dcen || !dvcam || !dcam ||
      !dmodel || !drec || !dprob || !dout || !dmask)
    return MI_BA_ERR_OUT_OF_MEMORY;
  if (hipMemcpy(dview, b->view_index + raw0, (size_t)N * 4, hipMemcpyHostToDevice) != hipSuccess ||
      (dpts && hipMemcpy(dpts, b->points + 2 * raw0, (size_t)N * 16, hipMemcpyHostToDevice) != hipSuccess) ||
      (dpn && hipMemcpy(dpn, b->points_normalized + 2 * raw0, (size_t)N * 16, hipMemcpyHostToDevice) != hipSuccess) ||
      hipMemcpy(dproj, b->proj_matrices, 12 * (size_t)V * 8, hipMemcpyHostToDevice) != hipSuccess ||
      hipMemcpy(dcen, b->proj_centers, 3 * (size_t)V * 8, hipMemcpyHostToDevice) != hipSuccess ||
      hipMemcpy(dvcam, b->camera_index, (size_t)V * 4, hipMemcpyHostToDevice) != hipSuccess ||
      hipMemcpy(dcam, cam.data(), cam.size() * 8, hipMemcpyHostToDevice) != hipSuccess ||
      hipMemcpy(dmodel, b->camera_model_ids, (size_t)C * 4, hipMemcpyHostToDevice) != hipSuccess ||
      hipMemcpy(dprob, list.data(), list.size() * sizeof(TriProblemDev), hipMemcpyHostToDevice) != hipSuccess ||
      hipMemset(dmask, 0, (size_t)N) != hipSuccess || hipMemset(dout, 0, (size_t)n * sizeof(TriResult)) != hipSuccess)
    return MI_BA_ERR_HIP;

  TriRecordArgs r{};
  r.view_index = dview;
  r.points = dpts;
  r.points_normalized = dpn;
  r.proj = dproj;
  r.centers = dcen;
  r.view_cam = dvcam;
  r.cams = TriCameras{dcam, dmodel};
  r.rec = drec;
  r.n = N;
  hipLaunchKernelGGL(triangulation_records_kernel, dim3((unsigned)((N + 255) / 256)), dim3(256), 0, 0, r);
  if (hipGetLastError() != hipSuccess) return MI_BA_ERR_HIP;

  TriArgs a{};
  a.prob = dprob;
  a.rec = drec;
  a.cams = r.cams;
  a.opt.min_tri_angle = o->min_tri_angle;
  a.opt.max_residual = o->max_error * o->max_error;
  a.opt.confidence = o->confidence;
  a.opt.dyn_num_trials_multiplier = o->dyn_num_trials_multiplier;
  a.opt.max_num_trials =
      tri_constructor_cap(o->max_num_trials, o->min_inlier_ratio, o->confidence, o->dyn_num_trials_multiplier);
  a.opt.residual_type = o->residual_type;
  a.out = dout;
  a.mask = dmask;
  a.num_listed = n;
  // the arrays' stride only: a track is resident exactly when its own count is at most kTriLdsObs
  a.lds_obs = (most_resident + 1) / 2 * 2;
  const size_t bytes = (size_t)kPoseWaves * kTriLdsStride * a.lds_obs * 8;
  if (hipFuncSetAttribute(reinterpret_cast<const void*>(&triangulation_kernel),
                          hipFuncAttributeMaxDynamicSharedMemorySize, (int)bytes) != hipSuccess)
    return MI_BA_ERR_HIP;
  const unsigned groups = (unsigned)((list.size() + kPoseWaves - 1) / kPoseWaves);
  hipLaunchKernelGGL(triangulation_kernel, dim3(groups), dim3(kPoseTB), bytes, 0, a);
  if (hipGetLastError() != hipSuccess) return MI_BA_ERR_HIP;
  if (hipStreamSynchronize(0) != hipSuccess) return MI_BA_ERR_HIP;

  std::vector<TriResult> out((size_t)n);
  std::vector<uint8_t> hmask((size_t)N);
  if (hipMemcpy(out.data(), dout, out.size() * sizeof(TriResult), hipMemcpyDeviceToHost) != hipSuccess ||
      hipMemcpy(hmask.data(), dmask, (size_t)N, hipMemcpyDeviceToHost) != hipSuccess)
    return MI_BA_ERR_HIP;
  for (int k = 0; k < n; ++k) {
    const TriResult& r = out[k];
    success[k] = r.success;
    if (num_trials) num_trials[k] = r.num_trials;
    if (num_inliers) num_inliers[k] = r.num_inliers;
    if (best_is_local) best_is_local[k] = r.best_is_local;
    if (!r.success) continue;  // a failed track leaves xyz and its mask untouched
    if (xyz)
      for (int m = 0; m < 3; ++m) xyz[3 * (size_t)k + m] = r.xyz[m];
    if (inlier_mask)
      std::memcpy(inlier_mask + b->obs_offsets[k], hmask.data() + (b->obs_offsets[k] - raw0),
                  (size_t)(b->obs_offsets[k + 1] - b->obs_offsets[k]));
  }
  return MI_BA_OK;
}

extern "C" mi_ba_status mi_ba_triangulate_points(const double* proj_matrix1, const double* proj_matrix2, int64_t m,
                                                 const double* points1, const double* points2,
                                                 const double* proj_center1, const double* proj_center2,
                                                 int32_t device, double* xyz, double* angles) {
  const bool tri = proj_matrix1 || proj_matrix2 || points1 || points2;
  const bool ang = proj_center1 || proj_center2 || angles;
  if (m < 0 || (!tri && !ang)) return MI_BA_ERR_INVALID_ARGUMENT;
  if (tri && (!proj_matrix1 || !proj_matrix2)) return MI_BA_ERR_INVALID_ARGUMENT;
  if (ang && (!proj_center1 || !proj_center2)) return MI_BA_ERR_INVALID_ARGUMENT;
  if (m > 0 && (!xyz || (tri && (!points1 || !points2)) || (ang && !angles))) return MI_BA_ERR_INVALID_ARGUMENT;
  mi_ba_status st = pose_select_device(device);
  if (st != MI_BA_OK) return st;
  if (m == 0) return MI_BA_OK;
  Buf bufs[4];
  double2* d1 = tri ? bufs[0].alloc<double2>(m) : nullptr;
  double2* d2 = tri ? bufs[1].alloc<double2>(m) : nullptr;
  double* dxyz = bufs[2].alloc<double>(3 * (size_t)m);
  double* dang = ang ? bufs[3].alloc<double>(m) : nullptr;
  if ((tri && (!d1 || !d2)) || !dxyz || (ang && !dang)) return MI_BA_ERR_OUT_OF_MEMORY;
  if (tri) {
    if (hipMemcpy(d1, points1, (size_t)m * 16, hipMemcpyHostToDevice) != hipSuccess ||
        hipMemcpy(d2, points2, (size_t)m * 16, hipMemcpyHostToDevice) != hipSuccess)
      return MI_BA_ERR_HIP;
  } else if (hipMemcpy(dxyz, xyz, 3 * (size_t)m * 8, hipMemcpyHostToDevice) != hipSuccess) {
    return MI_BA_ERR_HIP;
  }
  TriPointsArgs a{};
  for (int k = 0; k < 12; ++k) {
    a.P1[k] = tri ? proj_matrix1[k] : 0.0;
    a.P2[k] = tri ? proj_matrix2[k] : 0.0;
  }
  for (int k = 0; k < 3; ++k) {
    a.c1[k] = ang ? proj_center1[k] : 0.0;
    a.c2[k] = ang ? proj_center2[k] : 0.0;
  }
  a.p1 = d1;
  a.p2 = d2;
  a.xyz = dxyz;
  a.angles = dang;
  a.m = m;
  a.triangulate = tri ? 1 : 0;
  a.with_angles = ang ? 1 : 0;
  hipLaunchKernelGGL(triangulate_points_kernel, dim3((unsigned)((m + 255) / 256)), dim3(256), 0, 0, a);
  if (hipGetLastError() != hipSuccess || hipStreamSynchronize(0) != hipSuccess) return MI_BA_ERR_HIP;
  if ((tri && hipMemcpy(xyz, dxyz, 3 * (size_t)m * 8, hipMemcpyDeviceToHost) != hipSuccess) ||
      (ang && hipMemcpy(angles, dang, (size_t)m * 8, hipMemcpyDeviceToHost) != hipSuccess))
    return MI_BA_ERR_HIP;
  return MI_BA_OK;
}
