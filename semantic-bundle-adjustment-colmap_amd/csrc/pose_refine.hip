// pose_refine.hip — batched absolute-pose refinement (product code).
//
//   mi_ba_refine_absolute_pose_batch  <- RefineAbsolutePose
//                                        (src/estimators/pose.cc:198-322)
//
// One workgroup per problem; the whole Levenberg-Marquardt solve (Ceres 2.1
// TrustRegionMinimizer with its default options, restated as in runtime.hip
// context_solve) runs inside pose_refine_kernel with no host round trip.
//
// Per linearization the four waves stride over the problem's observations in
// tiles of 64 (tile t belongs to wave t % 4).  Each lane evaluates the
// residual and the loss-corrected tangent Jacobian of its observation with
// the chain rule the reprojection kernel uses (reproj_block.h, ba_math.h) and
// writes its two rows, as the columns of the augmented matrix [J r], into the
// wave's LDS slab: column c holds 128 values (row x of the 64 observations,
// then row y).  Every lane owns one or two entries (i, j) of the upper
// triangle of [J r]'[J r] — J'J, the gradient J'r and r'r — and sums the
// slab's 128 products in order, so the accumulators never leave two
// registers per lane.  Waves are combined in wave order: every sum has a
// fixed order and no atomics, the same input gives the same bits.
//
// LDS banking (64 banks of 4 B): a column has a stride of 129 doubles, so
// the lanes' column reads (i * 129 + k) fall on banks 2 i + 2 k mod 64 — at
// most 15 distinct columns, no conflict; lanes that share a column read one
// address (broadcast).  The row writes are consecutive doubles.
//
// Wave 0 then runs the small solve with lane i owning row i of the system
// (at most 14 x 14): Jacobi scaling, LM damping, a right-looking Cholesky
// over LDS rows (column k reaches the other lanes through LDS), the two
// triangular solves, the model cost change and the candidate point: wave 0's
// blocks of pose_common.h (PoseLmLds), shared with generalized_pose_kernel.
// A second pass over the observations gives the candidate cost.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstring>
#include <vector>

#include "../../include/mi_ba.h"
#include "ba_math.h"
#include "pose_common.h"
#include "reproj_block.h"

namespace miba {
namespace {

// Most observations kept in LDS (5 doubles each: 80 KiB of the CU's 160 KiB,
// beside 70 KiB of slabs and system at the 14-wide instantiation).
constexpr int kPoseLdsObs = 2048;
struct PoseProblemDev {
  int64_t obs_begin;  // into the compacted correspondence arrays
  int32_t count;      // inliers
  int32_t model;
  int32_t ct;         // refined intrinsics (0: pose only)
  int32_t np;         // camera parameters
  int32_t idx[8];     // refined parameter indices
  int32_t index;      // problem index of the batch (state / out / cov rows)
  int32_t pad;
};

struct PoseArgs {
  const PoseProblemDev* prob;
  const double2* p2;
  const double* p3;
  double* state;  // [n][16] q(4) t(3) pad params(8), in/out
  double* out;    // [n][kOutStride]
  double* cov;    // nullable [n][36]
  double gradient_tolerance;
  double loss_scale;
  int32_t max_num_iterations;
  int32_t lds_obs;  // observations the launch's LDS holds
  uint8_t* trace;   // nullable [n][trace_cap]: outcome of each LM iteration (mi_ba_pose_refine_set_trace)
  int32_t trace_cap;
};

// Cost 0.5 rho(|r|^2) of one observation at the parameters st (q t pad params).
__device__ inline double pose_obs_cost(int model, const double* st, double loss_scale, double ox, double oy,
                                       const double X[3]) {
  const double q[4] = {st[0], st[1], st[2], st[3]};
  double prm[8];
#pragma unroll
  for (int k = 0; k < 8; ++k) prm[k] = st[8 + k];
  double P[3];
  unit_quat_rotate(q, X, P);
  P[0] += st[4];
  P[1] += st[5];
  P[2] += st[6];
  const double iz = 1.0 / P[2];
  double x, y;
  world_to_image_all(model, prm, P[0] * iz, P[1] * iz, &x, &y);
  const double r0 = x - ox, r1 = y - oy;
  double rho[3];
  loss_eval(kLossCauchy, loss_scale, r0 * r0 + r1 * r1, rho);
  return 0.5 * rho[0];
}

// Residual, loss-corrected tangent rows (rotation 3, translation 3, refined
// intrinsics NT - 6) and cost of one observation: the arithmetic of
// reproj_jacobian_kernel for a variable pose and a constant point.
template <int NT>
__device__ inline void pose_obs_rows(int model, const double* st, const int* idx, int ct, double loss_scale, double ox,
                                     double oy, const double X[3], double (&J0)[NT + 1], double (&J1)[NT + 1],
                                     double* cost) {
  const double q[4] = {st[0], st[1], st[2], st[3]};
  double prm[8];
#pragma unroll
  for (int k = 0; k < 8; ++k) prm[k] = st[8 + k];
  double P[3];
  unit_quat_rotate(q, X, P);
  const double a0 = P[0], a1 = P[1], a2 = P[2];  // R X
  P[0] += st[4];
  P[1] += st[5];
  P[2] += st[6];
  const double iz = 1.0 / P[2];
  const double u = P[0] * iz, v = P[1] * iz;
  double x, y, A[4], Jp8[16];
  world_to_image_jac_all(model, prm, u, v, &x, &y, A, Jp8);
  const double r0 = x - ox, r1 = y - oy;
  double rho[3];
  loss_eval(kLossCauchy, loss_scale, r0 * r0 + r1 * r1, rho);
  *cost = 0.5 * rho[0];
  // Ceres Corrector, rho'' <= 0 branch: r, J *= sqrt(rho')
  const double sc = sqrt(rho[1]);
  double B[6], Mq[9];
  reproj_dpixel_dpoint(A, iz, u, v, B);
#pragma unroll
  for (int k = 0; k < 6; ++k) B[k] *= sc;
  rotation_tangent_jacobian(q, X, a0, a1, a2, true, quat_is_unit(q), Mq);
  emit_row_pose(0, J0, B, Mq, true, 0u);
  emit_row_pose(1, J1, B, Mq, true, 0u);
  // The refined-intrinsics columns and the residual column.  Kept in this
  // function, not in a helper shared with gpose_obs_rows: moved into one, the
  // compiler pairs the products of the camera model's Jacobian differently and
  // a last bit of [J r]'[J r] changes.
  if constexpr (NT > 6) {
#pragma unroll
    for (int m = 0; m < NT - 6; ++m) {
      double v0 = 0.0, v1 = 0.0;
      const int im = m < ct ? idx[m] : -1;
#pragma unroll
      for (int k = 0; k < 8; ++k) {
        v0 = im == k ? Jp8[k] : v0;
        v1 = im == k ? Jp8[8 + k] : v1;
      }
      J0[6 + m] = v0 * sc;
      J1[6 + m] = v1 * sc;
    }
  }
  J0[NT] = r0 * sc;
  J1[NT] = r1 * sc;
}

template <int NT>
constexpr int pose_lds_doubles(int lds_obs) {
  constexpr int NC = NT + 1;
  return kPoseWaves * NC * kColStride + kPoseWaves * 128 + NC * NC + kPoseTB + 16 + 16 + NT * (NT + 1) + 3 * 16 +
         (int)(sizeof(PoseLm) / 8) + 8 + 5 * lds_obs;
}
static_assert(pose_lds_doubles<14>(kPoseLdsObs) * 8 <= 160 * 1024, "LDS budget of one workgroup");

template <int NT>
__global__ __launch_bounds__(kPoseTB) void pose_refine_kernel(PoseArgs a) {
  constexpr int NC = NT + 1;
  constexpr int NE = NC * (NC + 1) / 2;
  constexpr int EPL = (NE + 63) / 64;
  extern __shared__ double lds[];
  double* slab_all = lds;
  double* red = slab_all + kPoseWaves * NC * kColStride;
  double* sM = red + kPoseWaves * 128;  // [NC][NC] symmetric [J r]'[J r]
  double* sCost = sM + NC * NC;
  double* sState = sCost + kPoseTB;
  double* sCand = sState + 16;
  double* sA = sCand + 16;              // [NT][NT + 1] system / factor
  double* sScale = sA + NT * (NT + 1);  // Jacobi scaling per column, from the first Jacobian
  double* sStep = sScale + 16;
  double* sD0 = sStep + 16;
  PoseLm* lm = reinterpret_cast<PoseLm*>(sD0 + 16);
  int* sIdx = reinterpret_cast<int*>(reinterpret_cast<double*>(lm) + sizeof(PoseLm) / 8);
  int* sTan = sIdx + 8 - 6;  // tangent column 6 + m -> index into sState, in the second half of sIdx's 16 ints
  double* sObs = reinterpret_cast<double*>(sIdx) + 8;
  const PoseLmLds<NC, NT + 1, 16, false> solve{sM, sA, sScale, sStep, sD0, lm, sTan};

  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const PoseProblemDev* pb = a.prob + blockIdx.x;
  const int count = pb->count, model = pb->model, ct = pb->ct, n = 6 + ct, index = pb->index;
  const PoseLmOptions opt{a.gradient_tolerance, a.max_num_iterations, a.trace, a.trace_cap, index};
  if (count <= 0) {  // nothing to do: CONVERGENCE, parameters as they are
    if (tid == 0) {
      double* out = a.out + (size_t)index * kOutStride;
      out[0] = 0.0; out[1] = 0.0; out[2] = 0.0; out[3] = 0.0; out[4] = MI_BA_CONVERGENCE; out[5] = 0.0;
    }
    return;
  }
  PoseObsSource<false> src;
  src.lds_obs = a.lds_obs;
  src.resident = count <= a.lds_obs;
  src.sx = sObs;
  src.p2 = a.p2 + pb->obs_begin;
  src.p3 = a.p3 + 3 * pb->obs_begin;
  src.stage(tid, count);
  if (tid < 16) sState[tid] = a.state[(size_t)index * 16 + tid];
  if (tid < 8) {
    sIdx[tid] = pb->idx[tid];
    sTan[6 + tid] = 8 + pb->idx[tid];
  }
  solve.init(tid);
  __syncthreads();

  int ei[EPL], ej[EPL];
  pose_triangle_entries<NC>(lane, ei, ej);

  bool first = true;
  int action = kActAccept;  // the first pass linearizes at the given point
  while (true) {
    if (action == kActAccept) {
      // [J r]'[J r] and the cost at sState -> sM
      double* slab = slab_all + wave * NC * kColStride;
      int idx[8];
#pragma unroll
      for (int k = 0; k < 8; ++k) idx[k] = sIdx[k];
      double acc[EPL];
#pragma unroll
      for (int s = 0; s < EPL; ++s) acc[s] = 0.0;
      double cost_acc = 0.0;
      for (int tile = wave; tile * 64 < count; tile += kPoseWaves) {
        const int i = tile * 64 + lane;
        double J0[NC], J1[NC];
#pragma unroll
        for (int c = 0; c < NC; ++c) { J0[c] = 0.0; J1[c] = 0.0; }
        if (i < count) {
          double ox, oy, X[3], cost;
          src.load(i, &ox, &oy, X);
          pose_obs_rows<NT>(model, sState, idx, ct, a.loss_scale, ox, oy, X, J0, J1, &cost);
          cost_acc += cost;
        }
        pose_tile_products<NC>(slab, lane, J0, J1, ei, ej, acc);
      }
#pragma unroll
      for (int s = 0; s < EPL; ++s) red[wave * 128 + lane + 64 * s] = acc[s];
      sCost[tid] = cost_acc;
      __syncthreads();
      if (wave == 0) {
#pragma unroll
        for (int s = 0; s < EPL; ++s) {
          const int e = lane + 64 * s;
          if (e < NE) {
            double v = red[e];
#pragma unroll
            for (int w = 1; w < kPoseWaves; ++w) v += red[w * 128 + e];
            sM[ei[s] * NC + ej[s]] = v;
            sM[ej[s] * NC + ei[s]] = v;
          }
        }
        const double total = pose_cost_total(sCost, lane);
        wave_sync();
        if (first) solve.first(n, lane, total);
      }
      first = false;
    }

    if (wave == 0) {
      int act = kActStop;
      double model_cost_change;
      if (solve.propose(sState, sCand, 16, n, lane, opt, &model_cost_change)) {
        // |x|^2, |x - candidate|^2 over the variable blocks in ambient
        // coordinates: qvec, tvec, and every parameter of a refined camera
        double xn2 = 0.0, sn2 = 0.0;
        const int nstate = ct > 0 ? 8 + pb->np : 7;
#pragma unroll 1  // rolled, as it compiled inside the kernel's own LM loop
        for (int m = 0; m < nstate; ++m) {
          if (m == 7) continue;
          const double xv = sState[m], dv = xv - sCand[m];
          xn2 += xv * xv;
          sn2 += dv * dv;
        }
        solve.candidate_ready(lane, model_cost_change, xn2, sn2);
        act = kActEval;
      }
      if (lane == 0) lm->action0 = act;
    }
    __syncthreads();
    if (lm->action0 == kActStop) break;

    // candidate cost: the second pass over the observations
    {
      double cost_acc = 0.0;
      for (int i = tid; i < count; i += kPoseTB) {
        double ox, oy, X[3];
        src.load(i, &ox, &oy, X);
        cost_acc += pose_obs_cost(model, sCand, a.loss_scale, ox, oy, X);
      }
      sCost[tid] = cost_acc;
    }
    __syncthreads();
    if (wave == 0 && solve.judge(sCost, lane, opt) == kActAccept && lane < 16) sState[lane] = sCand[lane];
    __syncthreads();
    action = lm->action1;
    if (action == kActStop) break;
  }

  if (wave != 0) return;
  wave_sync();
  solve.finish(n, lane, a.cov, a.out, index);
  if (lane < 16 && lm->termination != MI_BA_FAILURE) a.state[(size_t)index * 16 + lane] = sState[lane];
}

}  // namespace
}  // namespace miba

using namespace miba;

namespace {
uint8_t* g_pose_trace = nullptr;
int32_t g_pose_trace_cap = 0;
}  // namespace

void miba::pose_trace_target(uint8_t** trace, int32_t* capacity) {
  *trace = g_pose_trace;
  *capacity = g_pose_trace_cap;
}

extern "C" void mi_ba_pose_refine_set_trace(uint8_t* trace, int32_t capacity) {
  g_pose_trace = capacity > 0 ? trace : nullptr;
  g_pose_trace_cap = trace ? capacity : 0;
}

extern "C" void mi_ba_default_pose_refine_options(mi_ba_pose_refine_options* o) {
  if (!o) return;
  std::memset(o, 0, sizeof(*o));
  // AbsolutePoseRefinementOptions (src/estimators/pose.h:93-124)
  o->gradient_tolerance = 1.0;
  o->max_num_iterations = 100;
  o->loss_function_scale = 1.0;
  o->refine_focal_length = 1;
  o->refine_extra_params = 1;
  o->device = 0;
}

extern "C" int32_t mi_ba_pose_refine_intrinsics(int32_t camera_model, int32_t refine_focal_length,
                                                int32_t refine_extra_params, int32_t* idxs) {
  if (num_params(camera_model) < 0) return -1;
  // the principal point stays fixed (pose.cc:251-257)
  const unsigned mask =
      cam_tangent_mask_all(camera_model, (refine_focal_length ? 1 : 0) | (refine_extra_params ? 4 : 0));
  int32_t c = 0;
  for (int k = 0; k < 8; ++k)
    if ((mask >> k) & 1u) {
      if (idxs) idxs[c] = k;
      ++c;
    }
  return c;
}

extern "C" int32_t mi_ba_pose_refine_lds_capacity(void) { return kPoseLdsObs; }

extern "C" mi_ba_status mi_ba_refine_absolute_pose_batch(const mi_ba_pose_refine_options* o,
                                                         const mi_ba_pose_batch* b, int32_t* statuses,
                                                         mi_ba_summary* summaries, int32_t* usable) {
  if (!o || !b || b->num_problems < 0) return MI_BA_ERR_INVALID_ARGUMENT;
  if (!pose_options_check(o->gradient_tolerance, o->max_num_iterations, o->loss_function_scale))
    return MI_BA_ERR_INVALID_ARGUMENT;
  const int n = b->num_problems;
  if (n == 0) return MI_BA_OK;
  if (!statuses || !summaries || !usable || !b->obs_offsets || !b->camera_model_ids || !b->camera_param_offsets ||
      !b->camera_params || !b->qvec || !b->tvec)
    return MI_BA_ERR_INVALID_ARGUMENT;
  if (b->obs_offsets[0] < 0 || b->camera_param_offsets[0] < 0) return MI_BA_ERR_INVALID_ARGUMENT;
  for (int k = 0; k < n; ++k) {
    const int64_t c = b->obs_offsets[k + 1] - b->obs_offsets[k];
    if (c < 0 || c > INT32_MAX) return MI_BA_ERR_INVALID_ARGUMENT;
    const int np = num_params(b->camera_model_ids[k]);
    const int64_t have = b->camera_param_offsets[k + 1] - b->camera_param_offsets[k];
    if (have < 0 || (np >= 0 && have != np)) return MI_BA_ERR_INVALID_ARGUMENT;
  }
  const int64_t total = b->obs_offsets[n];
  if (total > 0 && (!b->points2D || !b->points3D)) return MI_BA_ERR_INVALID_ARGUMENT;
  const mi_ba_status dev = pose_select_device(o->device);
  if (dev != MI_BA_OK) return dev;

  // Host assembly: inlier compaction, unit qvec, refined-intrinsics sets.
  std::vector<PoseProblemDev> narrow, wide;
  std::vector<double> state(16 * (size_t)n, 0.0);
  std::vector<double> c2, c3;  // compacted correspondences (with a mask)
  const bool masked = b->inlier_mask != nullptr;
  if (masked) {
    c2.reserve(2 * (size_t)total);
    c3.reserve(3 * (size_t)total);
  }
  for (int k = 0; k < n; ++k) {
    std::memset(&summaries[k], 0, sizeof(mi_ba_summary));
    usable[k] = 0;
    const int model = b->camera_model_ids[k];
    const int np = num_params(model);
    if (np < 0) {
      statuses[k] = MI_BA_ERR_UNSUPPORTED;
      continue;
    }
    statuses[k] = MI_BA_OK;
    PoseProblemDev pb{};
    pb.model = model;
    pb.np = np;
    pb.index = k;
    pb.ct = mi_ba_pose_refine_intrinsics(model, o->refine_focal_length, o->refine_extra_params, pb.idx);
    const int64_t b0 = b->obs_offsets[k], b1 = b->obs_offsets[k + 1];
    if (masked) {
      pb.obs_begin = (int64_t)(c2.size() / 2);
      for (int64_t i = b0; i < b1; ++i) {
        if (!b->inlier_mask[i]) continue;
        c2.push_back(b->points2D[2 * i]);
        c2.push_back(b->points2D[2 * i + 1]);
        for (int m = 0; m < 3; ++m) c3.push_back(b->points3D[3 * i + m]);
      }
      pb.count = (int32_t)((int64_t)(c2.size() / 2) - pb.obs_begin);
    } else {
      pb.obs_begin = b0;
      pb.count = (int32_t)(b1 - b0);
    }
    double* st = &state[16 * (size_t)k];
    pose_unit_quat_copy(b->qvec + 4 * (size_t)k, st);
    for (int m = 0; m < 3; ++m) st[4 + m] = b->tvec[3 * (size_t)k + m];
    for (int m = 0; m < np; ++m) st[8 + m] = b->camera_params[b->camera_param_offsets[k] + m];
    summaries[k].num_residuals_reduced = 2 * (int64_t)pb.count;
    summaries[k].num_effective_parameters_reduced = pb.count > 0 ? 6 + pb.ct : 0;
    if (pb.count == 0) {  // no residuals: nothing to do
      summaries[k].termination_type = MI_BA_CONVERGENCE;
      usable[k] = 1;
      continue;
    }
    (pb.ct == 0 ? narrow : wide).push_back(pb);
  }
  if (narrow.empty() && wide.empty()) return MI_BA_OK;

  const double* h2 = masked ? c2.data() : b->points2D;
  const double* h3 = masked ? c3.data() : b->points3D;
  const int64_t N = masked ? (int64_t)(c2.size() / 2) : total;
  Buf bufs[7];
  double2* d2 = bufs[0].alloc<double2>(N);
  double* d3 = bufs[1].alloc<double>(3 * (size_t)N);
  double* dstate = bufs[2].alloc<double>(state.size());
  double* dout = bufs[3].alloc<double>(kOutStride * (size_t)n);
  double* dcov = b->rot_tvec_covariance ? bufs[4].alloc<double>(36 * (size_t)n) : nullptr;
  if (!d2 || !d3 || !dstate || !dout || (b->rot_tvec_covariance && !dcov)) return MI_BA_ERR_OUT_OF_MEMORY;
  if (hipMemcpy(d2, h2, (size_t)N * 16, hipMemcpyHostToDevice) != hipSuccess ||
      hipMemcpy(d3, h3, (size_t)N * 24, hipMemcpyHostToDevice) != hipSuccess ||
      hipMemcpy(dstate, state.data(), state.size() * 8, hipMemcpyHostToDevice) != hipSuccess ||
      hipMemset(dout, 0, kOutStride * (size_t)n * 8) != hipSuccess)
    return MI_BA_ERR_HIP;
  PoseArgs a{};
  a.p2 = d2;
  a.p3 = d3;
  a.state = dstate;
  a.out = dout;
  a.cov = dcov;
  a.gradient_tolerance = o->gradient_tolerance;
  a.loss_scale = o->loss_function_scale;
  a.max_num_iterations = o->max_num_iterations;
  PoseTraceBuf trace;
  mi_ba_status st = trace.setup(n);
  if (st != MI_BA_OK) return st;
  a.trace = trace.dev;
  a.trace_cap = trace.cap;
  // specialised on the tangent width: pose only (6) and pose + intrinsics (up to 14)
  st = pose_launch(&pose_refine_kernel<6>, &pose_lds_doubles<6>, kPoseLdsObs, a, narrow, &bufs[5]);
  if (st != MI_BA_OK) return st;
  st = pose_launch(&pose_refine_kernel<14>, &pose_lds_doubles<14>, kPoseLdsObs, a, wide, &bufs[6]);
  if (st != MI_BA_OK) return st;
  if (hipStreamSynchronize(0) != hipSuccess) return MI_BA_ERR_HIP;
  std::vector<double> out(kOutStride * (size_t)n), cov(dcov ? 36 * (size_t)n : 0);
  if (!pose_download(&state, dstate) || !pose_download(&out, dout) || (dcov && !pose_download(&cov, dcov)))
    return MI_BA_ERR_HIP;
  if (trace.download() != MI_BA_OK) return MI_BA_ERR_HIP;
  auto finish = [&](const PoseProblemDev& pb) {
    const int k = pb.index;
    const double* r = &out[kOutStride * (size_t)k];
    bool ok = pose_summary_fill(r, &summaries[k]);
    if (ok) {
      const double* stp = &state[16 * (size_t)k];
      for (int m = 0; m < 4; ++m) b->qvec[4 * (size_t)k + m] = stp[m];
      for (int m = 0; m < 3; ++m) b->tvec[3 * (size_t)k + m] = stp[4 + m];
      for (int m = 0; m < pb.ct; ++m) b->camera_params[b->camera_param_offsets[k] + pb.idx[m]] = stp[8 + pb.idx[m]];
      if (dcov) {
        if (r[5] != 0.0)
          std::memcpy(b->rot_tvec_covariance + 36 * (size_t)k, &cov[36 * (size_t)k], 36 * 8);
        else
          ok = false;  // covariance.Compute failed (pose.cc:311-313)
      }
    }
    usable[k] = ok ? 1 : 0;
  };
  for (const PoseProblemDev& pb : narrow) finish(pb);
  for (const PoseProblemDev& pb : wide) finish(pb);
  return MI_BA_OK;
}
