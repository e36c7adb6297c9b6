// generalized_pose.hip — batched generalized absolute-pose refinement of
// camera rigs (product code).
//
//   mi_ba_refine_generalized_absolute_pose_batch
//       <- RefineGeneralizedAbsolutePose (src/estimators/pose.cc:354-520)
//
// One workgroup per problem, the whole Levenberg-Marquardt loop on the device,
// as pose_refine_kernel.  The residual is RigBundleAdjustmentCostFunction's
// (cost_functions.h:160-214) with the relative poses and the points constant:
// Y = R(q_rig) X + t_rig, P = R(q_rel) Y + t_rel, so the pixel's derivative by
// the rig tangent is (B R_rel) times the pose Jacobian of Y, B = d pixel / dP.
//
// Layout.  The host lists the inliers stably grouped by camera (an index per
// inlier into the caller's arrays, which are uploaded as they are); a tile of
// 64 never straddles two cameras.  The tile list (camera major) is
// cut into four contiguous runs, one per wave.  A run of tiles of one camera
// inside one wave is a segment: at most cameras + 3 of them.  Per segment the
// wave sums the camera's 15-wide [J r]'[J r] (6 rig columns, up to 8 of the
// camera, r) with pose_refine_kernel's slab scheme, two triangle entries per
// lane, and parks the 120 sums in LDS.  Wave 0 then adds the segments in
// segment order into the dense system: the rig block and gradient collect
// every segment, a camera's own columns its segments only.  Every sum has a
// fixed order and no atomics; the order depends on the problem alone.
//
// The solve is dense, lane i of wave 0 owning row i (tangent <= 64): Jacobi
// scaling, LM damping, Cholesky, the two triangular solves.  The system
// matrix lives in the slabs' LDS, which is idle between linearizations.
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

constexpr int kGMaxCams = 16;
constexpr int kGMaxTangent = 64;
constexpr int kGMaxSegs = kGMaxCams + kPoseWaves - 1;
// Most observations kept in LDS (5 doubles each, 35 KiB) beside the wide
// instantiation's 121 KiB of slabs, segment sums, system and state.
constexpr int kGLdsObs = 896;
constexpr int kGStateDoubles = 8 + 8 * kGMaxCams;  // q(4) t(3) pad, then 8 per camera
constexpr int kGCamInts = 12;                      // model, np, ct, tangent offset, idx[8]

struct GCamDev {
  double rel[12];  // R(q_rel) row-major, t_rel
  int32_t model, np, ct, off;  // off: first tangent column, -1 for a camera without inliers
  int32_t idx[8];
};

struct GTile {
  int32_t cam, start, count, seg;
};

struct GProblemDev {
  int64_t obs_begin;   // into the grouped inlier list
  int64_t raw_begin;   // the problem's first correspondence in the uploaded arrays
  int64_t tile_begin;  // into the tile table
  int64_t cam_begin;   // into the camera table and the camera parameter slots
  int32_t count, ncam, n, ntiles, nseg, index;
  int32_t wave_tile[kPoseWaves + 1];  // wave w owns tiles wave_tile[w] .. wave_tile[w + 1])
  int32_t seg_cam[kGMaxSegs];
};

struct GPoseArgs {
  const GProblemDev* prob;
  const GCamDev* cams;
  const GTile* tiles;
  const int32_t* order;  // grouped inlier list: correspondence indices local to their problem
  const double2* p2;
  const double* p3;
  double* rig;   // [n][8] q(4) t(3) pad, in/out
  double* cprm;  // [cameras][8], in/out
  double* out;   // [n][kOutStride]
  double* cov;   // nullable [n][36]
  double gradient_tolerance;
  double loss_scale;
  int32_t max_num_iterations;
  int32_t lds_obs;
  uint8_t* trace;
  int32_t trace_cap;
};

// Camera-frame point of the rig camera: P = R_rel (R(q) X + t) + t_rel; a = R(q) X.
__device__ __forceinline__ void gpose_point(const double* rig, const double* rel, const double X[3], double a[3],
                                            double P[3]) {
  const double q[4] = {rig[0], rig[1], rig[2], rig[3]};
  unit_quat_rotate(q, X, a);
  const double Y0 = a[0] + rig[4], Y1 = a[1] + rig[5], Y2 = a[2] + rig[6];
  P[0] = rel[0] * Y0 + rel[1] * Y1 + rel[2] * Y2 + rel[9];
  P[1] = rel[3] * Y0 + rel[4] * Y1 + rel[5] * Y2 + rel[10];
  P[2] = rel[6] * Y0 + rel[7] * Y1 + rel[8] * Y2 + rel[11];
}

// Cost 0.5 rho(|r|^2) of one observation: rig = q t, prm8 the camera's slot.
__device__ inline double gpose_obs_cost(int model, const double* rig, const double* prm8, const double* rel,
                                        double loss_scale, double ox, double oy, const double X[3]) {
  double prm[8];
#pragma unroll
  for (int k = 0; k < 8; ++k) prm[k] = prm8[k];
  double a[3], P[3];
  gpose_point(rig, rel, X, a, P);
  const double iz = 1.0 / P[2];
  double x, y;
  world_to_image_all(model, prm, P[0] * iz, P[1] * iz, &x, &y);
  const double r0 = x - ox, r1 = y - oy;
  double rho[3];
  loss_eval(kLossCauchy, loss_scale, r0 * r0 + r1 * r1, rho);
  return 0.5 * rho[0];
}

// Residual, loss-corrected rows (rig rotation 3, rig translation 3, the
// camera's refined intrinsics LT - 6) and cost of one observation.
template <int LT>
__device__ inline void gpose_obs_rows(int model, const double* rig, const double* prm8, const double* rel,
                                      const int* idx, int ct, double loss_scale, double ox, double oy,
                                      const double X[3], double (&J0)[LT + 1], double (&J1)[LT + 1], double* cost) {
  const double q[4] = {rig[0], rig[1], rig[2], rig[3]};
  double prm[8];
#pragma unroll
  for (int k = 0; k < 8; ++k) prm[k] = prm8[k];
  double a[3], P[3];
  gpose_point(rig, rel, X, a, P);
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
  double B[6], BR[6], Mq[9];
  reproj_dpixel_dpoint(A, iz, u, v, B);
#pragma unroll
  for (int k = 0; k < 6; ++k) B[k] *= sc;
  // d pixel / dY = B R_rel
#pragma unroll
  for (int r = 0; r < 2; ++r)
#pragma unroll
    for (int b = 0; b < 3; ++b) BR[r * 3 + b] = B[r * 3] * rel[b] + B[r * 3 + 1] * rel[3 + b] + B[r * 3 + 2] * rel[6 + b];
  rotation_tangent_jacobian(q, X, a[0], a[1], a[2], true, quat_is_unit(q), Mq);
  emit_row_pose(0, J0, BR, Mq, true, 0u);
  emit_row_pose(1, J1, BR, Mq, true, 0u);
  // The refined-intrinsics columns and the residual column.  Kept in this
  // function, not in a helper shared with pose_obs_rows: moved into one, the
  // compiler pairs the products of the camera model's Jacobian differently and
  // a last bit of [J r]'[J r] changes.
  if constexpr (LT > 6) {
#pragma unroll
    for (int m = 0; m < LT - 6; ++m) {
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
  J0[LT] = r0 * sc;
  J1[LT] = r1 * sc;
}

// LT: width of one camera's local tangent (6: no intrinsics refined anywhere
// in the problem, 14: up to 8 per camera).  The dense system then has at most
// 6 or kGMaxTangent rows.
template <int LT>
struct GLayout {
  static constexpr int LC = LT + 1;
  static constexpr int NE = LC * (LC + 1) / 2;
  static constexpr int EPL = (NE + 63) / 64;
  static constexpr int NTG = LT == 6 ? 6 : kGMaxTangent;
  static constexpr int NCG = NTG + 1;
  static constexpr int S = NTG + 1;  // row stride of the system
  static constexpr int kSlab = kPoseWaves * LC * kColStride;
  static constexpr int kRed = kGMaxSegs * EPL * 64;
  static constexpr int kFixed = kSlab + kRed + NCG * NCG + kPoseTB + 2 * kGStateDoubles + 12 * kGMaxCams + 3 * 64 +
                                (int)(sizeof(PoseLm) / 8) + (kGMaxCams * kGCamInts + 64 + kGMaxSegs + 1) / 2;
  static_assert(NTG * S <= kSlab, "the system matrix lives in the slabs");
  static constexpr int doubles(int lds_obs) { return kFixed + 5 * lds_obs; }
};
static_assert(GLayout<14>::doubles(kGLdsObs) * 8 <= 160 * 1024, "LDS budget of one workgroup");

template <int LT>
__global__ __launch_bounds__(kPoseTB) void generalized_pose_kernel(GPoseArgs a) {
  using L = GLayout<LT>;
  constexpr int LC = L::LC, NE = L::NE, EPL = L::EPL, NTG = L::NTG, NCG = L::NCG, S = L::S;
  extern __shared__ double lds[];
  double* slab_all = lds;
  double* sA = lds;  // [n][S] system / factor, while no linearization runs
  double* red = slab_all + L::kSlab;  // [segment][EPL * 64]
  double* sM = red + L::kRed;         // [NCG][NCG] symmetric [J r]'[J r], column NTG = r
  double* sCost = sM + NCG * NCG;
  double* sState = sCost + kPoseTB;
  double* sCand = sState + kGStateDoubles;
  double* sRel = sCand + kGStateDoubles;  // [camera][12]
  double* sScale = sRel + 12 * kGMaxCams;
  double* sStep = sScale + 64;
  double* sD0 = sStep + 64;
  PoseLm* lm = reinterpret_cast<PoseLm*>(sD0 + 64);
  int* sCam = reinterpret_cast<int*>(reinterpret_cast<double*>(lm) + sizeof(PoseLm) / 8);  // [camera][kGCamInts]
  int* sTan = sCam + kGMaxCams * kGCamInts;  // tangent column -> index into sState
  int* sSegCam = sTan + 64;
  double* sObs = lds + L::kFixed;
  const PoseLmLds<NCG, S, 64, true> solve{sM, sA, sScale, sStep, sD0, lm, sTan};

  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const GProblemDev* pb = a.prob + blockIdx.x;
  const int count = pb->count, ncam = pb->ncam, n = pb->n, index = pb->index, nseg = pb->nseg, ntiles = pb->ntiles;
  const int nstate = 8 + 8 * ncam;
  const PoseLmOptions opt{a.gradient_tolerance, a.max_num_iterations, a.trace, a.trace_cap, index};
  const GTile* tiles = a.tiles + pb->tile_begin;
  PoseObsSource<true> src;
  src.lds_obs = a.lds_obs;
  src.resident = count <= a.lds_obs;
  src.sx = sObs;
  src.order = a.order + pb->obs_begin;
  src.p2 = a.p2 + pb->raw_begin;
  src.p3 = a.p3 + 3 * pb->raw_begin;
  src.stage(tid, count);
  if (tid < 8) sState[tid] = a.rig[(size_t)index * 8 + tid];
  for (int i = tid; i < 8 * ncam; i += kPoseTB) sState[8 + i] = a.cprm[8 * (size_t)pb->cam_begin + i];
  for (int i = tid; i < ncam * 12; i += kPoseTB) sRel[i] = a.cams[pb->cam_begin + i / 12].rel[i % 12];
  if (tid < ncam) {
    const GCamDev* c = a.cams + pb->cam_begin + tid;
    int* d = sCam + tid * kGCamInts;
    d[0] = c->model; d[1] = c->np; d[2] = c->ct; d[3] = c->off;
    for (int k = 0; k < 8; ++k) d[4 + k] = c->idx[k];
    for (int k = 0; k < c->ct; ++k) sTan[c->off + k] = 8 + 8 * tid + c->idx[k];
  }
  if (tid < nseg) sSegCam[tid] = pb->seg_cam[tid];
  solve.init(tid);
  __syncthreads();

  // the lane's entries of a camera's upper triangle
  int ei[EPL], ej[EPL];
  pose_triangle_entries<LC>(lane, ei, ej);
  const int tile0 = pb->wave_tile[wave], tile1 = pb->wave_tile[wave + 1];

  bool first = true;
  int action = kActAccept;  // the first pass linearizes at the given point
  while (true) {
    if (action == kActAccept) {
      // the cameras' [J r]'[J r] and the cost at sState -> red, sM
      double* slab = slab_all + wave * LC * kColStride;
      for (int i = tid; i < NCG * NCG; i += kPoseTB) sM[i] = 0.0;
      double acc[EPL];
      double cost_acc = 0.0;
      int seg = -1, cam = 0, model = 0, ct = 0;
      int idx[8];
      for (int tile = tile0; tile < tile1; ++tile) {
        const GTile tl = tiles[tile];
        if (tl.seg != seg) {
          if (seg >= 0) {
#pragma unroll
            for (int s = 0; s < EPL; ++s) red[(seg * EPL + s) * 64 + lane] = acc[s];
          }
          seg = tl.seg;
          cam = tl.cam;
          model = sCam[cam * kGCamInts];
          ct = sCam[cam * kGCamInts + 2];
#pragma unroll
          for (int k = 0; k < 8; ++k) idx[k] = sCam[cam * kGCamInts + 4 + k];
#pragma unroll
          for (int s = 0; s < EPL; ++s) acc[s] = 0.0;
        }
        double J0[LC], J1[LC];
#pragma unroll
        for (int c = 0; c < LC; ++c) { J0[c] = 0.0; J1[c] = 0.0; }
        if (lane < tl.count) {
          double ox, oy, X[3], cost;
          src.load(tl.start + lane, &ox, &oy, X);
          gpose_obs_rows<LT>(model, sState, sState + 8 + 8 * cam, sRel + 12 * cam, idx, ct, a.loss_scale, ox, oy, X,
                             J0, J1, &cost);
          cost_acc += cost;
        }
        pose_tile_products<LC>(slab, lane, J0, J1, ei, ej, acc);
      }
      if (seg >= 0) {
#pragma unroll
        for (int s = 0; s < EPL; ++s) red[(seg * EPL + s) * 64 + lane] = acc[s];
      }
      sCost[tid] = cost_acc;
      __syncthreads();
      if (wave == 0) {
        // segments in order: camera major, wave order inside a camera
#pragma unroll
        for (int s = 0; s < EPL; ++s) {
          const int e = lane + 64 * s;
          if (e < NE) {
            const int li = ei[s], lj = ej[s];
            for (int g = 0; g < nseg; ++g) {
              const int* cm = sCam + sSegCam[g] * kGCamInts;
              const int cct = cm[2], off = cm[3];
              const int gi = li < 6 ? li : li < LT ? (li - 6 < cct ? off + li - 6 : -1) : NTG;
              const int gj = lj < 6 ? lj : lj < LT ? (lj - 6 < cct ? off + lj - 6 : -1) : NTG;
              if (gi < 0 || gj < 0) continue;
              const double v = sM[gi * NCG + gj] + red[(g * EPL + s) * 64 + lane];
              sM[gi * NCG + gj] = v;
              sM[gj * NCG + gi] = v;
            }
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
      if (solve.propose(sState, sCand, nstate, n, lane, opt, &model_cost_change)) {
        // |x|^2, |x - candidate|^2 over the variable blocks in ambient
        // coordinates: qvec, tvec, and every parameter of a refined camera
        double xn2 = 0.0, sn2 = 0.0;
        for (int m = 0; m < 7; ++m) {
          const double xv = sState[m], dv = xv - sCand[m];
          xn2 += xv * xv;
          sn2 += dv * dv;
        }
#pragma unroll 1  // rolled, as it compiled inside the kernel's own LM loop
        for (int c = 0; c < ncam; ++c) {
          const int* cm = sCam + c * kGCamInts;
          if (cm[3] < 0 || cm[2] == 0) continue;
          for (int m = 0; m < cm[1]; ++m) {
            const double xv = sState[8 + 8 * c + m], dv = xv - sCand[8 + 8 * c + m];
            xn2 += xv * xv;
            sn2 += dv * dv;
          }
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
      for (int tile = wave; tile < ntiles; tile += kPoseWaves) {
        const GTile tl = tiles[tile];
        if (lane < tl.count) {
          double ox, oy, X[3];
          src.load(tl.start + lane, &ox, &oy, X);
          cost_acc += gpose_obs_cost(sCam[tl.cam * kGCamInts], sCand, sCand + 8 + 8 * tl.cam, sRel + 12 * tl.cam,
                                     a.loss_scale, ox, oy, X);
        }
      }
      sCost[tid] = cost_acc;
    }
    __syncthreads();
    if (wave == 0 && solve.judge(sCost, lane, opt) == kActAccept)
      for (int m = lane; m < nstate; m += 64) sState[m] = sCand[m];
    __syncthreads();
    action = lm->action1;
    if (action == kActStop) break;
  }

  if (wave != 0) return;
  wave_sync();
  solve.finish(n, lane, a.cov, a.out, index);
  if (lm->termination != MI_BA_FAILURE) {
    if (lane < 8) a.rig[(size_t)index * 8 + lane] = sState[lane];
    for (int i = lane; i < 8 * ncam; i += 64) a.cprm[8 * (size_t)pb->cam_begin + i] = sState[8 + i];
  }
}

// Parameters of a model id the reference knows (camera_models.h), -1 otherwise.
int reference_num_params(int model) {
  if (model == 6 || model == 10) return 12;  // FULL_OPENCV, THIN_PRISM_FISHEYE: known, not supported
  return num_params(model);
}

struct GPlan {
  int32_t status = MI_BA_OK;
  int32_t tangent = 0;  // 6 + refined intrinsics of the cameras with inliers; 0 without inliers
  int64_t inliers = 0;
  std::vector<int32_t> cam_count;  // inliers per camera
};

// Argument checks of the call (the reference's CHECKs) and the per-problem
// plan.  Host only.
mi_ba_status generalized_pose_plan(const mi_ba_pose_refine_options* o, const mi_ba_generalized_pose_batch* b,
                                   std::vector<GPlan>* plans) {
  if (!o || !b || b->num_problems < 0) return MI_BA_ERR_INVALID_ARGUMENT;
  if (!pose_options_check(o->gradient_tolerance, o->max_num_iterations, o->loss_function_scale))
    return MI_BA_ERR_INVALID_ARGUMENT;
  const int n = b->num_problems;
  plans->assign(n, GPlan());
  if (n == 0) return MI_BA_OK;
  if (!b->obs_offsets || !b->camera_offsets || !b->camera_model_ids || !b->camera_param_offsets || !b->camera_params ||
      !b->rig_qvecs || !b->rig_tvecs || !b->qvec || !b->tvec)
    return MI_BA_ERR_INVALID_ARGUMENT;
  if (b->obs_offsets[0] < 0 || b->camera_offsets[0] < 0) return MI_BA_ERR_INVALID_ARGUMENT;
  for (int k = 0; k < n; ++k) {
    const int64_t c = b->obs_offsets[k + 1] - b->obs_offsets[k];
    const int64_t nc = b->camera_offsets[k + 1] - b->camera_offsets[k];
    if (c < 0 || c > INT32_MAX || nc < 0 || nc > INT32_MAX) return MI_BA_ERR_INVALID_ARGUMENT;
  }
  const int64_t total = b->obs_offsets[n], cams0 = b->camera_offsets[0], cams1 = b->camera_offsets[n];
  if (total > b->obs_offsets[0] && (!b->points2D || !b->points3D || !b->camera_idxs)) return MI_BA_ERR_INVALID_ARGUMENT;
  if (cams1 > cams0 && b->camera_param_offsets[cams0] < 0) return MI_BA_ERR_INVALID_ARGUMENT;
  for (int64_t c = cams0; c < cams1; ++c) {
    const int64_t have = b->camera_param_offsets[c + 1] - b->camera_param_offsets[c];
    const int np = reference_num_params(b->camera_model_ids[c]);
    if (have < 0 || (np >= 0 && have != np)) return MI_BA_ERR_INVALID_ARGUMENT;
  }
  for (int k = 0; k < n; ++k) {
    GPlan& p = (*plans)[k];
    const int64_t c0 = b->camera_offsets[k], nc = b->camera_offsets[k + 1] - c0;
    p.cam_count.assign((size_t)nc, 0);
    for (int64_t i = b->obs_offsets[k]; i < b->obs_offsets[k + 1]; ++i) {
      const int32_t ci = b->camera_idxs[i];
      // CHECK_GE(min camera_idxs, 0), CHECK_LT(max camera_idxs, cameras->size()): outliers included
      if (ci < 0 || ci >= nc) return MI_BA_ERR_INVALID_ARGUMENT;
      if (b->inlier_mask && !b->inlier_mask[i]) continue;
      p.cam_count[ci] += 1;
      p.inliers += 1;
    }
    if (p.inliers == 0) continue;
    int tangent = 6;
    for (int64_t c = 0; c < nc; ++c) {
      if (p.cam_count[c] == 0) continue;
      const int ct = mi_ba_pose_refine_intrinsics(b->camera_model_ids[c0 + c], o->refine_focal_length,
                                                  o->refine_extra_params, nullptr);
      if (ct < 0) {
        p.status = MI_BA_ERR_UNSUPPORTED;
        tangent = -1;
        break;
      }
      tangent += ct;
    }
    p.tangent = tangent;
    if (nc > kGMaxCams || tangent > kGMaxTangent) p.status = MI_BA_ERR_UNSUPPORTED;
  }
  return MI_BA_OK;
}

}  // namespace
}  // namespace miba

using namespace miba;

extern "C" void mi_ba_generalized_pose_limits(int32_t* max_cameras, int32_t* max_tangent, int32_t* lds_capacity) {
  if (max_cameras) *max_cameras = kGMaxCams;
  if (max_tangent) *max_tangent = kGMaxTangent;
  if (lds_capacity) *lds_capacity = kGLdsObs;
}

extern "C" mi_ba_status mi_ba_generalized_pose_plan(const mi_ba_pose_refine_options* o,
                                                    const mi_ba_generalized_pose_batch* b, int32_t* statuses,
                                                    int32_t* tangent_sizes, int64_t* inlier_counts) {
  std::vector<GPlan> plans;
  const mi_ba_status st = generalized_pose_plan(o, b, &plans);
  if (st != MI_BA_OK) return st;
  for (size_t k = 0; k < plans.size(); ++k) {
    if (statuses) statuses[k] = plans[k].status;
    if (tangent_sizes) tangent_sizes[k] = plans[k].tangent;
    if (inlier_counts) inlier_counts[k] = plans[k].inliers;
  }
  return MI_BA_OK;
}

extern "C" mi_ba_status mi_ba_refine_generalized_absolute_pose_batch(const mi_ba_pose_refine_options* o,
                                                                     const mi_ba_generalized_pose_batch* b,
                                                                     int32_t* statuses, mi_ba_summary* summaries,
                                                                     int32_t* usable) {
  std::vector<GPlan> plans;
  mi_ba_status st = generalized_pose_plan(o, b, &plans);
  if (st != MI_BA_OK) return st;
  const int n = b->num_problems;
  if (n == 0) return MI_BA_OK;
  if (!statuses || !summaries || !usable) return MI_BA_ERR_INVALID_ARGUMENT;
  st = pose_select_device(o->device);
  if (st != MI_BA_OK) return st;

  // Host assembly: the inliers listed stably grouped by camera, tiles, wave
  // runs and segments, unit quaternions, refined-intrinsics sets.
  const int64_t ncams_all = b->camera_offsets[n] - b->camera_offsets[0], cam_base = b->camera_offsets[0];
  std::vector<GProblemDev> narrow, wide;
  std::vector<GCamDev> cams((size_t)ncams_all);
  std::vector<GTile> tiles;
  std::vector<double> rig(8 * (size_t)n, 0.0), cprm(8 * (size_t)ncams_all, 0.0);
  std::vector<int64_t> cursor;
  const int64_t raw0 = b->obs_offsets[0], raw_total = b->obs_offsets[n] - raw0;
  int64_t listed = 0;
  for (const GPlan& plan : plans)
    if (plan.status == MI_BA_OK) listed += plan.inliers;
  std::vector<int32_t> order((size_t)listed);
  int64_t order_at = 0;
  for (int k = 0; k < n; ++k) {
    std::memset(&summaries[k], 0, sizeof(mi_ba_summary));
    usable[k] = 0;
    const GPlan& plan = plans[k];
    statuses[k] = plan.status;
    if (plan.status != MI_BA_OK) continue;
    summaries[k].num_residuals_reduced = 2 * plan.inliers;
    summaries[k].num_effective_parameters_reduced = plan.tangent;
    if (plan.inliers == 0) {  // no residuals: nothing to do
      summaries[k].termination_type = MI_BA_CONVERGENCE;
      usable[k] = 1;
      continue;
    }
    const int64_t c0 = b->camera_offsets[k];
    const int ncam = (int)(b->camera_offsets[k + 1] - c0);
    GProblemDev pb{};
    pb.index = k;
    pb.ncam = ncam;
    pb.n = plan.tangent;
    pb.count = (int32_t)plan.inliers;
    pb.obs_begin = order_at;
    pb.raw_begin = b->obs_offsets[k] - raw0;
    pb.tile_begin = (int64_t)tiles.size();
    pb.cam_begin = c0 - cam_base;
    pose_unit_quat_copy(b->qvec + 4 * (size_t)k, &rig[8 * (size_t)k]);
    for (int m = 0; m < 3; ++m) rig[8 * (size_t)k + 4 + m] = b->tvec[3 * (size_t)k + m];
    // cameras: tangent offsets, relative poses, grouped positions
    cursor.assign((size_t)ncam, 0);
    int off = 6;
    int64_t pos = 0;
    for (int c = 0; c < ncam; ++c) {
      GCamDev& cd = cams[(size_t)(pb.cam_begin + c)];
      cd = GCamDev{};
      cd.off = -1;
      cursor[c] = pos;
      const int cnt = plan.cam_count[c];
      if (cnt == 0) continue;
      const int model = b->camera_model_ids[c0 + c];
      cd.model = model;
      cd.np = num_params(model);
      cd.ct = mi_ba_pose_refine_intrinsics(model, o->refine_focal_length, o->refine_extra_params, cd.idx);
      cd.off = off;
      off += cd.ct;
      double qr[4];
      pose_unit_quat_copy(b->rig_qvecs + 4 * (size_t)(c0 + c), qr);
      unit_quat_matrix(qr, cd.rel);
      for (int m = 0; m < 3; ++m) cd.rel[9 + m] = b->rig_tvecs[3 * (size_t)(c0 + c) + m];
      for (int m = 0; m < cd.np; ++m) cprm[8 * (size_t)(pb.cam_begin + c) + m] = b->camera_params[b->camera_param_offsets[c0 + c] + m];
      for (int s = 0; s < cnt; s += 64) tiles.push_back(GTile{c, (int32_t)(pos + s), cnt - s < 64 ? cnt - s : 64, 0});
      pos += cnt;
    }
    for (int64_t i = b->obs_offsets[k]; i < b->obs_offsets[k + 1]; ++i) {
      if (b->inlier_mask && !b->inlier_mask[i]) continue;
      order[(size_t)(order_at + cursor[b->camera_idxs[i]]++)] = (int32_t)(i - b->obs_offsets[k]);
    }
    order_at += plan.inliers;
    // four contiguous runs of tiles, one per wave; a segment is a camera's run inside a wave
    pb.ntiles = (int32_t)((int64_t)tiles.size() - pb.tile_begin);
    for (int w = 0; w <= kPoseWaves; ++w) pb.wave_tile[w] = (int32_t)((int64_t)w * pb.ntiles / kPoseWaves);
    int seg = -1, wv = 0, last_cam = -1, last_wave = -1;
    for (int t = 0; t < pb.ntiles; ++t) {
      while (t >= pb.wave_tile[wv + 1]) ++wv;
      GTile& tl = tiles[(size_t)pb.tile_begin + t];
      if (tl.cam != last_cam || wv != last_wave) {
        ++seg;
        pb.seg_cam[seg] = tl.cam;
        last_cam = tl.cam;
        last_wave = wv;
      }
      tl.seg = seg;
    }
    pb.nseg = seg + 1;
    (pb.n == 6 ? narrow : wide).push_back(pb);
  }
  if (narrow.empty() && wide.empty()) return MI_BA_OK;

  const int64_t N = raw_total;
  Buf bufs[9];
  double2* d2 = bufs[0].alloc<double2>(N);
  double* d3 = bufs[1].alloc<double>(3 * (size_t)N);
  int32_t* dorder = bufs[8].alloc<int32_t>(order.size());
  double* drig = bufs[2].alloc<double>(rig.size());
  double* dprm = bufs[3].alloc<double>(cprm.size());
  double* dout = bufs[4].alloc<double>(kOutStride * (size_t)n);
  double* dcov = b->rot_tvec_covariance ? bufs[5].alloc<double>(36 * (size_t)n) : nullptr;
  GCamDev* dcams = bufs[6].alloc<GCamDev>(cams.size());
  GTile* dtiles = bufs[7].alloc<GTile>(tiles.size());
  if (!d2 || !d3 || !dorder || !drig || !dprm || !dout || !dcams || !dtiles || (b->rot_tvec_covariance && !dcov))
    return MI_BA_ERR_OUT_OF_MEMORY;
  if (hipMemcpy(d2, b->points2D + 2 * raw0, (size_t)N * 16, hipMemcpyHostToDevice) != hipSuccess ||
      hipMemcpy(d3, b->points3D + 3 * raw0, (size_t)N * 24, hipMemcpyHostToDevice) != hipSuccess ||
      hipMemcpy(dorder, order.data(), order.size() * 4, hipMemcpyHostToDevice) != hipSuccess ||
      hipMemcpy(drig, rig.data(), rig.size() * 8, hipMemcpyHostToDevice) != hipSuccess ||
      hipMemcpy(dprm, cprm.data(), cprm.size() * 8, hipMemcpyHostToDevice) != hipSuccess ||
      hipMemcpy(dcams, cams.data(), cams.size() * sizeof(GCamDev), hipMemcpyHostToDevice) != hipSuccess ||
      hipMemcpy(dtiles, tiles.data(), tiles.size() * sizeof(GTile), hipMemcpyHostToDevice) != hipSuccess ||
      hipMemset(dout, 0, kOutStride * (size_t)n * 8) != hipSuccess)
    return MI_BA_ERR_HIP;
  GPoseArgs a{};
  a.cams = dcams;
  a.tiles = dtiles;
  a.order = dorder;
  a.p2 = d2;
  a.p3 = d3;
  a.rig = drig;
  a.cprm = dprm;
  a.out = dout;
  a.cov = dcov;
  a.gradient_tolerance = o->gradient_tolerance;
  a.loss_scale = o->loss_function_scale;
  a.max_num_iterations = o->max_num_iterations;
  PoseTraceBuf trace;
  st = trace.setup(n);
  if (st != MI_BA_OK) return st;
  a.trace = trace.dev;
  a.trace_cap = trace.cap;
  // specialised on a camera's tangent width: rig pose only (6), and rig pose + up to 8 intrinsics (14)
  Buf pbufs[2];
  st = pose_launch(&generalized_pose_kernel<6>, &GLayout<6>::doubles, kGLdsObs, a, narrow, &pbufs[0]);
  if (st != MI_BA_OK) return st;
  st = pose_launch(&generalized_pose_kernel<14>, &GLayout<14>::doubles, kGLdsObs, a, wide, &pbufs[1]);
  if (st != MI_BA_OK) return st;
  if (hipStreamSynchronize(0) != hipSuccess) return MI_BA_ERR_HIP;
  std::vector<double> out(kOutStride * (size_t)n), cov(dcov ? 36 * (size_t)n : 0);
  if (!pose_download(&rig, drig) || !pose_download(&cprm, dprm) || !pose_download(&out, dout) ||
      (dcov && !pose_download(&cov, dcov)))
    return MI_BA_ERR_HIP;
  if (trace.download() != MI_BA_OK) return MI_BA_ERR_HIP;
  auto finish = [&](const GProblemDev& pb) {
    const int k = pb.index;
    const double* r = &out[kOutStride * (size_t)k];
    bool ok = pose_summary_fill(r, &summaries[k]);
    if (ok) {
      for (int m = 0; m < 4; ++m) b->qvec[4 * (size_t)k + m] = rig[8 * (size_t)k + m];
      for (int m = 0; m < 3; ++m) b->tvec[3 * (size_t)k + m] = rig[8 * (size_t)k + 4 + m];
      for (int c = 0; c < pb.ncam; ++c) {
        const GCamDev& cd = cams[(size_t)(pb.cam_begin + c)];
        if (cd.off < 0) continue;  // a camera without inliers is not in the problem
        double* dst = b->camera_params + b->camera_param_offsets[cam_base + pb.cam_begin + c];
        for (int m = 0; m < cd.ct; ++m) dst[cd.idx[m]] = cprm[8 * (size_t)(pb.cam_begin + c) + cd.idx[m]];
      }
      if (dcov) {
        if (r[5] != 0.0)
          std::memcpy(b->rot_tvec_covariance + 36 * (size_t)k, &cov[36 * (size_t)k], 36 * 8);
        else
          ok = false;  // covariance.Compute failed (pose.cc:495-497)
      }
    }
    usable[k] = ok ? 1 : 0;
  };
  for (const GProblemDev& pb : narrow) finish(pb);
  for (const GProblemDev& pb : wide) finish(pb);
  return MI_BA_OK;
}
