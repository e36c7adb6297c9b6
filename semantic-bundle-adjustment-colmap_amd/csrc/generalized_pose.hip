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

__device__ __forceinline__ void gpose_trace(const GPoseArgs& a, int index, int it, int valid, int successful, int end) {
  if (a.trace && it >= 1 && it <= a.trace_cap)
    a.trace[(size_t)index * a.trace_cap + it - 1] = (uint8_t)(valid | successful << 1 | end << 2);
}

struct GObsSource {
  const double* sx;      // LDS, SoA in grouped order (resident) ...
  const int32_t* order;  // ... or device memory through the grouped list
  const double2* p2;
  const double* p3;
  bool resident;
  int lds_obs;
  __device__ __forceinline__ void load(int i, double* ox, double* oy, double X[3]) const {
    if (resident) {
      *ox = sx[i];
      *oy = sx[lds_obs + i];
      X[0] = sx[2 * lds_obs + i];
      X[1] = sx[3 * lds_obs + i];
      X[2] = sx[4 * lds_obs + i];
    } else {
      const size_t j = (size_t)order[i];
      const double2 o = p2[j];
      *ox = o.x;
      *oy = o.y;
      X[0] = p3[3 * j];
      X[1] = p3[3 * j + 1];
      X[2] = p3[3 * j + 2];
    }
  }
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

// Dense Cholesky by one wave, in LDS: lane i < n owns row i of the lower
// triangle in sA (row stride S); on return sA holds L.  A pivot k with
// !(pivot > tol * d0[k]) makes the result false.
__device__ inline bool gwave_cholesky(double* sA, int S, int n, int lane, double tol, const double* d0) {
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

// Solves L L' x = b with L in sA: lane i < n passes b_i and receives x_i.
__device__ inline double gwave_chol_solve(const double* sA, int S, int n, double b, int lane, double* sx) {
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

  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const GProblemDev* pb = a.prob + blockIdx.x;
  const int count = pb->count, ncam = pb->ncam, n = pb->n, index = pb->index, nseg = pb->nseg, ntiles = pb->ntiles;
  const int nstate = 8 + 8 * ncam;
  double* out = a.out + (size_t)index * kOutStride;
  const GTile* tiles = a.tiles + pb->tile_begin;
  GObsSource src;
  src.lds_obs = a.lds_obs;
  src.resident = count <= a.lds_obs;
  src.sx = sObs;
  src.order = a.order + pb->obs_begin;
  src.p2 = a.p2 + pb->raw_begin;
  src.p3 = a.p3 + 3 * pb->raw_begin;
  if (src.resident) {
    for (int i = tid; i < count; i += kPoseTB) {
      const size_t j = (size_t)src.order[i];
      const double2 o = src.p2[j];
      sObs[i] = o.x;
      sObs[a.lds_obs + i] = o.y;
      sObs[2 * a.lds_obs + i] = src.p3[3 * j];
      sObs[3 * a.lds_obs + i] = src.p3[3 * j + 1];
      sObs[4 * a.lds_obs + i] = src.p3[3 * j + 2];
    }
  }
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
  if (tid == 0) {
    lm->radius = kInitialRadius;
    lm->decrease_factor = 2.0;
    lm->iteration = 0;
    lm->consecutive_invalid = 0;
    lm->n_successful = 0;
    lm->n_unsuccessful = 0;
    lm->termination = MI_BA_NO_CONVERGENCE;
    lm->last_successful = 1;  // iteration 0 counts as successful (IterationZero)
  }
  __syncthreads();

  // the lane's entries (i, j), i <= j < LC, of a camera's upper triangle
  int ei[EPL], ej[EPL];
#pragma unroll
  for (int s = 0; s < EPL; ++s) {
    int e = lane + 64 * s, i = 0, w = LC;
    if (e >= NE) e = 0;  // idle slot: sums entry 0, never stored
    while (e >= w) { e -= w; --w; ++i; }
    ei[s] = i;
    ej[s] = i + e;
  }
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
        {
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
#pragma unroll
          for (int c = 0; c < LC; ++c) {
            slab[c * kColStride + lane] = J0[c];
            slab[c * kColStride + 64 + lane] = J1[c];
          }
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
        if (first) {
          sScale[lane] = lane < n ? 1.0 / (1.0 + sqrt(sM[lane * NCG + lane])) : 1.0;
          if (lane == 0) {
            lm->x_cost = total;
            lm->initial_cost = total;
          }
          wave_sync();
        }
      }
      first = false;
    }

    if (wave == 0) {
      int act = kActStop;
      // a non-finite initial cost: FAILURE, parameters untouched
      bool go = isfinite(lm->x_cost);
      if (!go && lane == 0) lm->termination = MI_BA_FAILURE;
      while (go) {
        // FinalizeIterationAndCheckIfMinimizerCanContinue
        if (lm->iteration >= a.max_num_iterations) {
          if (lane == 0) lm->termination = MI_BA_NO_CONVERGENCE;
          break;
        }
        if (lm->last_successful) {
          // GradientToleranceReached: |x - Plus(x, -g)|_inf, g = J'r
          const double d[3] = {-sM[0 * NCG + NTG], -sM[1 * NCG + NTG], -sM[2 * NCG + NTG]};
          const double q[4] = {sState[0], sState[1], sState[2], sState[3]};
          double qn[4], gmax = 0.0;
          quat_plus(q, d, qn);
#pragma unroll
          for (int m = 0; m < 4; ++m) gmax = fmax(gmax, fabs(q[m] - qn[m]));
          for (int m = 0; m < 3; ++m)
            gmax = fmax(gmax, fabs(sState[4 + m] - (sState[4 + m] + -sM[(3 + m) * NCG + NTG])));
          for (int m = 6; m < n; ++m) {
            const double xv = sState[sTan[m]];
            gmax = fmax(gmax, fabs(xv - (xv + -sM[m * NCG + NTG])));
          }
          if (gmax <= a.gradient_tolerance) {
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
        // row `lane` of the scaled, damped system; LM diagonal: the clipped
        // scaled column norm over the radius
        const double scale = sScale[lane];
        double gs = 0.0;
        if (lane < n) {
          for (int j = 0; j <= lane; ++j) {
            double v = sM[lane * NCG + j] * scale * sScale[j];
            if (j == lane) v = v + fmin(fmax(v, 1e-6), 1e32) / radius;
            sA[lane * S + j] = v;
          }
          sD0[lane] = 1.0;
          gs = sM[lane * NCG + NTG] * scale;
        }
        bool ok = gwave_cholesky(sA, S, n, lane, 0.0, sD0);
        double step = 0.0, model = 0.0;
        if (ok) {
          // Ceres solves (J'J + D'D) x = J'r, step = -x
          step = -gwave_chol_solve(sA, S, n, gs, lane, sStep);
          sStep[lane] = lane < n ? step : 0.0;
          wave_sync();
          double term = 0.0;
          if (lane < n) {
            double hstep = 0.0;
            for (int j = 0; j < n; ++j) hstep += sM[lane * NCG + j] * scale * sScale[j] * sStep[j];
            term = step * (gs + 0.5 * hstep);
          }
          model = -wave_sum_fixed(term);
          ok = isfinite(model) && model > 0.0;
        }
        if (!ok) {
          const int inv = lm->consecutive_invalid + 1;
          const double df = lm->decrease_factor;
          wave_sync();
          if (lane == 0) {
            lm->last_successful = 0;
            lm->consecutive_invalid = inv;
            lm->n_unsuccessful += 1;
            lm->radius = radius / df;
            lm->decrease_factor = df * 2.0;
            if (inv > kMaxConsecutiveInvalid) lm->termination = MI_BA_FAILURE;
            gpose_trace(a, index, lm->iteration, 0, 0, inv > kMaxConsecutiveInvalid ? 1 : 0);
          }
          wave_sync();
          if (inv > kMaxConsecutiveInvalid) break;
          continue;
        }
        // candidate = Plus(x, step * scale)
        const double delta = step * scale;
        for (int m = lane; m < nstate; m += 64) sCand[m] = sState[m];
        sStep[lane] = lane < n ? delta : 0.0;
        wave_sync();
        {
          const double dq[3] = {sStep[0], sStep[1], sStep[2]};
          const double q[4] = {sState[0], sState[1], sState[2], sState[3]};
          double qn[4];
          quat_plus(q, dq, qn);
          if (lane < 4) sCand[lane] = lane == 0 ? qn[0] : lane == 1 ? qn[1] : lane == 2 ? qn[2] : qn[3];
          if (lane >= 3 && lane < 6) sCand[1 + lane] = sState[1 + lane] + delta;
          if (lane >= 6 && lane < n) sCand[sTan[lane]] = sState[sTan[lane]] + delta;
        }
        wave_sync();
        // |x|^2, |x - candidate|^2 over the variable blocks in ambient
        // coordinates: qvec, tvec, and every parameter of a refined camera
        double xn2 = 0.0, sn2 = 0.0;
        for (int m = 0; m < 7; ++m) {
          const double xv = sState[m], dv = xv - sCand[m];
          xn2 += xv * xv;
          sn2 += dv * dv;
        }
        for (int c = 0; c < ncam; ++c) {
          const int* cm = sCam + c * kGCamInts;
          if (cm[3] < 0 || cm[2] == 0) continue;
          for (int m = 0; m < cm[1]; ++m) {
            const double xv = sState[8 + 8 * c + m], dv = xv - sCand[8 + 8 * c + m];
            xn2 += xv * xv;
            sn2 += dv * dv;
          }
        }
        if (lane == 0) {
          lm->consecutive_invalid = 0;
          lm->model_cost_change = model;
          lm->x_norm = sqrt(xn2);
          lm->step_norm = sqrt(sn2);
        }
        act = kActEval;
        break;
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
    if (wave == 0) {
      const double cand_cost = pose_cost_total(sCost, lane);
      const double x_cost = lm->x_cost, radius = lm->radius, df = lm->decrease_factor;
      const double cost_change = x_cost - cand_cost;
      const double relative_decrease = cost_change / lm->model_cost_change;
      const bool success = isfinite(cand_cost) && relative_decrease > kMinRelativeDecrease;
      // ParameterToleranceReached / FunctionToleranceReached: Ceres returns
      // before accepting the candidate
      const bool tol = lm->step_norm <= kParameterTolerance * (lm->x_norm + kParameterTolerance) ||
                       fabs(cost_change) <= kFunctionTolerance * x_cost;
      wave_sync();
      if (tol) {
        if (lane == 0) {
          lm->n_unsuccessful += 1;
          lm->termination = MI_BA_CONVERGENCE;
          lm->action1 = kActStop;
          gpose_trace(a, index, lm->iteration, 1, 0, 1);
        }
      } else if (success) {
        for (int m = lane; m < nstate; m += 64) sState[m] = sCand[m];
        if (lane == 0) {
          lm->n_successful += 1;
          lm->last_successful = 1;
          lm->x_cost = cand_cost;
          lm->radius = fmin(kMaxRadius, radius / fmax(1.0 / 3.0, 1.0 - pow(2.0 * relative_decrease - 1.0, 3.0)));
          lm->decrease_factor = 2.0;
          lm->action1 = kActAccept;
          gpose_trace(a, index, lm->iteration, 1, 1, 0);
        }
      } else {
        if (lane == 0) {
          lm->n_unsuccessful += 1;
          lm->last_successful = 0;
          lm->radius = radius / df;
          lm->decrease_factor = df * 2.0;
          lm->action1 = kActReject;
          gpose_trace(a, index, lm->iteration, 1, 0, 0);
        }
      }
    }
    __syncthreads();
    action = lm->action1;
    if (action == kActStop) break;
  }

  if (wave != 0) return;
  wave_sync();
  const int termination = lm->termination;
  // rot_tvec_covariance: rig-pose block of inv(J'J) at the final point (sM)
  double cov_ok = 0.0;
  if (a.cov && termination != MI_BA_FAILURE) {
    if (lane < n) {
      for (int j = 0; j <= lane; ++j) sA[lane * S + j] = sM[lane * NCG + j];
      sD0[lane] = sM[lane * NCG + lane];
    }
    if (gwave_cholesky(sA, S, n, lane, kCovPivotTolerance, sD0)) {
      cov_ok = 1.0;
      double* cov = a.cov + (size_t)index * 36;
#pragma unroll 1
      for (int c = 0; c < 6; ++c) {
        const double x = gwave_chol_solve(sA, S, n, lane == c ? 1.0 : 0.0, lane, sStep);
        if (lane < 6) cov[lane * 6 + c] = x;
      }
    }
  }
  if (termination != MI_BA_FAILURE) {
    if (lane < 8) a.rig[(size_t)index * 8 + lane] = sState[lane];
    for (int i = lane; i < 8 * ncam; i += 64) a.cprm[8 * (size_t)pb->cam_begin + i] = sState[8 + i];
  }
  if (lane == 0) {
    out[0] = lm->initial_cost;
    out[1] = lm->x_cost;
    out[2] = lm->n_successful;
    out[3] = lm->n_unsuccessful;
    out[4] = termination;
    out[5] = cov_ok;
  }
}

template <int LT>
mi_ba_status launch_generalized_pose(GPoseArgs a, const std::vector<GProblemDev>& list, Buf* buf) {
  if (list.empty()) return MI_BA_OK;
  int most = 0;
  for (const GProblemDev& pb : list) most = pb.count > most ? pb.count : most;
  a.lds_obs = most > kGLdsObs ? kGLdsObs : (most + 63) / 64 * 64;
  GProblemDev* d = buf->alloc<GProblemDev>(list.size());
  if (!d) return MI_BA_ERR_OUT_OF_MEMORY;
  if (hipMemcpy(d, list.data(), list.size() * sizeof(GProblemDev), hipMemcpyHostToDevice) != hipSuccess)
    return MI_BA_ERR_HIP;
  a.prob = d;
  const size_t bytes = (size_t)GLayout<LT>::doubles(a.lds_obs) * 8;
  if (hipFuncSetAttribute(reinterpret_cast<const void*>(&generalized_pose_kernel<LT>),
                          hipFuncAttributeMaxDynamicSharedMemorySize, (int)bytes) != hipSuccess)
    return MI_BA_ERR_HIP;
  hipLaunchKernelGGL(generalized_pose_kernel<LT>, dim3((unsigned)list.size()), dim3(kPoseTB), bytes, 0, a);
  return hipGetLastError() == hipSuccess ? MI_BA_OK : MI_BA_ERR_HIP;
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
  // AbsolutePoseRefinementOptions::Check (pose.h:119-123)
  if (!(o->gradient_tolerance >= 0.0) || o->max_num_iterations < 0 || !(o->loss_function_scale >= 0.0))
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

void unit_quat_copy(const double* q, double* dst) {
  const double nq = std::sqrt(q[0] * q[0] + q[1] * q[1] + q[2] * q[2] + q[3] * q[3]);
  // a unit quaternion is kept bit for bit
  const bool unit = quat_is_unit(q);
  for (int m = 0; m < 4; ++m) dst[m] = unit ? q[m] : q[m] / nq;
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
  int ndev = 0;
  if (hipGetDeviceCount(&ndev) != hipSuccess || ndev == 0) return MI_BA_ERR_NO_DEVICE;
  if (o->device < 0 || o->device >= ndev) return MI_BA_ERR_INVALID_ARGUMENT;
  if (hipSetDevice(o->device) != hipSuccess) return MI_BA_ERR_HIP;

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
    unit_quat_copy(b->qvec + 4 * (size_t)k, &rig[8 * (size_t)k]);
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
      unit_quat_copy(b->rig_qvecs + 4 * (size_t)(c0 + c), qr);
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
  Buf bufs[10];
  double2* d2 = bufs[0].alloc<double2>(N);
  double* d3 = bufs[1].alloc<double>(3 * (size_t)N);
  int32_t* dorder = bufs[9].alloc<int32_t>(order.size());
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
  uint8_t* trace = nullptr;
  int32_t trace_cap = 0;
  pose_trace_target(&trace, &trace_cap);
  if (trace) {
    a.trace = bufs[8].alloc<uint8_t>((size_t)n * trace_cap);
    a.trace_cap = trace_cap;
    if (!a.trace) return MI_BA_ERR_OUT_OF_MEMORY;
    if (hipMemset(a.trace, 0xFF, (size_t)n * trace_cap) != hipSuccess) return MI_BA_ERR_HIP;
  }
  // specialised on a camera's tangent width: rig pose only (6), and rig pose + up to 8 intrinsics (14)
  Buf pbufs[2];
  st = launch_generalized_pose<6>(a, narrow, &pbufs[0]);
  if (st != MI_BA_OK) return st;
  st = launch_generalized_pose<14>(a, wide, &pbufs[1]);
  if (st != MI_BA_OK) return st;
  if (hipStreamSynchronize(0) != hipSuccess) return MI_BA_ERR_HIP;
  std::vector<double> out(kOutStride * (size_t)n), cov;
  if (hipMemcpy(rig.data(), drig, rig.size() * 8, hipMemcpyDeviceToHost) != hipSuccess ||
      hipMemcpy(cprm.data(), dprm, cprm.size() * 8, hipMemcpyDeviceToHost) != hipSuccess ||
      hipMemcpy(out.data(), dout, out.size() * 8, hipMemcpyDeviceToHost) != hipSuccess)
    return MI_BA_ERR_HIP;
  if (trace && hipMemcpy(trace, a.trace, (size_t)n * trace_cap, hipMemcpyDeviceToHost) != hipSuccess)
    return MI_BA_ERR_HIP;
  if (dcov) {
    cov.resize(36 * (size_t)n);
    if (hipMemcpy(cov.data(), dcov, cov.size() * 8, hipMemcpyDeviceToHost) != hipSuccess) return MI_BA_ERR_HIP;
  }
  auto finish = [&](const GProblemDev& pb) {
    const int k = pb.index;
    const double* r = &out[kOutStride * (size_t)k];
    mi_ba_summary& s = summaries[k];
    s.initial_cost = r[0];
    s.final_cost = r[1];
    s.num_successful_steps = (int32_t)r[2];
    s.num_unsuccessful_steps = (int32_t)r[3];
    s.termination_type = (int32_t)r[4];
    s.num_jacobian_evaluations = 1 + s.num_successful_steps;
    s.num_linear_solver_iterations = s.num_successful_steps + s.num_unsuccessful_steps;
    // Ceres leaves the user's parameter blocks untouched on FAILURE
    bool ok = s.termination_type == MI_BA_CONVERGENCE || s.termination_type == MI_BA_NO_CONVERGENCE ||
              s.termination_type == MI_BA_USER_SUCCESS;
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
