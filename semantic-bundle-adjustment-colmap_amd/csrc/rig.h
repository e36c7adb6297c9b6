// rig.h — projection of the reduced camera system onto camera-rig parameters
// (product code; kernels in rig.hip).
//
// A rig image's pose is the concatenation of its snapshot's rig pose and its
// camera's relative pose (RigBundleAdjustmentCostFunction,
// src/base/cost_functions.h:160-214), so its tangent is linear in theirs:
// d_img(i) = A_i d_owner(i) + B_i d_rel(i).  Stacked as T (identity on the
// images of no rig and on the intrinsics), the rig problem's reduced camera
// system is S_rig = T^T S_img T, b_rig = T^T b_img.
//
// Layouts.  Per-image: 6 I pose unknowns, then nc intrinsics.  Rig: 6 per
// slot (snapshot poses, poses of images in no rig, variable relative poses;
// the set-up chooses the numbering), then the same nc intrinsics.  Both
// matrices follow S's conventions: upper triangle, row-major.
#pragma once

#include <hip/hip_runtime.h>

#include <cstdint>
#include <vector>

#include "../../include/mi_ba.h"
#include "context.h"

namespace miba {

// Lanes of a wave, the member pairs of one pass of rig_project_kernel's
// member-pair loop, and the member pairs one workgroup sums: an output block with more is split into chunks
// of this many, summed per chunk and combined in chunk order.
constexpr int kRigLanes = 64;
constexpr int kRigPairsPerPass = 32;  // two lanes per member pair
constexpr int kRigChunkPairs = 1024;

struct RigItem {       // one workgroup of rig_project_kernel
  int32_t a, b;        // output block (slot a, slot b), a <= b
  int32_t first;       // first member pair (row-major over members(a) x members(b))
  int32_t count;       // member pairs (<= kRigChunkPairs)
  int32_t part;        // partial-sum slot, -1: the block's only chunk, written to S_rig
  int32_t pad;
};

struct RigDest {       // an output block summed from several chunks
  int32_t a, b;
  int32_t first;       // first partial-sum slot
  int32_t count;
};

// Device tables of one T.  Built once per problem structure; the 72-double
// image records (A_i, B_i row-major) are refreshed per linearization.
struct RigPlan {
  int num_images = 0, num_intrinsics = 0, num_slots = 0;
  DevArray<int32_t> slot_off;   // [num_slots + 1] into members
  DevArray<int2> members;       // (image, record offset 72 i + 36 which), image order per slot
  DevArray<RigItem> items;
  DevArray<RigDest> dests;
  DevArray<double> part;        // [partial slots][36]
  DevArray<double> rec;         // [num_images][72]
  int64_t n_img() const { return 6 * (int64_t)num_images + num_intrinsics; }
  int64_t n_rig() const { return 6 * (int64_t)num_slots + num_intrinsics; }
};

// Validates the table and uploads the plan (synchronous copies on `s`).
mi_ba_status rig_plan_build(const mi_ba_rig_table& t, hipStream_t s, RigPlan* plan);

// S_rig = T^T S_img T (upper triangle; the rest of S_rig is not touched) and,
// with b_img, b_rig = T^T b_img.  Reads S_img's upper triangle only.  Device
// pointers; asynchronous on `s`.  No floating-point atomics: every sum runs
// in a fixed order, so the result is bitwise repeatable.
// The two halves of launch_rig_project: the pose x pose blocks (and their
// chunk combine), then the pose x intrinsics strips, b_rig and the intrinsics.
hipError_t launch_rig_project_blocks(RigPlan& plan, const double* S_img, int64_t ld_img, double* S_rig,
                                     int64_t ld_rig, hipStream_t s);
hipError_t launch_rig_project_tail(RigPlan& plan, const double* S_img, int64_t ld_img, const double* b_img,
                                   double* S_rig, int64_t ld_rig, double* b_rig, hipStream_t s);
hipError_t launch_rig_project(RigPlan& plan, const double* S_img, int64_t ld_img, const double* b_img, double* S_rig,
                              int64_t ld_rig, double* b_rig, hipStream_t s);

// Rig state of a context (mi_ba_rig_solve): the rig parameters, T and the
// projected system.  Parameter records: the snapshots' rig poses [0,
// num_snapshots), then the rig cameras' relative poses, q(4) t(3) pad.  A
// record that is a variable parameter block with an observation has a slot
// in the rig layout (par_slot >= 0); the images of no rig keep their own pose
// and have a slot each (A = I); constant-pose images have none.
struct RigState {
  mi_ba_rig rig{};                 // caller arrays (write-back)
  RigSetup setup;
  RigPlan plan;
  int num_par = 0, num_snapshots = 0;
  int64_t nf = 0, lds = 0;         // the rig system: 6 slots + intrinsics; lds as DevProblem::lds
  std::vector<int32_t> par_slot_host;
  DevArray<double> par, par_c;     // [num_par][8] current / candidate
  DevArray<int32_t> par_slot;      // [num_par] slot or -1
  DevArray<int2> img_par;          // [I] (snapshot record, relative-pose record), (-1, -1): in no rig
  DevArray<int2> img_slots;        // [I] (owner slot, relative-pose slot), -1: none
  DevArray<uint32_t> flags_free;   // img_flags with the rig images' variable bit cleared
  DevArray<double> S, b, x;        // projected system, rhs, step
  DevArray<double> scale, diag, lambda;  // [6 slots] Jacobi scale, LM diagonal, damping (fblock_finalize's rule)
};

// Called at the end of context creation (the set-up ran build_rig_setup).
mi_ba_status rig_create(mi_ba_context* ctx, const mi_ba_rig& rig, RigSetup&& rs);
void rig_destroy(mi_ba_context* ctx);
// Concatenated poses of the rig images from the parameter records `par`
// into qt (RigBundleAdjustmentCostFunction's operation order).
void rig_compose(mi_ba_context* ctx, const double* par, double* qt);
// After fblock_dense, before the Schur terms: A_i / B_i records at the
// current point, d_rig = diag(T^T U T) from S's diagonal blocks, and the
// slots' Jacobi scale / LM diagonal / damping by launch_fblock_finalize's rule.
void rig_udiag(mi_ba_context* ctx, int first, int reuse_diag, double radius);
// S_rig = T^T S T + damping, b_rig = T^T bvec (after the Schur terms).
mi_ba_status rig_project(mi_ba_context* ctx);
// cg_x = T x_rig.
void rig_expand(mi_ba_context* ctx);
// Candidate rig parameters (quat_plus, tvec add) and the rig images'
// candidate poses into qt_c.
void rig_plus(mi_ba_context* ctx, double* qt_c);
void rig_accept(mi_ba_context* ctx);
// |x|^2, |x - x_c|^2 over the variable rig parameter blocks added into out[0..1].
void rig_state_norms(mi_ba_context* ctx, double* out);
// g_rig = T^T g; |x - Plus(x, -g_rig)|_inf of the rig parameter blocks max-ed into *out.
void rig_grad_max(mi_ba_context* ctx, const double* g, double* out);
// mi_ba_rig_evaluate: the blocks' rig Jacobians [nb][2][15 + ct] from the
// downloaded per-image Jacobians J [nb][2][9 + ct] (host) and the A_i / B_i
// records rig_records_kernel forms at the current rig parameters (device).
mi_ba_status rig_block_jacobians(mi_ba_context* ctx, const double* J, double* out);
// Rig poses, relative poses and the rig images' concatenated poses (TearDown).
mi_ba_status rig_writeback(mi_ba_context* ctx);

}  // namespace miba
