// rig.hip — camera-rig projection of the reduced camera system (gfx950).
//
// S_rig = T^T S_img T as a gather: output block (slot a, slot b), a <= b, is
// the sum of M_ia^T S_ij M_jb over the member pairs (i in members(a), j in
// members(b)), members in image order.  One wave per chunk of at most
// kRigChunkPairs member pairs; two lanes per pair (three output columns
// each), lane pair l takes pairs l, l + 32, ... in that order, the 32 sums of
// a column half are combined by a fixed butterfly, and a block of
// several chunks is combined from its partial sums in chunk order.  With j
// the fast index, neighbouring lanes read neighbouring 48-byte row segments
// of S_img.  Only S_img's upper triangle is read (S_ji = S_ij^T).
#include "rig.h"

#include <algorithm>

#include "ba_math.h"

namespace miba {

namespace {

// S_img(row, col) from the stored (upper, row-major) triangle.
__device__ __forceinline__ double s_upper(const double* __restrict__ S, int64_t ld, int64_t row, int64_t col) {
  const int64_t lo = row < col ? row : col, hi = row < col ? col : row;
  return S[lo * ld + hi];
}

__global__ __launch_bounds__(kRigLanes) void rig_project_kernel(
    const RigItem* __restrict__ items, const int32_t* __restrict__ slot_off, const int2* __restrict__ members,
    const double* __restrict__ rec, const double* __restrict__ S, int64_t ld, double* __restrict__ out, int64_t ldo,
    double* __restrict__ part) {
  // Two lanes per member pair, each with three of the block's six columns: half
  // the accumulators and half of M_jb per lane keep the kernel at several
  // waves per SIMD (the loads of a pair's S rows are shared by its two lanes).
  const RigItem it = items[blockIdx.x];
  const int lane = threadIdx.x, h = lane & 1, c0 = 3 * h;
  const int32_t a0 = slot_off[it.a], b0 = slot_off[it.b];
  const int32_t nb = slot_off[it.b + 1] - b0;
  double acc[18];
#pragma unroll
  for (int k = 0; k < 18; ++k) acc[k] = 0.0;
  for (int32_t p = lane >> 1; p < it.count; p += kRigPairsPerPass) {  // one pass of the member loop per 32 pairs
    const int32_t pair = it.first + p;
    const int2 ea = members[a0 + pair / nb];
    const int2 eb = members[b0 + pair % nb];
    const double* __restrict__ Ma = rec + ea.y;
    const double* __restrict__ Mb = rec + eb.y + c0;
    double mb[18];
#pragma unroll
    for (int k = 0; k < 6; ++k)
#pragma unroll
      for (int c = 0; c < 3; ++c) mb[3 * k + c] = Mb[6 * k + c];
    const int64_t gi = 6 * (int64_t)ea.x, gj = 6 * (int64_t)eb.x;
#pragma unroll
    for (int r = 0; r < 6; ++r) {
      double srow[6], tmp[3];
#pragma unroll
      for (int c = 0; c < 6; ++c) srow[c] = s_upper(S, ld, gi + r, gj + c);
#pragma unroll
      for (int c = 0; c < 3; ++c) {  // tmp = S_ij(r, :) M_jb(:, c0 + c)
        double v = 0.0;
#pragma unroll
        for (int k = 0; k < 6; ++k) v += srow[k] * mb[3 * k + c];
        tmp[c] = v;
      }
#pragma unroll
      for (int q = 0; q < 6; ++q) {  // acc += M_ia(r, :)^T tmp
        const double m = Ma[6 * r + q];
#pragma unroll
        for (int c = 0; c < 3; ++c) acc[3 * q + c] += m * tmp[c];
      }
    }
  }
  // fixed butterfly over the lanes of one column half: lanes 0 and 1 end with the sums
#pragma unroll
  for (int k = 0; k < 18; ++k) {
#pragma unroll
    for (int off = 2; off < kRigLanes; off <<= 1) acc[k] += __shfl_xor(acc[k], off, kRigLanes);
  }
  if (lane > 1) return;
  if (it.part >= 0) {
    double* __restrict__ dst = part + 36 * (int64_t)it.part;
#pragma unroll
    for (int q = 0; q < 6; ++q)
#pragma unroll
      for (int c = 0; c < 3; ++c) dst[6 * q + c0 + c] = acc[3 * q + c];
    return;
  }
#pragma unroll
  for (int q = 0; q < 6; ++q)
#pragma unroll
    for (int c = 0; c < 3; ++c)
      if (it.a != it.b || c0 + c >= q)
        out[(6 * (int64_t)it.a + q) * ldo + 6 * (int64_t)it.b + c0 + c] = acc[3 * q + c];
}

// Blocks of several chunks: partial sums added in chunk order.
__global__ void rig_project_combine_kernel(const RigDest* __restrict__ dests, int ndest,
                                           const double* __restrict__ part, double* __restrict__ out, int64_t ldo) {
  const int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= 36 * (int64_t)ndest) return;
  const RigDest d = dests[t / 36];
  const int k = (int)(t % 36), q = k / 6, c = k % 6;
  double v = 0.0;
  for (int32_t n = 0; n < d.count; ++n) v += part[36 * (int64_t)(d.first + n) + k];
  if (d.a != d.b || c >= q) out[(6 * (int64_t)d.a + q) * ldo + 6 * (int64_t)d.b + c] = v;
}

// Sum over the wave by a fixed butterfly: every lane ends with the same bits.
__device__ __forceinline__ double wave_sum_fixed(double v) {
#pragma unroll
  for (int off = 1; off < kRigLanes; off <<= 1) v += __shfl_xor(v, off, kRigLanes);
  return v;
}

// Pose x intrinsics strips and the right-hand side: one wave per (slot a,
// column c) sums M_ia^T S_img(i, c) over members(a), lane l the members l,
// l + 64, ... in order, then the fixed butterfly; column nc is b.
__global__ __launch_bounds__(kRigLanes) void rig_project_tail_kernel(
    int num_slots, int num_images, int nc, const int32_t* __restrict__ slot_off, const int2* __restrict__ members,
    const double* __restrict__ rec, const double* __restrict__ S, int64_t ld, const double* __restrict__ b_img,
    double* __restrict__ out, int64_t ldo, double* __restrict__ b_rig) {
  const int ncol = nc + 1;
  const int a = blockIdx.x / ncol, c = blockIdx.x % ncol;
  if (a >= num_slots || (c == nc && !b_img)) return;
  double acc[6] = {0, 0, 0, 0, 0, 0};
  for (int32_t m = slot_off[a] + threadIdx.x; m < slot_off[a + 1]; m += kRigLanes) {
    const int2 e = members[m];
    const double* __restrict__ M = rec + e.y;
#pragma unroll
    for (int r = 0; r < 6; ++r) {
      const int64_t row = 6 * (int64_t)e.x + r;
      const double v = c == nc ? b_img[row] : S[row * ld + 6 * (int64_t)num_images + c];
#pragma unroll
      for (int q = 0; q < 6; ++q) acc[q] += M[6 * r + q] * v;
    }
  }
#pragma unroll
  for (int q = 0; q < 6; ++q) acc[q] = wave_sum_fixed(acc[q]);
  if (threadIdx.x != 0) return;
#pragma unroll
  for (int q = 0; q < 6; ++q) {
    if (c == nc) b_rig[6 * (int64_t)a + q] = acc[q];
    else out[(6 * (int64_t)a + q) * ldo + 6 * (int64_t)num_slots + c] = acc[q];
  }
}

// Intrinsics x intrinsics (upper triangle) and the intrinsics' right-hand side: copies.
__global__ void rig_copy_intrinsics_kernel(int num_slots, int num_images, int nc, const double* __restrict__ S,
                                           int64_t ld, const double* __restrict__ b_img, double* __restrict__ out,
                                           int64_t ldo, double* __restrict__ b_rig) {
  const int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= (int64_t)nc * (nc + 1)) return;
  const int r = (int)(t / (nc + 1)), c = (int)(t % (nc + 1));
  const int64_t i0 = 6 * (int64_t)num_images, o0 = 6 * (int64_t)num_slots;
  if (c == nc) {
    if (b_img) b_rig[o0 + r] = b_img[i0 + r];
  } else if (c >= r) {
    out[(o0 + r) * ldo + o0 + c] = S[(i0 + r) * ld + i0 + c];
  }
}

}  // namespace

mi_ba_status rig_plan_build(const mi_ba_rig_table& t, hipStream_t s, RigPlan* plan) {
  const int I = t.num_images, ns = t.num_slots;
  if (I < 0 || ns < 0 || t.num_intrinsics < 0) return MI_BA_ERR_INVALID_ARGUMENT;
  if (I > 0 && (!t.owner_slot || !t.A)) return MI_BA_ERR_INVALID_ARGUMENT;
  if ((int64_t)6 * I + t.num_intrinsics > INT32_MAX / 72 || (int64_t)6 * ns + t.num_intrinsics > INT32_MAX / 72)
    return MI_BA_ERR_UNSUPPORTED;
  std::vector<int32_t> off(ns + 1, 0);
  for (int i = 0; i < I; ++i) {
    const int32_t o = t.owner_slot[i], r = t.rel_slot ? t.rel_slot[i] : -1;
    if (o < -1 || o >= ns || r < -1 || r >= ns || (o >= 0 && r == o) || (o < 0 && r >= 0))
      return MI_BA_ERR_INVALID_ARGUMENT;
    if (r >= 0 && !t.B) return MI_BA_ERR_INVALID_ARGUMENT;
    if (o < 0) continue;  // no variable pose: the image's rows drop out
    off[o + 1]++;
    if (r >= 0) off[r + 1]++;
  }
  for (int a = 0; a < ns; ++a) off[a + 1] += off[a];
  std::vector<int2> mem(off[ns]);
  std::vector<double> rec(72 * (size_t)I, 0.0);
  {
    std::vector<int32_t> pos(off.begin(), off.end() - 1);
    for (int i = 0; i < I; ++i) {  // image order within every slot
      if (t.owner_slot[i] < 0) continue;
      mem[pos[t.owner_slot[i]]++] = make_int2(i, 72 * i);
      std::copy(t.A + 36 * (size_t)i, t.A + 36 * (size_t)i + 36, rec.begin() + 72 * (size_t)i);
      const int32_t r = t.rel_slot ? t.rel_slot[i] : -1;
      if (r >= 0) {
        mem[pos[r]++] = make_int2(i, 72 * i + 36);
        std::copy(t.B + 36 * (size_t)i, t.B + 36 * (size_t)i + 36, rec.begin() + 72 * (size_t)i + 36);
      }
    }
  }
  std::vector<RigItem> items;
  std::vector<RigDest> dests;
  int64_t nparts = 0;
  items.reserve((size_t)ns * (ns + 1) / 2);
  for (int a = 0; a < ns; ++a)
    for (int b = a; b < ns; ++b) {
      const int64_t npairs = (int64_t)(off[a + 1] - off[a]) * (off[b + 1] - off[b]);
      if (npairs > INT32_MAX) return MI_BA_ERR_UNSUPPORTED;
      const int64_t nchunk = std::max<int64_t>(1, (npairs + kRigChunkPairs - 1) / kRigChunkPairs);
      if (nchunk > 1) dests.push_back(RigDest{a, b, (int32_t)nparts, (int32_t)nchunk});
      for (int64_t k = 0; k < nchunk; ++k) {
        const int64_t first = k * kRigChunkPairs;
        const int32_t count = (int32_t)std::min<int64_t>(kRigChunkPairs, npairs - first);
        items.push_back(RigItem{a, b, (int32_t)first, count, nchunk > 1 ? (int32_t)(nparts + k) : -1, 0});
      }
      if (nchunk > 1) nparts += nchunk;
      if (nparts > INT32_MAX / 36 || items.size() > (size_t)INT32_MAX) return MI_BA_ERR_UNSUPPORTED;
    }
  plan->num_images = I;
  plan->num_intrinsics = t.num_intrinsics;
  plan->num_slots = ns;
  if (plan->slot_off.alloc(off.size()) || plan->members.alloc(mem.size()) || plan->items.alloc(items.size()) ||
      plan->dests.alloc(dests.size()) || plan->part.alloc(36 * (size_t)nparts) || plan->rec.alloc(rec.size()))
    return MI_BA_ERR_OUT_OF_MEMORY;
  auto up = [&](void* dst, const void* src, size_t bytes) {
    return bytes == 0 || hipMemcpyAsync(dst, src, bytes, hipMemcpyHostToDevice, s) == hipSuccess;
  };
  if (!up(plan->slot_off.ptr, off.data(), plan->slot_off.bytes()) ||
      !up(plan->members.ptr, mem.data(), plan->members.bytes()) ||
      !up(plan->items.ptr, items.data(), plan->items.bytes()) ||
      !up(plan->dests.ptr, dests.data(), plan->dests.bytes()) || !up(plan->rec.ptr, rec.data(), plan->rec.bytes()) ||
      hipStreamSynchronize(s) != hipSuccess)  // the host vectors go out of scope
    return MI_BA_ERR_HIP;
  return MI_BA_OK;
}

hipError_t launch_rig_project_blocks(RigPlan& plan, const double* S_img, int64_t ld_img, double* S_rig,
                                     int64_t ld_rig, hipStream_t s) {
  if (plan.items.n > 0)
    hipLaunchKernelGGL(rig_project_kernel, dim3((unsigned)plan.items.n), dim3(kRigLanes), 0, s, plan.items.ptr,
                       plan.slot_off.ptr, plan.members.ptr, plan.rec.ptr, S_img, ld_img, S_rig, ld_rig,
                       plan.part.ptr);
  if (plan.dests.n > 0) {
    const int64_t n = 36 * (int64_t)plan.dests.n;
    hipLaunchKernelGGL(rig_project_combine_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, plan.dests.ptr,
                       (int)plan.dests.n, plan.part.ptr, S_rig, ld_rig);
  }
  return hipGetLastError();
}

hipError_t launch_rig_project_tail(RigPlan& plan, const double* S_img, int64_t ld_img, const double* b_img,
                                   double* S_rig, int64_t ld_rig, double* b_rig, hipStream_t s) {
  const int ns = plan.num_slots, I = plan.num_images, nc = plan.num_intrinsics;
  if (ns > 0)
    hipLaunchKernelGGL(rig_project_tail_kernel, dim3((unsigned)((int64_t)ns * (nc + 1))), dim3(kRigLanes), 0, s, ns, I,
                       nc, plan.slot_off.ptr, plan.members.ptr, plan.rec.ptr, S_img, ld_img, b_img, S_rig, ld_rig,
                       b_rig);
  if (nc > 0) {
    const int64_t n = (int64_t)nc * (nc + 1);
    hipLaunchKernelGGL(rig_copy_intrinsics_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, ns, I, nc,
                       S_img, ld_img, b_img, S_rig, ld_rig, b_rig);
  }
  return hipGetLastError();
}

hipError_t launch_rig_project(RigPlan& plan, const double* S_img, int64_t ld_img, const double* b_img, double* S_rig,
                              int64_t ld_rig, double* b_rig, hipStream_t s) {
  const hipError_t e = launch_rig_project_blocks(plan, S_img, ld_img, S_rig, ld_rig, s);
  return e != hipSuccess ? e : launch_rig_project_tail(plan, S_img, ld_img, b_img, S_rig, ld_rig, b_rig, s);
}

// ---------------------------------------------------------------------------
// LM hooks (context_solve's rig branch)
// ---------------------------------------------------------------------------
namespace {

// Concatenated pose of every rig image in the reference functor's order
// (cost_functions.h:178-187): q = QuaternionProduct(rel, rig), t =
// UnitQuaternionRotatePoint(rel, t_rig) + t_rel.
__global__ void rig_compose_kernel(int num_images, const int2* __restrict__ img_par, const double* __restrict__ par,
                                   double* __restrict__ qt) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= num_images) return;
  const int2 ip = img_par[i];
  if (ip.x < 0) return;
  const double* g = par + 8 * (size_t)ip.x;
  const double* l = par + 8 * (size_t)ip.y;
  const double w[4] = {g[0], g[1], g[2], g[3]}, z[4] = {l[0], l[1], l[2], l[3]};
  const double tg[3] = {g[4], g[5], g[6]};
  double* o = qt + 8 * (size_t)i;
  o[0] = z[0] * w[0] - z[1] * w[1] - z[2] * w[2] - z[3] * w[3];
  o[1] = z[0] * w[1] + z[1] * w[0] + z[2] * w[3] - z[3] * w[2];
  o[2] = z[0] * w[2] - z[1] * w[3] + z[2] * w[0] + z[3] * w[1];
  o[3] = z[0] * w[3] + z[1] * w[2] - z[2] * w[1] + z[3] * w[0];
  double t[3];
  unit_quat_rotate(z, tg, t);
  o[4] = t[0] + l[4];
  o[5] = t[1] + l[5];
  o[6] = t[2] + l[6];
}

// A_i = diag(R_rel, R_rel), B_i = [[I, 0], [-2 [R_rel t_rig]x, I]] of every
// rig image at the current rig parameters (the images of no rig keep A = I).
__global__ void rig_records_kernel(int num_images, const int2* __restrict__ img_par, const double* __restrict__ par,
                                   double* __restrict__ rec) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= num_images) return;
  const int2 ip = img_par[i];
  if (ip.x < 0) return;
  const double* g = par + 8 * (size_t)ip.x;
  const double* l = par + 8 * (size_t)ip.y;
  const double z[4] = {l[0], l[1], l[2], l[3]};
  const double tg[3] = {g[4], g[5], g[6]};
  double R[9], v[3];
  unit_quat_matrix(z, R);
  unit_quat_rotate(z, tg, v);
  double* A = rec + 72 * (size_t)i;
  double* B = A + 36;
  for (int k = 0; k < 36; ++k) {
    A[k] = 0.0;
    B[k] = 0.0;
  }
  for (int r = 0; r < 3; ++r)
    for (int c = 0; c < 3; ++c) {
      A[6 * r + c] = R[3 * r + c];
      A[6 * (r + 3) + c + 3] = R[3 * r + c];
    }
  for (int k = 0; k < 6; ++k) B[6 * k + k] = 1.0;
  B[6 * 3 + 1] = 2.0 * v[2];  B[6 * 3 + 2] = -2.0 * v[1];
  B[6 * 4 + 0] = -2.0 * v[2]; B[6 * 4 + 2] = 2.0 * v[0];
  B[6 * 5 + 0] = 2.0 * v[1];  B[6 * 5 + 1] = -2.0 * v[0];
}

// d_rig(slot a, q) = sum over members(a) of (M_i^T U_ii M_i)(q, q), in a fixed
// order (lane sums, then the butterfly), then launch_fblock_finalize's rule (Ceres scales and damps in the
// parameters it optimises).
__global__ __launch_bounds__(kRigLanes) void rig_udiag_kernel(
    int num_slots, const int32_t* __restrict__ slot_off, const int2* __restrict__ members,
    const double* __restrict__ rec, const double* __restrict__ S, int64_t ld, double* __restrict__ scale,
    double* __restrict__ diag, double* __restrict__ lambda, int first, int reuse_diag, double radius) {
  const int t = blockIdx.x;  // one wave per (slot, q); lane l the members l, l + 64, ...
  if (t >= 6 * num_slots) return;
  const int a = t / 6, q = t % 6;
  double d = 0.0;
  for (int32_t m = slot_off[a] + threadIdx.x; m < slot_off[a + 1]; m += kRigLanes) {
    const int2 e = members[m];
    const double* __restrict__ M = rec + e.y;
    const int64_t g0 = 6 * (int64_t)e.x;
    double mq[6];
#pragma unroll
    for (int r = 0; r < 6; ++r) mq[r] = M[6 * r + q];
    double v = 0.0;
#pragma unroll
    for (int r = 0; r < 6; ++r) {
      double w = 0.0;
#pragma unroll
      for (int k = 0; k < 6; ++k) w += s_upper(S, ld, g0 + r, g0 + k) * mq[k];
      v += mq[r] * w;
    }
    d += v;
  }
  d = wave_sum_fixed(d);
  if (threadIdx.x != 0) return;
  double s;
  if (first) {
    s = 1.0 / (1.0 + sqrt(d));
    scale[t] = s;
  } else {
    s = scale[t];
  }
  double dg;
  if (!reuse_diag) {
    dg = fmin(fmax(s * s * d, 1e-6), 1e32);
    diag[t] = dg;
  } else {
    dg = diag[t];
  }
  lambda[t] = dg / (radius * s * s);
}

// Damping on S_rig's diagonal; the intrinsics keep launch_fblock_finalize's
// damping, identity on the slots of constant cameras.
__global__ void rig_damp_kernel(int num_slots, int num_images, int nc, int ct, const uint8_t* __restrict__ cam_var,
                                const double* __restrict__ lambda_rig, const double* __restrict__ lambda_f,
                                double* __restrict__ S, int64_t ld) {
  const int64_t k = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  const int64_t n0 = 6 * (int64_t)num_slots;
  if (k >= n0 + nc) return;
  if (k < n0) {
    S[k * ld + k] += lambda_rig[k];
  } else {
    const int64_t j = k - n0;
    if (cam_var[j / (ct > 0 ? ct : 1)]) S[k * ld + k] += lambda_f[6 * (int64_t)num_images + j];
    else S[k * ld + k] = 1.0;
  }
}

// d_img = T d_rig.
__global__ void rig_expand_kernel(int num_slots, int num_images, int nc, const int2* __restrict__ img_slots,
                                  const double* __restrict__ rec, const double* __restrict__ x,
                                  double* __restrict__ df) {
  const int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (t < num_images) {
    const int2 sl = img_slots[t];
    double o[6] = {0, 0, 0, 0, 0, 0};
    if (sl.x >= 0) {
      const double* __restrict__ A = rec + 72 * (size_t)t;
      const double* xa = x + 6 * (size_t)sl.x;
#pragma unroll
      for (int r = 0; r < 6; ++r)
#pragma unroll
        for (int k = 0; k < 6; ++k) o[r] += A[6 * r + k] * xa[k];
    }
    if (sl.y >= 0) {
      const double* __restrict__ B = rec + 72 * (size_t)t + 36;
      const double* xb = x + 6 * (size_t)sl.y;
#pragma unroll
      for (int r = 0; r < 6; ++r)
#pragma unroll
        for (int k = 0; k < 6; ++k) o[r] += B[6 * r + k] * xb[k];
    }
#pragma unroll
    for (int r = 0; r < 6; ++r) df[6 * (size_t)t + r] = o[r];
  } else if (t < (int64_t)num_images + nc) {
    const int64_t j = t - num_images;
    df[6 * (int64_t)num_images + j] = x[6 * (int64_t)num_slots + j];
  }
}

// Candidate rig parameters: QuaternionManifold Plus on qvec, tvec add.
__global__ void rig_plus_kernel(int num_par, const int32_t* __restrict__ par_slot, const double* __restrict__ par,
                                const double* __restrict__ x, double* __restrict__ par_c) {
  const int p = blockIdx.x * blockDim.x + threadIdx.x;
  if (p >= num_par) return;
  const double* a = par + 8 * (size_t)p;
  double* o = par_c + 8 * (size_t)p;
  const int32_t sl = par_slot[p];
  if (sl < 0) {
    for (int m = 0; m < 8; ++m) o[m] = a[m];
    return;
  }
  const double* d = x + 6 * (size_t)sl;
  const double q[4] = {a[0], a[1], a[2], a[3]}, dq[3] = {d[0], d[1], d[2]};
  double qn[4];
  quat_plus(q, dq, qn);
  for (int m = 0; m < 4; ++m) o[m] = qn[m];
  for (int m = 0; m < 3; ++m) o[4 + m] = a[4 + m] + d[3 + m];
  o[7] = 0.0;
}

// One thread, record order: a fixed sum.
__global__ void rig_state_norms_kernel(int num_par, const int32_t* __restrict__ par_slot,
                                       const double* __restrict__ par, const double* __restrict__ par_c,
                                       double* __restrict__ out) {
  if (blockIdx.x != 0 || threadIdx.x != 0) return;
  double vx = 0.0, vd = 0.0;
  for (int p = 0; p < num_par; ++p) {
    if (par_slot[p] < 0) continue;
    for (int m = 0; m < 7; ++m) {
      const double a = par[8 * (size_t)p + m], d = a - par_c[8 * (size_t)p + m];
      vx += a * a;
      vd += d * d;
    }
  }
  out[0] += vx;
  out[1] += vd;
}

__global__ void rig_grad_max_kernel(int num_par, const int32_t* __restrict__ par_slot, const double* __restrict__ par,
                                    const int32_t* __restrict__ slot_off, const int2* __restrict__ members,
                                    const double* __restrict__ rec, const double* __restrict__ g,
                                    unsigned long long* out) {
  const int p = blockIdx.x * blockDim.x + threadIdx.x;
  if (p >= num_par) return;
  const int32_t sl = par_slot[p];
  if (sl < 0) return;
  double gr[6] = {0, 0, 0, 0, 0, 0};
  for (int32_t m = slot_off[sl]; m < slot_off[sl + 1]; ++m) {
    const int2 e = members[m];
    const double* __restrict__ M = rec + e.y;
    const double* gi = g + 6 * (size_t)e.x;
    for (int r = 0; r < 6; ++r)
      for (int q = 0; q < 6; ++q) gr[q] += M[6 * r + q] * gi[r];
  }
  const double* a = par + 8 * (size_t)p;
  const double q[4] = {a[0], a[1], a[2], a[3]}, d[3] = {-gr[0], -gr[1], -gr[2]};
  double qn[4];
  quat_plus(q, d, qn);
  double mx = 0.0;
  for (int m = 0; m < 4; ++m) mx = fmax(mx, fabs(q[m] - qn[m]));
  for (int m = 0; m < 3; ++m) mx = fmax(mx, fabs(a[4 + m] - (a[4 + m] + -gr[3 + m])));
  // non-negative doubles order as their bit patterns
  if (mx > 0.0) atomicMax(out, (unsigned long long)__double_as_longlong(mx));
}

inline unsigned grid_of(int64_t n, int block) { return (unsigned)std::max<int64_t>(1, (n + block - 1) / block); }

}  // namespace

mi_ba_status rig_create(mi_ba_context* ctx, const mi_ba_rig& rig, RigSetup&& rs) {
  const mi_ba_problem* p = &ctx->problem;
  const HostSetup& s = ctx->setup;
  const DevProblem& d = ctx->dev;
  const int I = p->num_images, C = p->num_cameras;
  RigState* R = new RigState();
  ctx->rig = R;
  R->rig = rig;
  R->setup = std::move(rs);
  const RigSetup& u = R->setup;
  const int nsnap = rig.num_snapshots, ncam = rig.num_rigs > 0 ? rig.rig_camera_off[rig.num_rigs] : 0;
  R->num_snapshots = nsnap;
  R->num_par = nsnap + ncam;
  // slots: used snapshots, variable images of no rig, variable relative poses
  std::vector<int32_t>& ps = R->par_slot_host;
  ps.assign(R->num_par, -1);
  int ns = 0;
  for (int k = 0; k < nsnap; ++k)
    if (u.snapshot_used[k]) ps[k] = ns++;
  std::vector<int32_t> owner(I, -1), rel(I, -1);
  std::vector<int2> ipar(I, make_int2(-1, -1)), isl(I, make_int2(-1, -1));
  std::vector<uint32_t> fl(I);
  for (int i = 0; i < I; ++i)
    if (s.img_var[i] && u.img_snapshot[i] < 0) owner[i] = ns++;
  for (int k = 0; k < ncam; ++k)
    if (u.rel_var[k]) ps[nsnap + k] = ns++;
  for (int i = 0; i < I; ++i) {
    fl[i] = (s.img_var[i] ? 1u : 0u) | ((uint32_t)s.img_tvec_mask[i] << 1);
    if (!s.img_var[i] || u.img_snapshot[i] < 0) continue;
    fl[i] &= ~1u;
    ipar[i] = make_int2(u.img_snapshot[i], nsnap + u.img_rel[i]);
    owner[i] = ps[u.img_snapshot[i]];
    rel[i] = ps[nsnap + u.img_rel[i]];
  }
  for (int i = 0; i < I; ++i) isl[i] = make_int2(owner[i], rel[i]);
  const int nc = d.ct * C;
  std::vector<double> eye(36 * (size_t)std::max(1, I), 0.0);
  for (int i = 0; i < I; ++i)
    for (int k = 0; k < 6; ++k) eye[36 * (size_t)i + 7 * k] = 1.0;
  mi_ba_rig_table t{};
  t.num_images = I;
  t.num_intrinsics = nc;
  t.num_slots = ns;
  t.owner_slot = owner.data();
  t.rel_slot = rel.data();
  t.A = eye.data();
  t.B = eye.data();  // refreshed per linearization (rig_records_kernel)
  mi_ba_status st = rig_plan_build(t, ctx->stream, &R->plan);
  if (st != MI_BA_OK) return st;
  R->nf = 6 * (int64_t)ns + nc;
  R->lds = (R->nf + 1 + 15) / 16 * 16;
  std::vector<double> par(8 * (size_t)R->num_par, 0.0);
  for (int k = 0; k < nsnap; ++k) {
    for (int m = 0; m < 4; ++m) par[8 * (size_t)k + m] = rig.snapshot_qvec[4 * (size_t)k + m];
    for (int m = 0; m < 3; ++m) par[8 * (size_t)k + 4 + m] = rig.snapshot_tvec[3 * (size_t)k + m];
  }
  for (int k = 0; k < ncam; ++k) {
    for (int m = 0; m < 4; ++m) par[8 * (size_t)(nsnap + k) + m] = rig.rel_qvec[4 * (size_t)k + m];
    for (int m = 0; m < 3; ++m) par[8 * (size_t)(nsnap + k) + 4 + m] = rig.rel_tvec[3 * (size_t)k + m];
  }
  if (R->par.alloc(par.size()) || R->par_c.alloc(par.size()) || R->par_slot.alloc(ps.size()) ||
      R->img_par.alloc(I) || R->img_slots.alloc(I) || R->flags_free.alloc(I) ||
      R->S.alloc((size_t)R->nf * R->lds) || R->b.alloc(R->nf) || R->x.alloc(R->nf) ||
      R->scale.alloc(6 * (size_t)ns) || R->diag.alloc(6 * (size_t)ns) || R->lambda.alloc(6 * (size_t)ns))
    return MI_BA_ERR_OUT_OF_MEMORY;
  auto up = [&](void* dst, const void* src, size_t bytes) {
    return bytes == 0 || hipMemcpy(dst, src, bytes, hipMemcpyHostToDevice) == hipSuccess;
  };
  if (!up(R->par.ptr, par.data(), R->par.bytes()) || !up(R->par_c.ptr, par.data(), R->par_c.bytes()) ||
      !up(R->par_slot.ptr, ps.data(), R->par_slot.bytes()) || !up(R->img_par.ptr, ipar.data(), R->img_par.bytes()) ||
      !up(R->img_slots.ptr, isl.data(), R->img_slots.bytes()) || !up(R->flags_free.ptr, fl.data(), R->flags_free.bytes()))
    return MI_BA_ERR_HIP;
  // the rig images' poses the first linearization reads
  rig_compose(ctx, R->par.ptr, ctx->qt.ptr);
  return hipGetLastError() == hipSuccess ? MI_BA_OK : MI_BA_ERR_HIP;
}

void rig_destroy(mi_ba_context* ctx) {
  delete ctx->rig;
  ctx->rig = nullptr;
}

void rig_compose(mi_ba_context* ctx, const double* par, double* qt) {
  RigState* R = ctx->rig;
  const int I = ctx->dev.num_images;
  if (I > 0)
    hipLaunchKernelGGL(rig_compose_kernel, dim3(grid_of(I, 64)), dim3(64), 0, ctx->stream, I, R->img_par.ptr, par, qt);
}

void rig_udiag(mi_ba_context* ctx, int first, int reuse_diag, double radius) {
  RigState* R = ctx->rig;
  const int I = ctx->dev.num_images, ns = R->plan.num_slots;
  hipStream_t s = ctx->stream;
  hipEvent_t stop;
  timer_begin(ctx, "rig_udiag", &stop);
  if (I > 0)
    hipLaunchKernelGGL(rig_records_kernel, dim3(grid_of(I, 64)), dim3(64), 0, s, I, R->img_par.ptr, R->par.ptr,
                       R->plan.rec.ptr);
  if (ns > 0)
    hipLaunchKernelGGL(rig_udiag_kernel, dim3((unsigned)(6 * ns)), dim3(kRigLanes), 0, s, ns, R->plan.slot_off.ptr,
                       R->plan.members.ptr, R->plan.rec.ptr, ctx->S.ptr, ctx->dev.lds, R->scale.ptr, R->diag.ptr,
                       R->lambda.ptr, first, reuse_diag, radius);
  timer_end(ctx, stop);
}

mi_ba_status rig_project(mi_ba_context* ctx) {
  RigState* R = ctx->rig;
  const DevProblem& d = ctx->dev;
  hipStream_t s = ctx->stream;
  if (hipMemsetAsync(R->S.ptr, 0, R->S.bytes(), s) != hipSuccess) return MI_BA_ERR_HIP;
  hipEvent_t stop;
  timer_begin(ctx, "rig_project_blocks", &stop);
  const hipError_t e1 = launch_rig_project_blocks(R->plan, ctx->S.ptr, d.lds, R->S.ptr, R->lds, s);
  timer_end(ctx, stop);
  timer_begin(ctx, "rig_project_tail", &stop);
  const hipError_t e2 = launch_rig_project_tail(R->plan, ctx->S.ptr, d.lds, ctx->bvec.ptr, R->S.ptr, R->lds, R->b.ptr, s);
  timer_end(ctx, stop);
  if (e1 != hipSuccess || e2 != hipSuccess) return MI_BA_ERR_HIP;
  hipLaunchKernelGGL(rig_damp_kernel, dim3(grid_of(R->nf, 256)), dim3(256), 0, s, R->plan.num_slots, d.num_images,
                     R->plan.num_intrinsics, d.ct, d.cam_var, R->lambda.ptr, ctx->lambda_f.ptr, R->S.ptr, R->lds);
  return MI_BA_OK;
}

void rig_expand(mi_ba_context* ctx) {
  RigState* R = ctx->rig;
  const int I = ctx->dev.num_images, nc = R->plan.num_intrinsics;
  hipLaunchKernelGGL(rig_expand_kernel, dim3(grid_of((int64_t)I + nc, 256)), dim3(256), 0, ctx->stream,
                     R->plan.num_slots, I, nc, R->img_slots.ptr, R->plan.rec.ptr, R->x.ptr, ctx->cg_x.ptr);
}

void rig_plus(mi_ba_context* ctx, double* qt_c) {
  RigState* R = ctx->rig;
  if (R->num_par > 0)
    hipLaunchKernelGGL(rig_plus_kernel, dim3(grid_of(R->num_par, 64)), dim3(64), 0, ctx->stream, R->num_par,
                       R->par_slot.ptr, R->par.ptr, R->x.ptr, R->par_c.ptr);
  rig_compose(ctx, R->par_c.ptr, qt_c);
}

void rig_accept(mi_ba_context* ctx) { std::swap(ctx->rig->par.ptr, ctx->rig->par_c.ptr); }

void rig_state_norms(mi_ba_context* ctx, double* out) {
  RigState* R = ctx->rig;
  hipLaunchKernelGGL(rig_state_norms_kernel, dim3(1), dim3(64), 0, ctx->stream, R->num_par, R->par_slot.ptr,
                     R->par.ptr, R->par_c.ptr, out);
}

void rig_grad_max(mi_ba_context* ctx, const double* g, double* out) {
  RigState* R = ctx->rig;
  const int I = ctx->dev.num_images;
  hipStream_t s = ctx->stream;
  if (I > 0)
    hipLaunchKernelGGL(rig_records_kernel, dim3(grid_of(I, 64)), dim3(64), 0, s, I, R->img_par.ptr, R->par.ptr,
                       R->plan.rec.ptr);
  if (R->num_par > 0)
    hipLaunchKernelGGL(rig_grad_max_kernel, dim3(grid_of(R->num_par, 64)), dim3(64), 0, s, R->num_par,
                       R->par_slot.ptr, R->par.ptr, R->plan.slot_off.ptr, R->plan.members.ptr, R->plan.rec.ptr, g,
                       reinterpret_cast<unsigned long long*>(out));
}

mi_ba_status rig_block_jacobians(mi_ba_context* ctx, const double* J, double* out) {
  RigState* R = ctx->rig;
  const mi_ba_problem* p = &ctx->problem;
  const HostSetup& s = ctx->setup;
  const int I = p->num_images, W = ctx->dev.W, ct = ctx->dev.ct, Wo = 15 + ct;
  const int64_t nb = ctx->dev.nb;
  if (I > 0)
    hipLaunchKernelGGL(rig_records_kernel, dim3(grid_of(I, 64)), dim3(64), 0, ctx->stream, I, R->img_par.ptr,
                       R->par.ptr, R->plan.rec.ptr);
  std::vector<double> rec(72 * (size_t)I);
  if (hipStreamSynchronize(ctx->stream) != hipSuccess ||
      (I > 0 && hipMemcpy(rec.data(), R->plan.rec.ptr, rec.size() * 8, hipMemcpyDeviceToHost) != hipSuccess))
    return MI_BA_ERR_HIP;
  for (int64_t b = 0; b < nb; ++b) {
    const int img = p->obs_image[ctx->block_obs[b]];
    const bool rig_img = s.img_var[img] && R->setup.img_snapshot[img] >= 0;
    const bool rel_var = rig_img && R->par_slot_host[R->num_snapshots + R->setup.img_rel[img]] >= 0;
    const double* A = rec.data() + 72 * (size_t)img;
    for (int row = 0; row < 2; ++row) {
      const double* j = J + ((size_t)b * 2 + row) * W;
      double* o = out + ((size_t)b * 2 + row) * Wo;
      for (int c = 0; c < 6; ++c) {
        double va = 0.0, vb = 0.0;
        for (int r = 0; r < 6; ++r) {
          va += j[r] * A[6 * r + c];
          vb += j[r] * A[36 + 6 * r + c];
        }
        o[c] = rig_img ? va : j[c];
        o[6 + c] = rel_var ? vb : 0.0;
      }
      for (int c = 0; c < 3 + ct; ++c) o[12 + c] = j[6 + c];
    }
  }
  return MI_BA_OK;
}

mi_ba_status rig_writeback(mi_ba_context* ctx) {
  RigState* R = ctx->rig;
  mi_ba_problem* p = &ctx->problem;
  const mi_ba_rig& rig = R->rig;
  std::vector<double> par(8 * (size_t)R->num_par);
  if (!par.empty() && hipMemcpy(par.data(), R->par.ptr, par.size() * 8, hipMemcpyDeviceToHost) != hipSuccess)
    return MI_BA_ERR_HIP;
  const int nsnap = R->num_snapshots;
  for (int k = 0; k < R->num_par; ++k) {
    if (R->par_slot_host[k] < 0) continue;  // constant or unused: left as given
    double* q = k < nsnap ? rig.snapshot_qvec + 4 * (size_t)k : rig.rel_qvec + 4 * (size_t)(k - nsnap);
    double* t = k < nsnap ? rig.snapshot_tvec + 3 * (size_t)k : rig.rel_tvec + 3 * (size_t)(k - nsnap);
    for (int m = 0; m < 4; ++m) q[m] = par[8 * (size_t)k + m];
    for (int m = 0; m < 3; ++m) t[m] = par[8 * (size_t)k + 4 + m];
  }
  // TearDown (bundle_adjustment.cc:891-903): every snapshot image
  for (int i = 0; i < p->num_images; ++i) {
    const int sn = R->setup.img_snapshot[i];
    if (sn < 0) continue;
    const int k = R->setup.img_rel[i];
    rig_concatenate_poses(rig.snapshot_qvec + 4 * (size_t)sn, rig.snapshot_tvec + 3 * (size_t)sn,
                          rig.rel_qvec + 4 * (size_t)k, rig.rel_tvec + 3 * (size_t)k, p->qvec + 4 * (size_t)i,
                          p->tvec + 3 * (size_t)i);
  }
  return MI_BA_OK;
}

}  // namespace miba

using namespace miba;

extern "C" {

void mi_ba_default_rig(mi_ba_rig* rig) {
  if (!rig) return;
  *rig = mi_ba_rig{};
  rig->refine_relative_poses = 1;  // RigBundleAdjuster::Options (bundle_adjustment.h:272-280)
  rig->max_reproj_error = 1000.0;
}

mi_ba_status mi_ba_rig_setup_stats(const mi_ba_options* o, const mi_ba_problem* p, const mi_ba_rig* rig,
                                   mi_ba_setup_info* info) {
  if (!o || !p || !rig || !info) return MI_BA_ERR_INVALID_ARGUMENT;
  // SetUp normalises qvecs in place; work on a private copy of the qvecs.
  mi_ba_problem copy = *p;
  std::vector<double> q;
  if (p->qvec && p->num_images > 0) q.assign(p->qvec, p->qvec + 4 * (size_t)p->num_images);
  copy.qvec = p->qvec ? q.data() : nullptr;
  HostSetup s;
  RigSetup rs;
  const mi_ba_status st = build_rig_setup(*o, &copy, *rig, &s, &rs);
  if (st != MI_BA_OK) return st;
  info->num_residual_blocks = s.num_residual_blocks;
  info->num_residuals_reduced = s.num_residuals_reduced;
  info->num_effective_parameters_reduced = s.num_effective_parameters_reduced;
  info->num_variable_images = 0;
  for (size_t i = 0; i < s.img_var.size(); ++i) info->num_variable_images += s.img_var[i] && rs.img_snapshot[i] < 0;
  info->num_variable_cameras = 0;
  for (uint8_t v : s.cam_var) info->num_variable_cameras += v;
  info->num_variable_points = 0;
  for (uint8_t v : s.pt_var) info->num_variable_points += v;
  info->camera_tangent_size = s.ct;
  return MI_BA_OK;
}

int32_t mi_ba_rig_project_chunk(int32_t* lanes) {
  if (lanes) *lanes = kRigPairsPerPass;
  return kRigChunkPairs;
}

mi_ba_status mi_ba_rig_reduce_dense(int32_t device, int32_t n_img, const double* S_img, const double* b_img,
                                    const mi_ba_rig_table* table, int32_t n_rig, double* S_rig, double* b_rig) {
  if (!table || !S_img || !S_rig || (b_img == nullptr) != (b_rig == nullptr)) return MI_BA_ERR_INVALID_ARGUMENT;
  if (table->num_images < 0 || table->num_slots < 0 || table->num_intrinsics < 0 ||
      (int64_t)n_img != 6 * (int64_t)table->num_images + table->num_intrinsics ||
      (int64_t)n_rig != 6 * (int64_t)table->num_slots + table->num_intrinsics)
    return MI_BA_ERR_INVALID_ARGUMENT;
  int ndev = 0;
  if (hipGetDeviceCount(&ndev) != hipSuccess || ndev == 0) return MI_BA_ERR_NO_DEVICE;
  if (device < 0 || device >= ndev) return MI_BA_ERR_INVALID_ARGUMENT;
  if (hipSetDevice(device) != hipSuccess) return MI_BA_ERR_HIP;
  if (n_rig == 0) return MI_BA_OK;
  hipStream_t s = nullptr;
  RigPlan plan;
  DevArray<double> dS, dR, db, dbr;
  mi_ba_status st = MI_BA_OK;
  do {
    if (hipStreamCreateWithFlags(&s, hipStreamNonBlocking) != hipSuccess) { s = nullptr; st = MI_BA_ERR_HIP; break; }
    st = rig_plan_build(*table, s, &plan);
    if (st != MI_BA_OK) break;
    if (dS.alloc((size_t)n_img * n_img) || dR.alloc((size_t)n_rig * n_rig) || db.alloc(b_img ? n_img : 0) ||
        dbr.alloc(b_img ? n_rig : 0)) {
      st = MI_BA_ERR_OUT_OF_MEMORY;
      break;
    }
    if ((dS.n && hipMemcpyAsync(dS.ptr, S_img, dS.bytes(), hipMemcpyHostToDevice, s) != hipSuccess) ||
        (db.n && hipMemcpyAsync(db.ptr, b_img, db.bytes(), hipMemcpyHostToDevice, s) != hipSuccess) ||
        hipMemsetAsync(dR.ptr, 0, dR.bytes(), s) != hipSuccess ||
        (dbr.n && hipMemsetAsync(dbr.ptr, 0, dbr.bytes(), s) != hipSuccess) ||
        launch_rig_project(plan, dS.ptr, n_img, db.ptr, dR.ptr, n_rig, dbr.ptr, s) != hipSuccess ||
        hipMemcpyAsync(S_rig, dR.ptr, dR.bytes(), hipMemcpyDeviceToHost, s) != hipSuccess ||
        (dbr.n && hipMemcpyAsync(b_rig, dbr.ptr, dbr.bytes(), hipMemcpyDeviceToHost, s) != hipSuccess) ||
        hipStreamSynchronize(s) != hipSuccess)
      st = MI_BA_ERR_HIP;
  } while (false);
  if (s) {
    (void)hipStreamSynchronize(s);
    (void)hipStreamDestroy(s);
  }
  return st;
}

}  // extern "C"
