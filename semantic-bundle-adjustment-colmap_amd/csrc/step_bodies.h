// step_bodies.h — device bodies of the linearization step's small kernels
// (product code), shared by the stand-alone kernels (kernels.hip,
// semantic.hip) and by the fused launches of "linearize_fusion": the step
// prologue (semantic.hip: pair tables + image records + input warm-up) and the
// step epilogue (kernels.hip: both cost sums + pair blocks).  Both forms call
// the same code, so their results are the same bits.
#pragma once

#include <hip/hip_runtime.h>

#include <cstdint>

#include "device.h"

namespace miba {

// unit_quat_matrix (ba_math.h) with FMA contraction whatever the translation
// unit's setting: the image records are built in kernels.hip (contracting) and
// in the step prologue (semantic.hip, built with -ffp-contract=off), and the
// reprojection kernel's results follow the records' last bits.
__device__ inline void unit_quat_matrix_contracted(const double q[4], double R[9]) {
#pragma clang fp contract(fast)
  const double t2 = q[0] * q[1], t3 = q[0] * q[2], t4 = q[0] * q[3];
  const double t5 = -(q[1] * q[1]), t6 = q[1] * q[2], t7 = q[1] * q[3];
  const double t8 = -(q[2] * q[2]), t9 = q[2] * q[3], t1 = -(q[3] * q[3]);
  R[0] = 2.0 * (t8 + t1) + 1.0; R[1] = 2.0 * (t6 - t4);       R[2] = 2.0 * (t3 + t7);
  R[3] = 2.0 * (t4 + t6);       R[4] = 2.0 * (t5 + t1) + 1.0; R[5] = 2.0 * (t9 - t2);
  R[6] = 2.0 * (t7 - t3);       R[7] = 2.0 * (t2 + t9);       R[8] = 2.0 * (t5 + t8) + 1.0;
}

// Image record k (and scalar slot k of zero[0..nzero) cleared): the body of
// pack_images_kernel, one thread per k.
__device__ inline void pack_image_record(const DevProblem& p, double* __restrict__ rec, double* __restrict__ zero,
                                         int nzero, int k) {
#pragma clang fp contract(fast)
  if (k < nzero) zero[k] = 0.0;
  if (k >= p.num_images) return;
  const uint32_t cam = p.img_cam[k];
  double* o = rec + kImgRec * (size_t)k;
#pragma unroll
  for (int m = 0; m < 7; ++m) o[m] = p.qt[8 * (size_t)k + m];
  o[7] = __longlong_as_double(
      (long long)(p.img_flags[k] | ((p.cam_var[cam] != 0 ? 1u : 0u) << 8) | ((uint32_t)p.cam_model[cam] << 16)));
  const double q[4] = {o[0], o[1], o[2], o[3]};
  double R[9];
  unit_quat_matrix_contracted(q, R);
#pragma unroll
  for (int m = 0; m < 9; ++m) o[16 + m] = R[m];
  o[25] = fabs(q[0] * q[0] + q[1] * q[1] + q[2] * q[2] + q[3] * q[3] - 1.0) <= 1e-12 ? 1.0 : 0.0;
#pragma unroll
  for (int m = 26; m < kImgRec; ++m) o[m] = 0.0;
  // the camera's parameters last: copied when the rotation's registers are free
#pragma unroll
  for (int m = 0; m < 8; ++m) o[8 + m] = p.cam[8 * (size_t)cam + m];
}

// The input warm-up's ranges (launch_touch_inputs): 16-B words of each.
struct TouchRanges {
  const uint4* ptr[5];
  int64_t n16[5];
};

// Grid-stride read of the ranges by workgroup `block` of `nblocks` 256-thread
// workgroups, U loads in flight per lane (the body of touch_kernel).  The
// values are dropped; the sink is written only for an impossible sum.
template <int U>
__device__ inline void touch_ranges(const TouchRanges& t, unsigned* sink, int block, int nblocks) {
  unsigned acc = 0u;
  const int64_t stride = (int64_t)nblocks * 256;
#pragma unroll
  for (int q = 0; q < 5; ++q) {
    const uint4* a = t.ptr[q];
    const int64_t n = t.n16[q];
    int64_t k = (int64_t)block * 256 + threadIdx.x;
    for (; k + (U - 1) * stride < n; k += U * stride) {
      uint4 v[U];
#pragma unroll
      for (int u = 0; u < U; ++u) v[u] = a[k + u * stride];  // U loads in flight per lane
#pragma unroll
      for (int u = 0; u < U; ++u) acc ^= v[u].x ^ v[u].w;
    }
    for (; k < n; k += stride) acc ^= a[k].x;
  }
  if (acc == 0x9e3779b9u && t.n16[0] < 0) *sink = acc;
}

// Value e of pair p's block from the deferred pass's chunk partials, summed
// in chunk order (the body of pair_reduce_kernel; a pair without deferred
// samples gets zeros: its cleared samples have J = 0).
// pair_block_sum: the sum itself over the pair's nch chunk rows, the first at c
// (semantic_pair_kernel sums the rows its own workgroup wrote: no restrict).
__device__ inline double pair_block_sum(const double* c, uint32_t nch, int vals) {
  double v = 0.0;
  for (uint32_t j = 0; j < nch; ++j) v += c[(size_t)j * vals];
  return v;
}

__device__ inline void pair_block_value(const uint32_t* __restrict__ pair_cnt,
                                        const uint32_t* __restrict__ pair_chunk0, const double* __restrict__ cpart,
                                        double* __restrict__ pair_blk, int vals, int blk_stride, int p, int e) {
  if (e >= vals) return;
  const uint32_t nch = (pair_cnt[p] + 63) / 64;
  pair_blk[(size_t)p * blk_stride + e] = pair_block_sum(cpart + (size_t)pair_chunk0[p] * vals + e, nch, vals);
}

}  // namespace miba
