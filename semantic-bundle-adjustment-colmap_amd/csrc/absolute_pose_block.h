// absolute_pose_block.h — host/device math of the robust absolute pose
// (EstimateAbsolutePose, src/estimators/pose.cc:50-158): LiftImagePoint,
// P3PEstimator::Estimate and EPNPEstimator of src/estimators/absolute_pose.cc,
// ComputeSquaredReprojectionError (src/estimators/utils.cc:133-185),
// InlierSupportMeasurer, RANSAC's ComputeNumTrials for three samples
// (src/optim/ransac.h:159-180), a counter-based replacement of RandomSampler
// and, for the host, the whole LO-RANSAC of src/optim/loransac.h:88-249 as one
// sequential function.  Included by absolute_pose.hip and, compiled for the
// host, by tests/cpp/absolute_pose_block_test.cc and include/colmap_amd/pose.h.
//
// Eigen's EigenSolver, JacobiSVD and ColPivHouseholderQR are not restated:
//   - the quartic's roots come from a fixed-count Aberth iteration in complex
//     arithmetic with a guarded Newton polish of the real ones;
//   - every 3 x 3 SVD is used only as U V' with the reflection fix, which is
//     the proper rotation nearest the matrix: a one-sided (Hestenes) Jacobi,
//     the third singular pair completed by cross products, so a rank-2
//     covariance (three points, a planar inlier set) is the regular case;
//   - the eigenvectors of M'M come from a cyclic Jacobi on the symmetric
//     12 x 12 with a fixed sweep cap;
//   - the 6 x k least-squares solves and the Gauss-Newton step use one
//     Householder QR with column pivoting.
// Build decisions (documented in mi_ba.h): the models of one trial are taken
// in ascending order of the root x; the sampler is stateless.
//
// EPnP's sums over the inlier set go through a "set" type: the host's walks
// the correspondences in order (the reference's order), the kernel's strides
// them over the lanes of a wave and adds with a fixed butterfly.  The small
// dense algebra between the sums runs on the set's leader only and leaves its
// results in a workspace that every lane reads after a sync.
#pragma once

#include <cfloat>
#include <cmath>
#include <cstdint>

#include "ba_math.h"

#if defined(__HIPCC__)
#define MI_AP_NOUNROLL _Pragma("unroll 1")
// the leader's dense algebra: out of line, so that it costs the trial loop no register
#define MI_AP_FN __host__ __device__ inline __attribute__((noinline))
#else
#define MI_AP_NOUNROLL
#define MI_AP_FN inline
#endif

namespace miba {

// One correspondence: the normalised image point and the 3D point.
enum { kApX = 0, kApY = 1, kApW = 2, kApRecord = 5 };
constexpr int64_t kApMaxTrials = INT64_MAX;  // stands for size_t's maximum
constexpr int kApMaxLocalTrials = 10;        // loransac.h:160
constexpr int kApRootIters = 48;             // Aberth iterations, at most
constexpr int kApSweeps = 30;                // Jacobi sweeps, at most
constexpr double kApMaxRootImag = 1e-10;     // absolute_pose.cc:111

struct ApRecords {
  double* base;
  MI_HD double& at(int64_t i, int f) const { return base[i * kApRecord + f]; }
};

// RANSACOptions after the constructor's cap; max_residual is already
// (max_error / mean focal length)^2.
struct ApOptions {
  double max_residual, confidence, dyn_num_trials_multiplier;
  int64_t max_num_trials;
};

struct ApResult {
  double P[12], qvec[4], tvec[3];
  int64_t num_trials;
  int32_t success, num_inliers, best_is_local, pad;
};

// ---- RANSAC::ComputeNumTrials for kMinNumSamples = 3 (ransac.h:159-180) ----
// std::pow(r, 3) is written r * r * r (one rounding more; the device has no
// correctly rounded pow).  size_t's maximum is kApMaxTrials.
MI_HD int64_t ap_compute_num_trials(int64_t num_inliers, int64_t num_samples, double confidence, double multiplier) {
  const double inlier_ratio = (double)num_inliers / (double)num_samples;
  const double nom = 1.0 - confidence;
  if (nom <= 0.0) return kApMaxTrials;
  const double denom = 1.0 - inlier_ratio * inlier_ratio * inlier_ratio;
  if (denom <= 0.0) return 1;
  if (denom == 1.0) return kApMaxTrials;
  const double x = ceil(log(nom) / log(denom) * multiplier);
  if (!(x >= 0.0) || !(x < 9.2e18)) return kApMaxTrials;
  return (int64_t)x;
}

// The constructor's cap of max_num_trials (ransac.h:146-156).
MI_HD int64_t ap_constructor_cap(int64_t max_num_trials, double min_inlier_ratio, double confidence, double multiplier) {
  const int64_t dyn = ap_compute_num_trials((int64_t)(min_inlier_ratio * 100000.0), 100000, confidence, multiplier);
  return dyn < max_num_trials ? dyn : max_num_trials;
}

// ---- the sampler ----
// Trial t of the problem with seed s: the first three steps of a Fisher-Yates
// shuffle of the identity permutation of n >= 3 elements, j_i uniform in
// [i, n - 1].  j_i = i + mulhi(r_i, n - i) with r_i = mix(mix(mix(s) ^ t) ^ i),
// mix = splitmix64's finaliser; the multiply-high reduction is biased by at
// most (n - i) / 2^64.  Same distribution as RandomSampler::Sample
// (optim/random_sampler.cc), no state, so trials are independent.
MI_HD uint64_t ap_mix64(uint64_t z) {
  z += 0x9E3779B97F4A7C15ull;
  z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
  z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
  return z ^ (z >> 31);
}

MI_HD uint64_t ap_mulhi64(uint64_t a, uint64_t b) {
#if defined(__HIP_DEVICE_COMPILE__)
  return __umul64hi(a, b);
#else
  return (uint64_t)(((unsigned __int128)a * (unsigned __int128)b) >> 64);
#endif
}

MI_HD void ap_sample(uint64_t seed, int64_t t, int64_t n, int64_t idx[3]) {
  const uint64_t h = ap_mix64(ap_mix64(seed) ^ (uint64_t)t);
  const int64_t j0 = (int64_t)ap_mulhi64(ap_mix64(h ^ 0ull), (uint64_t)n);
  const int64_t j1 = 1 + (int64_t)ap_mulhi64(ap_mix64(h ^ 1ull), (uint64_t)(n - 1));
  const int64_t j2 = 2 + (int64_t)ap_mulhi64(ap_mix64(h ^ 2ull), (uint64_t)(n - 2));
  // perm = identity; swap(perm[0], perm[j0]); swap(perm[1], perm[j1]); swap(perm[2], perm[j2])
  idx[0] = j0;
  // after step 0: perm[0] = j0, perm[j0] = 0
  const int64_t p1 = j0 == 1 ? 0 : 1;            // perm[1] before step 1
  idx[1] = j1 == j0 ? 0 : (j1 == 1 ? p1 : j1);   // perm[j1] before step 1
  // after step 1: perm[1] = idx[1], perm[j1] = p1
  int64_t p2 = j0 == 2 ? 0 : 2;                  // perm[2] after step 0
  if (j1 == 2) p2 = p1;                          // ... after step 1
  int64_t pj2 = j2 == j0 ? 0 : j2;               // perm[j2] after step 0
  if (j2 == j1) pj2 = p1;                        // ... after step 1
  idx[2] = j2 == 2 ? p2 : pj2;
}

// ---- residuals and support ----
// LiftImagePoint (absolute_pose.cc:41-43).
MI_HD void ap_lift(double x, double y, double u[3]) {
  const double n = sqrt(x * x + y * y + 1.0);
  u[0] = x / n;
  u[1] = y / n;
  u[2] = 1.0 / n;
}

// ComputeSquaredReprojectionError for one correspondence (utils.cc:157-181).
MI_HD double ap_squared_error(double x, double y, const double X[3], const double P[12]) {
  const double pz = P[8] * X[0] + P[9] * X[1] + P[10] * X[2] + P[11];
  if (pz > DBL_EPSILON) {
    const double px = P[0] * X[0] + P[1] * X[1] + P[2] * X[2] + P[3];
    const double py = P[4] * X[0] + P[5] * X[1] + P[6] * X[2] + P[7];
    const double inv = 1.0 / pz;
    const double dx = x - px * inv, dy = y - py * inv;
    return dx * dx + dy * dy;
  }
  return DBL_MAX;
}

template <typename Rec>
MI_HD double ap_residual(const Rec& rec, int64_t i, const double P[12]) {
  const double X[3] = {rec.at(i, kApW), rec.at(i, kApW + 1), rec.at(i, kApW + 2)};
  return ap_squared_error(rec.at(i, kApX), rec.at(i, kApY), X, P);
}

// InlierSupportMeasurer::Compare (support_measurement.cc): strict.
MI_HD bool ap_better(int64_t n1, double s1, int64_t n2, double s2) { return n1 > n2 || (n1 == n2 && s1 < s2); }

// InlierSupportMeasurer::Evaluate over the whole problem in order.
template <typename Rec>
MI_HD void ap_support(const Rec& rec, int64_t n, const double P[12], double max_residual, int64_t* num_inliers,
                      double* residual_sum) {
  int64_t ni = 0;
  double sum = 0.0;
  MI_AP_NOUNROLL
  for (int64_t i = 0; i < n; ++i) {
    const double r = ap_residual(rec, i, P);
    if (r <= max_residual) {
      ni += 1;
      sum += r;
    }
  }
  *num_inliers = ni;
  *residual_sum = sum;
}

// ---- small dense pieces ----
MI_HD void ap_cross(const double a[3], const double b[3], double c[3]) {
  c[0] = a[1] * b[2] - a[2] * b[1];
  c[1] = a[2] * b[0] - a[0] * b[2];
  c[2] = a[0] * b[1] - a[1] * b[0];
}

// U diag(1, 1, det(U V')) V' of the SVD A = U S V' (A row-major): what
// Eigen::umeyama (Umeyama.h) and EPNPEstimator::EstimateRT
// (absolute_pose.cc:569-588) make of their covariance.  One-sided Jacobi on
// the columns of A; the pair of the smallest singular value is replaced by the
// cross products of the other two, which gives the same matrix and needs no
// third singular vector of a rank-2 A.  Static indexing only.
MI_HD void ap_rotation_from_covariance(const double A[9], double R[9]) {
  double u0[3] = {A[0], A[3], A[6]}, u1[3] = {A[1], A[4], A[7]}, u2[3] = {A[2], A[5], A[8]};
  double v0[3] = {1.0, 0.0, 0.0}, v1[3] = {0.0, 1.0, 0.0}, v2[3] = {0.0, 0.0, 1.0};
  bool rotated = true;
  MI_AP_NOUNROLL
  for (int sweep = 0; sweep < kApSweeps && rotated; ++sweep) {
    rotated = false;
    MI_UNROLL
    for (int pair = 0; pair < 3; ++pair) {
      // (0,1), (0,2), (1,2)
      double* up = pair == 2 ? u1 : u0;
      double* uq = pair == 0 ? u1 : u2;
      double* vp = pair == 2 ? v1 : v0;
      double* vq = pair == 0 ? v1 : v2;
      const double alpha = up[0] * up[0] + up[1] * up[1] + up[2] * up[2];
      const double beta = uq[0] * uq[0] + uq[1] * uq[1] + uq[2] * uq[2];
      const double gamma = up[0] * uq[0] + up[1] * uq[1] + up[2] * uq[2];
      if (fabs(gamma) > DBL_EPSILON * sqrt(alpha * beta)) {
        rotated = true;
        const double zeta = (beta - alpha) / (2.0 * gamma);
        const double t = (zeta >= 0.0 ? 1.0 : -1.0) / (fabs(zeta) + sqrt(1.0 + zeta * zeta));
        const double c = 1.0 / sqrt(1.0 + t * t), s = c * t;
        MI_UNROLL
        for (int k = 0; k < 3; ++k) {
          const double a = up[k], b = uq[k], d = vp[k], e = vq[k];
          up[k] = c * a - s * b;
          uq[k] = s * a + c * b;
          vp[k] = c * d - s * e;
          vq[k] = s * d + c * e;
        }
      }
    }
  }
  double n0 = u0[0] * u0[0] + u0[1] * u0[1] + u0[2] * u0[2];
  double n1 = u1[0] * u1[0] + u1[1] * u1[1] + u1[2] * u1[2];
  double n2 = u2[0] * u2[0] + u2[1] * u2[1] + u2[2] * u2[2];
  // the two columns of the largest norms into (a, b)
  double a[3], b[3], va[3], vb[3], na, nb;
  const bool drop0 = n0 <= n1 && n0 <= n2;
  const bool drop1 = !drop0 && n1 <= n2;
  MI_UNROLL
  for (int k = 0; k < 3; ++k) {
    a[k] = drop0 ? u1[k] : u0[k];
    va[k] = drop0 ? v1[k] : v0[k];
    b[k] = (drop0 || drop1) ? u2[k] : u1[k];
    vb[k] = (drop0 || drop1) ? v2[k] : v1[k];
  }
  na = sqrt(drop0 ? n1 : n0);
  nb = sqrt((drop0 || drop1) ? n2 : n1);
  MI_UNROLL
  for (int k = 0; k < 3; ++k) {
    a[k] /= na;
    b[k] /= nb;
  }
  double c[3], vc[3];
  ap_cross(a, b, c);
  ap_cross(va, vb, vc);
  MI_UNROLL
  for (int r = 0; r < 3; ++r) {
    MI_UNROLL
    for (int q = 0; q < 3; ++q) R[3 * r + q] = a[r] * va[q] + b[r] * vb[q] + c[r] * vc[q];
  }
}

// Eigen::Quaterniond(R) as (w, x, y, z) (RotationMatrixToQuaternion, base/pose.cc).
MI_HD void ap_rotation_to_quaternion(const double P[12], double q[4]) {
  const double m00 = P[0], m01 = P[1], m02 = P[2], m10 = P[4], m11 = P[5], m12 = P[6], m20 = P[8], m21 = P[9],
               m22 = P[10];
  double t = m00 + m11 + m22;
  if (t > 0.0) {
    t = sqrt(t + 1.0);
    q[0] = 0.5 * t;
    t = 0.5 / t;
    q[1] = (m21 - m12) * t;
    q[2] = (m02 - m20) * t;
    q[3] = (m10 - m01) * t;
  } else if (!(m11 > m00) && !(m22 > m00)) {  // i = 0, j = 1, k = 2
    t = sqrt(m00 - m11 - m22 + 1.0);
    q[1] = 0.5 * t;
    t = 0.5 / t;
    q[0] = (m21 - m12) * t;
    q[2] = (m10 + m01) * t;
    q[3] = (m20 + m02) * t;
  } else if (m11 > m00 && !(m22 > m11)) {  // i = 1, j = 2, k = 0
    t = sqrt(m11 - m22 - m00 + 1.0);
    q[2] = 0.5 * t;
    t = 0.5 / t;
    q[0] = (m02 - m20) * t;
    q[3] = (m21 + m12) * t;
    q[1] = (m01 + m10) * t;
  } else {  // i = 2, j = 0, k = 1
    t = sqrt(m22 - m00 - m11 + 1.0);
    q[3] = 0.5 * t;
    t = 0.5 / t;
    q[0] = (m10 - m01) * t;
    q[1] = (m02 + m20) * t;
    q[2] = (m12 + m21) * t;
  }
}

// ---- the quartic ----
// The real roots (|imag| <= kApMaxRootImag) of c[0] x^4 + ... + c[4], in
// ascending order; returns how many.  Aberth's simultaneous iteration from
// four points on a circle of Fujiwara's radius, at most kApRootIters rounds;
// coefficients that are not finite, or a leading one that is zero, give no
// root.  A real root is polished by two Newton steps, each taken only if it
// is small (so a near-double root is not thrown to its neighbour).
MI_HD int ap_quartic_real_roots(const double c[5], double roots[4]) {
  const double b1 = c[1] / c[0], b2 = c[2] / c[0], b3 = c[3] / c[0], b4 = c[4] / c[0];
  if (!(fabs(b1) <= DBL_MAX) || !(fabs(b2) <= DBL_MAX) || !(fabs(b3) <= DBL_MAX) || !(fabs(b4) <= DBL_MAX)) return 0;
  double rad = fabs(b1);
  const double r2 = sqrt(fabs(b2)), r3 = cbrt(fabs(b3)), r4 = sqrt(sqrt(fabs(b4)));
  rad = rad > r2 ? rad : r2;
  rad = rad > r3 ? rad : r3;
  rad = rad > r4 ? rad : r4;
  if (rad == 0.0) {  // x^4 = 0
    roots[0] = 0.0;
    return 1;
  }
  // cos / sin of 0.7 + k pi / 2
  const double c0 = 0.76484218728448842626, s0 = 0.64421768723769105367;
  double zr0 = rad * c0, zi0 = rad * s0, zr1 = -rad * s0, zi1 = rad * c0;
  double zr2 = -rad * c0, zi2 = -rad * s0, zr3 = rad * s0, zi3 = -rad * c0;
  MI_AP_NOUNROLL
  for (int it = 0; it < kApRootIters; ++it) {
    double moved = 0.0;
    MI_AP_NOUNROLL
    for (int k = 0; k < 4; ++k) {
      // rotate the roles so that root k is (zr0, zi0): static registers only
      const double xr = zr0, xi = zi0;
      // p and p' by Horner
      double pr = 1.0, pi = 0.0, dr = 0.0, di = 0.0;
      const double bs[4] = {b1, b2, b3, b4};
      MI_UNROLL
      for (int m = 0; m < 4; ++m) {
        const double ndr = dr * xr - di * xi + pr, ndi = dr * xi + di * xr + pi;
        dr = ndr;
        di = ndi;
        const double npr = pr * xr - pi * xi + bs[m], npi = pr * xi + pi * xr;
        pr = npr;
        pi = npi;
      }
      // w = p / p'
      const double dd = dr * dr + di * di;
      double wr = (pr * dr + pi * di) / dd, wi = (pi * dr - pr * di) / dd;
      if (dd == 0.0) {
        wr = (pr == 0.0 && pi == 0.0) ? 0.0 : 1e-3 * rad;
        wi = 0.0;
      }
      // s = sum 1 / (x - z_j)
      double sr = 0.0, si = 0.0;
      {
        const double ar = xr - zr1, ai = xi - zi1, am = ar * ar + ai * ai;
        if (am > 0.0) {
          sr += ar / am;
          si -= ai / am;
        }
        const double br = xr - zr2, bi = xi - zi2, bm = br * br + bi * bi;
        if (bm > 0.0) {
          sr += br / bm;
          si -= bi / bm;
        }
        const double cr = xr - zr3, ci = xi - zi3, cm = cr * cr + ci * ci;
        if (cm > 0.0) {
          sr += cr / cm;
          si -= ci / cm;
        }
      }
      // x -= w / (1 - w s)
      const double er = 1.0 - (wr * sr - wi * si), ei = -(wr * si + wi * sr), em = er * er + ei * ei;
      double tr = wr, ti = wi;
      if (em > 0.0) {
        tr = (wr * er + wi * ei) / em;
        ti = (wi * er - wr * ei) / em;
      }
      const double nr = xr - tr, ni = xi - ti;
      const double step = fabs(tr) + fabs(ti);
      const double size = fabs(nr) + fabs(ni);
      if (!(step <= 4.0 * DBL_EPSILON * size)) moved = 1.0;
      // rotate: (1, 2, 3, new 0)
      zr0 = zr1;
      zi0 = zi1;
      zr1 = zr2;
      zi1 = zi2;
      zr2 = zr3;
      zi2 = zi3;
      zr3 = nr;
      zi3 = ni;
    }
    if (moved == 0.0) break;
  }
  int count = 0;
  const double zr[4] = {zr0, zr1, zr2, zr3}, zi[4] = {zi0, zi1, zi2, zi3};
  double out[4] = {0.0, 0.0, 0.0, 0.0};
  MI_UNROLL
  for (int k = 0; k < 4; ++k) {
    double x = zr[k];
    const bool real = fabs(zi[k]) <= kApMaxRootImag && fabs(x) <= DBL_MAX;
    if (real) {
      MI_UNROLL
      for (int polish = 0; polish < 2; ++polish) {
        const double p = (((x + b1) * x + b2) * x + b3) * x + b4;
        const double d = ((4.0 * x + 3.0 * b1) * x + 2.0 * b2) * x + b3;
        const double s = p / d;
        if (fabs(s) <= 1e-6 * (fabs(x) > 1.0 ? fabs(x) : 1.0)) x -= s;
      }
    }
    // insertion into the ascending prefix, with static indices
    double v = real ? x : DBL_MAX;
    MI_UNROLL
    for (int m = 0; m < 4; ++m) {
      if (m <= k) {
        const bool take = m < count ? v < out[m] : m == count;
        if (m < count + 1 && take) {
          const double tmp = out[m];
          out[m] = v;
          v = tmp;
        }
      }
    }
    if (real) count += 1;
  }
  MI_UNROLL
  for (int k = 0; k < 4; ++k) roots[k] = out[k];
  return count;
}

// ---- P3PEstimator::Estimate (absolute_pose.cc:47-174) ----
// What the models of one sample share.
struct ApP3P {
  double u[3], v[3], w[3], A[3], B[3], C[3];
  double cos_uv, dist_AB, a, b, p, q, r;
  double x[4];
  int count;
};

template <typename Rec>
MI_HD void ap_p3p_roots(const Rec& rec, int64_t i0, int64_t i1, int64_t i2, ApP3P* s) {
  ap_lift(rec.at(i0, kApX), rec.at(i0, kApY), s->u);
  ap_lift(rec.at(i1, kApX), rec.at(i1, kApY), s->v);
  ap_lift(rec.at(i2, kApX), rec.at(i2, kApY), s->w);
  MI_UNROLL
  for (int m = 0; m < 3; ++m) {
    s->A[m] = rec.at(i0, kApW + m);
    s->B[m] = rec.at(i1, kApW + m);
    s->C[m] = rec.at(i2, kApW + m);
  }
  const double cos_uv = s->u[0] * s->v[0] + s->u[1] * s->v[1] + s->u[2] * s->v[2];
  const double cos_uw = s->u[0] * s->w[0] + s->u[1] * s->w[1] + s->u[2] * s->w[2];
  const double cos_vw = s->v[0] * s->w[0] + s->v[1] * s->w[1] + s->v[2] * s->w[2];
  double dist_AB_2 = 0.0, dist_AC_2 = 0.0, dist_BC_2 = 0.0;
  MI_UNROLL
  for (int m = 0; m < 3; ++m) {
    dist_AB_2 += (s->A[m] - s->B[m]) * (s->A[m] - s->B[m]);
    dist_AC_2 += (s->A[m] - s->C[m]) * (s->A[m] - s->C[m]);
    dist_BC_2 += (s->B[m] - s->C[m]) * (s->B[m] - s->C[m]);
  }
  s->cos_uv = cos_uv;
  s->dist_AB = sqrt(dist_AB_2);
  const double a = dist_BC_2 / dist_AB_2, b = dist_AC_2 / dist_AB_2;
  const double a2 = a * a, b2 = b * b;
  const double p = 2 * cos_vw, q = 2 * cos_uw, r = 2 * cos_uv;
  const double p2 = p * p, q2 = q * q, r2 = r * r;
  s->a = a;
  s->b = b;
  s->p = p;
  s->q = q;
  s->r = r;
  double coeffs[5];
  coeffs[0] = -2 * b + b2 + a2 + 1 + a * b * (2 - r2) - 2 * a;
  coeffs[1] = -2 * q * a2 - r * p * b2 + 4 * q * a + (2 * q + p * r) * b + (r2 * q - 2 * q + r * p) * a * b - 2 * q;
  coeffs[2] = (2 + q2) * a2 + (p2 + r2 - 2) * b2 - (4 + 2 * q2) * a - (p * q * r + p2) * b -
              (p * q * r + r2) * a * b + q2 + 2;
  coeffs[3] = -2 * q * a2 - r * p * b2 + 4 * q * a + (p * r + q * p2 - 2 * q) * b + (r * p + 2 * q) * a * b - 2 * q;
  coeffs[4] = a2 + b2 - 2 * a + (2 - p2) * b - 2 * a * b + 1;
  double roots[4];
  const int nr = ap_quartic_real_roots(coeffs, roots);
  int count = 0;
  MI_UNROLL
  for (int k = 0; k < 4; ++k) s->x[k] = 0.0;
  // keep x >= 0; ascending order survives
  MI_UNROLL
  for (int k = 0; k < 4; ++k) {
    if (k < nr && !(roots[k] < 0.0)) {
      MI_UNROLL
      for (int m = 0; m < 4; ++m)
        if (m == count) s->x[m] = roots[k];
      count += 1;
    }
  }
  s->count = count;
}

// The model of root x (absolute_pose.cc:116-170): y = b0 / b1, the depths,
// Eigen::umeyama(world, camera, false) on the three points.
MI_HD void ap_p3p_model(const ApP3P& s, double x, double P[12]) {
  const double a = s.a, b = s.b, p = s.p, q = s.q, r = s.r;
  const double a2 = a * a, b2 = b * b, p2 = p * p, p3 = p2 * p, q2 = q * q, r2 = r * r, r3 = r2 * r, r4 = r3 * r,
               r5 = r4 * r;
  const double x2 = x * x, x3 = x2 * x;
  const double bb1 = (p2 - p * q * r + r2) * a + (p2 - r2) * b - p2 + p * q * r - r2;
  const double b1 = b * bb1 * bb1;
  const double b0 =
      ((1 - a - b) * x2 + (a - 1) * q * x - a + b + 1) *
      (r3 * (a2 + b2 - 2 * a - 2 * b + (2 - r2) * a * b + 1) * x3 +
       r2 *
           (p + p * a2 - 2 * r * q * a * b + 2 * r * q * b - 2 * r * q - 2 * p * a - 2 * p * b + p * r2 * b +
            4 * r * q * a + q * r3 * a * b - 2 * r * q * a2 + 2 * p * a * b + p * b2 - r2 * p * b2) *
           x2 +
       (r5 * (b2 - a * b) - r4 * p * q * b + r3 * (q2 - 4 * a - 2 * q2 * a + q2 * a2 + 2 * a2 - 2 * b2 + 2) +
        r2 * (4 * p * q * a - 2 * p * q * a * b + 2 * p * q * b - 2 * p * q - 2 * p * q * a2) +
        r * (p2 * b2 - 2 * p2 * b + 2 * p2 * a * b - 2 * p2 * a + p2 + p2 * a2)) *
           x +
       (2 * p * r2 - 2 * r3 * q + p3 - 2 * p2 * q * r + p * q2 * r2) * a2 + (p3 - 2 * p * r2) * b2 +
       (4 * q * r3 - 4 * p * r2 - 2 * p3 + 4 * p2 * q * r - 2 * p * q2 * r2) * a +
       (-2 * q * r3 + p * r4 + 2 * p2 * q * r - 2 * p3) * b + (2 * p3 + 2 * q * r3 - 2 * p2 * q * r) * a * b +
       p * q2 * r2 - 2 * p2 * q * r + 2 * p * r2 + p3 - 2 * r3 * q);
  const double y = b0 / b1;
  const double y2 = y * y;
  const double nu = x2 + y2 - 2 * x * y * s.cos_uv;
  const double dist_PC = s.dist_AB / sqrt(nu);
  const double dist_PB = y * dist_PC;
  const double dist_PA = x * dist_PC;
  double cam[3][3];  // A', B', C'
  MI_UNROLL
  for (int m = 0; m < 3; ++m) {
    cam[0][m] = s.u[m] * dist_PA;
    cam[1][m] = s.v[m] * dist_PB;
    cam[2][m] = s.w[m] * dist_PC;
  }
  // umeyama without scaling: src = world, dst = camera
  double sm[3], dm[3];
  MI_UNROLL
  for (int m = 0; m < 3; ++m) {
    sm[m] = (s.A[m] + s.B[m] + s.C[m]) / 3.0;
    dm[m] = (cam[0][m] + cam[1][m] + cam[2][m]) / 3.0;
  }
  double S[9];
  MI_UNROLL
  for (int i = 0; i < 3; ++i) {
    MI_UNROLL
    for (int j = 0; j < 3; ++j)
      S[3 * i + j] = ((cam[0][i] - dm[i]) * (s.A[j] - sm[j]) + (cam[1][i] - dm[i]) * (s.B[j] - sm[j]) +
                      (cam[2][i] - dm[i]) * (s.C[j] - sm[j])) /
                     3.0;
  }
  double R[9];
  ap_rotation_from_covariance(S, R);
  MI_UNROLL
  for (int i = 0; i < 3; ++i) {
    MI_UNROLL
    for (int j = 0; j < 3; ++j) P[4 * i + j] = R[3 * i + j];
    P[4 * i + 3] = dm[i] - (R[3 * i] * sm[0] + R[3 * i + 1] * sm[1] + R[3 * i + 2] * sm[2]);
  }
}

// ---- dense algebra of EPnP on the leader, over a workspace ----
// Layout of the workspace (doubles).
enum {
  kApWsA = 0,        // 12 x 12 M'M, diagonalised in place
  kApWsV = 144,      // 12 x 12 eigenvectors, columns
  kApWsUt = 288,     // 4 x 12: row i is the reference's Ut(11 - i)
  kApWsL = 336,      // L6x10
  kApWsRho = 396,    // rho
  kApWsBetas = 402,  // 3 x 4
  kApWsLs = 414,     // 6 x 5 least-squares matrix, its right-hand side 6, column norms 5, permutation 5
  kApWsOk = 460,     // 1: the rank test passed
  kApWsCws = 461,    // 4 x 3 control points
  kApWsCCinv = 473,  // 3 x 3
  kApWsRt = 482,     // R 3 x 3, t 3
  kApWsIn = 496,     // what the leader hands in: up to 40 sums
  kApWsSize = 536
};

// Cyclic Jacobi on the symmetric n x n A (row-major, overwritten by its
// diagonal form), V its eigenvectors in columns; at most kApSweeps sweeps.
MI_AP_FN void ap_sym_jacobi(double* A, double* V, int n) {
  for (int r = 0; r < n; ++r)
    for (int c = 0; c < n; ++c) V[r * n + c] = r == c ? 1.0 : 0.0;
  bool rotated = true;
  MI_AP_NOUNROLL
  for (int sweep = 0; sweep < kApSweeps && rotated; ++sweep) {
    rotated = false;
    MI_AP_NOUNROLL
    for (int p = 0; p < n - 1; ++p) {
      MI_AP_NOUNROLL
      for (int q = p + 1; q < n; ++q) {
        const double apq = A[p * n + q];
        if (fabs(apq) > DBL_EPSILON * sqrt(fabs(A[p * n + p] * A[q * n + q]))) {
          rotated = true;
          const double theta = (A[q * n + q] - A[p * n + p]) / (2.0 * apq);
          const double t = (theta >= 0.0 ? 1.0 : -1.0) / (fabs(theta) + sqrt(1.0 + theta * theta));
          const double c = 1.0 / sqrt(1.0 + t * t), s = c * t;
          MI_AP_NOUNROLL
          for (int k = 0; k < n; ++k) {
            const double akp = A[k * n + p], akq = A[k * n + q];
            A[k * n + p] = c * akp - s * akq;
            A[k * n + q] = s * akp + c * akq;
          }
          MI_AP_NOUNROLL
          for (int k = 0; k < n; ++k) {
            const double apk = A[p * n + k], aqk = A[q * n + k];
            A[p * n + k] = c * apk - s * aqk;
            A[q * n + k] = s * apk + c * aqk;
          }
          MI_AP_NOUNROLL
          for (int k = 0; k < n; ++k) {
            const double vp = V[k * n + p], vq = V[k * n + q];
            V[k * n + p] = c * vp - s * vq;
            V[k * n + q] = s * vp + c * vq;
          }
        }
      }
    }
  }
}

// min |A x - b| for the 6 x k A (row-major, stride 5, overwritten; b too):
// Householder QR with column pivoting; a column whose remaining norm is at or
// below 1e-12 of the largest initial one is rank deficiency and its unknown
// is 0 (the basic solution; JacobiSVD::solve gives the minimum-norm one, the
// same at full rank).  ws: kApWsLs.
MI_AP_FN void ap_lstsq6(double* ws, int k, double* x) {
  double* A = ws;
  double* b = ws + 30;
  double* perm = ws + 41;
  for (int c = 0; c < k; ++c) perm[c] = (double)c;
  double scale = 0.0;
  for (int c = 0; c < k; ++c) {
    double s = 0.0;
    for (int r = 0; r < 6; ++r) s += A[r * 5 + c] * A[r * 5 + c];
    scale = s > scale ? s : scale;
  }
  int rank = 0;
  MI_AP_NOUNROLL
  for (int j = 0; j < k; ++j) {
    int best = j;
    double bn = -1.0;
    for (int c = j; c < k; ++c) {
      double s = 0.0;
      for (int r = j; r < 6; ++r) s += A[r * 5 + c] * A[r * 5 + c];
      if (s > bn) {
        bn = s;
        best = c;
      }
    }
    if (!(bn > 1e-24 * scale)) break;
    if (best != j) {
      for (int r = 0; r < 6; ++r) {
        const double t = A[r * 5 + j];
        A[r * 5 + j] = A[r * 5 + best];
        A[r * 5 + best] = t;
      }
      const double t = perm[j];
      perm[j] = perm[best];
      perm[best] = t;
    }
    // Householder vector of column j below the diagonal
    const double norm = sqrt(bn);
    const double ajj = A[j * 5 + j];
    const double alpha = ajj > 0.0 ? -norm : norm;
    const double v0 = ajj - alpha;
    double vv = v0 * v0;
    for (int r = j + 1; r < 6; ++r) vv += A[r * 5 + j] * A[r * 5 + j];
    if (vv > 0.0) {
      for (int c = j + 1; c <= k; ++c) {  // column k stands for b
        double dot = v0 * (c < k ? A[j * 5 + c] : b[j]);
        for (int r = j + 1; r < 6; ++r) dot += A[r * 5 + j] * (c < k ? A[r * 5 + c] : b[r]);
        const double f = 2.0 * dot / vv;
        if (c < k) {
          A[j * 5 + c] -= f * v0;
          for (int r = j + 1; r < 6; ++r) A[r * 5 + c] -= f * A[r * 5 + j];
        } else {
          b[j] -= f * v0;
          for (int r = j + 1; r < 6; ++r) b[r] -= f * A[r * 5 + j];
        }
      }
    }
    A[j * 5 + j] = alpha;
    rank = j + 1;
  }
  double* y = ws + 36;  // k values
  for (int c = 0; c < k; ++c) y[c] = 0.0;
  for (int j = rank - 1; j >= 0; --j) {
    double s = b[j];
    for (int c = j + 1; c < rank; ++c) s -= A[j * 5 + c] * y[c];
    y[j] = s / A[j * 5 + j];
  }
  for (int c = 0; c < k; ++c) x[(int)perm[c]] = y[c];
}

// RunGaussNewton (absolute_pose.cc:464-498).
MI_AP_FN void ap_gauss_newton(double* w, double* betas) {
  const double* L = w + kApWsL;
  const double* rho = w + kApWsRho;
  double* ls = w + kApWsLs;
  MI_AP_NOUNROLL
  for (int it = 0; it < 5; ++it) {
    const double b0 = betas[0], b1 = betas[1], b2 = betas[2], b3 = betas[3];
    for (int i = 0; i < 6; ++i) {
      const double* l = L + 10 * i;
      ls[i * 5 + 0] = 2 * l[0] * b0 + l[1] * b1 + l[3] * b2 + l[6] * b3;
      ls[i * 5 + 1] = l[1] * b0 + 2 * l[2] * b1 + l[4] * b2 + l[7] * b3;
      ls[i * 5 + 2] = l[3] * b0 + l[4] * b1 + 2 * l[5] * b2 + l[8] * b3;
      ls[i * 5 + 3] = l[6] * b0 + l[7] * b1 + l[8] * b2 + 2 * l[9] * b3;
      ls[30 + i] = rho[i] - (l[0] * b0 * b0 + l[1] * b0 * b1 + l[2] * b1 * b1 + l[3] * b0 * b2 + l[4] * b1 * b2 +
                             l[5] * b2 * b2 + l[6] * b0 * b3 + l[7] * b1 * b3 + l[8] * b2 * b3 + l[9] * b3 * b3);
    }
    double x[4];
    ap_lstsq6(ls, 4, x);
    for (int m = 0; m < 4; ++m) betas[m] += x[m];
  }
}

// ChooseControlPoints' decomposition and ComputeBarycentricCoordinates' rank
// test and inverse (absolute_pose.cc:257-307).  In the workspace's input area:
// the centroid c0, then the upper triangle of PW0' PW0 (xx, xy, xz, yy, yz,
// zz); count: the set's size.  (The dense functions take their operands from
// the workspace, not from the caller's registers: an array handed to an
// out-of-line function by address would live in scratch memory on the device.)
// The pose EPnP returns depends on the signs of the principal axes: c_i and
// 2 c_0 - c_i give different barycentric coordinates, a different M and, with
// noisy data, a null space that differs at the level of the noise.  The
// reference takes the signs JacobiSVD happens to return; here every axis is
// oriented so that its component of the largest magnitude is positive (a build
// decision, documented in mi_ba.h).
// Rank test: in the spirit of colPivHouseholderQr().rank() < 3, whose
// threshold is 3 epsilon relative to the largest pivot: the axes of CC are
// orthogonal by construction, of lengths sqrt(D_i / n), so the set is rank
// deficient when the smallest length is at or below 3 epsilon of the largest.
MI_AP_FN void ap_epnp_control_points(double* w, double count) {
  const double* c0 = w + kApWsIn;
  const double* S = w + kApWsIn + 3;
  double* A = w + kApWsA;
  double* V = w + kApWsV;
  A[0] = S[0];
  A[1] = A[3] = S[1];
  A[2] = A[6] = S[2];
  A[4] = S[3];
  A[5] = A[7] = S[4];
  A[8] = S[5];
  ap_sym_jacobi(A, V, 3);
  // descending order of the eigenvalues, as the SVD's singular values
  int o[3] = {0, 1, 2};
  for (int i = 0; i < 2; ++i)
    for (int j = 0; j < 2 - i; ++j)
      if (A[4 * o[j]] < A[4 * o[j + 1]]) {
        const int t = o[j];
        o[j] = o[j + 1];
        o[j + 1] = t;
      }
  double* cws = w + kApWsCws;
  double len[3];
  for (int m = 0; m < 3; ++m) cws[m] = c0[m];
  for (int i = 0; i < 3; ++i) {
    const double d = A[4 * o[i]];
    len[i] = sqrt((d > 0.0 ? d : 0.0) / count);
    // the axis' sign: its component of the largest magnitude is positive (see above)
    int big = 0;
    for (int m = 1; m < 3; ++m)
      if (fabs(V[m * 3 + o[i]]) > fabs(V[big * 3 + o[i]])) big = m;
    const double sign = V[big * 3 + o[i]] < 0.0 ? -1.0 : 1.0;
    for (int m = 0; m < 3; ++m) cws[3 * (i + 1) + m] = c0[m] + len[i] * (sign * V[m * 3 + o[i]]);
  }
  const bool ok = len[0] > 0.0 && len[2] > 3.0 * DBL_EPSILON * len[0] && len[0] <= DBL_MAX;
  w[kApWsOk] = ok ? 1.0 : 0.0;
  if (!ok) return;
  // CC(i, j - 1) = cws[j][i] - cws[0][i]; its inverse by cofactors
  double CC[9];
  for (int i = 0; i < 3; ++i)
    for (int j = 1; j < 4; ++j) CC[3 * i + j - 1] = cws[3 * j + i] - cws[i];
  const double det = CC[0] * (CC[4] * CC[8] - CC[5] * CC[7]) - CC[1] * (CC[3] * CC[8] - CC[5] * CC[6]) +
                     CC[2] * (CC[3] * CC[7] - CC[4] * CC[6]);
  double* I = w + kApWsCCinv;
  I[0] = (CC[4] * CC[8] - CC[5] * CC[7]) / det;
  I[1] = (CC[2] * CC[7] - CC[1] * CC[8]) / det;
  I[2] = (CC[1] * CC[5] - CC[2] * CC[4]) / det;
  I[3] = (CC[5] * CC[6] - CC[3] * CC[8]) / det;
  I[4] = (CC[0] * CC[8] - CC[2] * CC[6]) / det;
  I[5] = (CC[2] * CC[3] - CC[0] * CC[5]) / det;
  I[6] = (CC[3] * CC[7] - CC[4] * CC[6]) / det;
  I[7] = (CC[1] * CC[6] - CC[0] * CC[7]) / det;
  I[8] = (CC[0] * CC[4] - CC[1] * CC[3]) / det;
}

// From the 40 sums of alpha_j alpha_k (1, x, y, x^2 + y^2) (j <= k) to the
// three betas (absolute_pose.cc:216-241, 325-498).  M'M = sum over the set of
// (alpha alpha') (x) B with B = [1 0 -x; 0 1 -y; -x -y x^2+y^2], so its 78
// distinct entries are these 40 sums and M is never stored.
MI_AP_FN void ap_epnp_betas(double* w) {
  const double* T = w + kApWsIn;
  double* A = w + kApWsA;
  double* V = w + kApWsV;
  int e = 0;
  for (int j = 0; j < 4; ++j)
    for (int k = j; k < 4; ++k) {
      const double s1 = T[4 * e], sx = T[4 * e + 1], sy = T[4 * e + 2], sr = T[4 * e + 3];
      const double B[9] = {s1, 0.0, -sx, 0.0, s1, -sy, -sx, -sy, sr};
      for (int c = 0; c < 3; ++c)
        for (int d = 0; d < 3; ++d) {
          A[(3 * j + c) * 12 + 3 * k + d] = B[3 * c + d];
          A[(3 * k + d) * 12 + 3 * j + c] = B[3 * c + d];
        }
      ++e;
    }
  ap_sym_jacobi(A, V, 12);
  // the four smallest eigenvalues, ascending: Ut(11), Ut(10), Ut(9), Ut(8)
  double* Ut = w + kApWsUt;
  int taken[4] = {-1, -1, -1, -1};
  for (int i = 0; i < 4; ++i) {
    int best = -1;
    for (int c = 0; c < 12; ++c) {
      if (c == taken[0] || c == taken[1] || c == taken[2] || c == taken[3]) continue;
      if (best < 0 || A[13 * c] < A[13 * best]) best = c;
    }
    taken[i] = best;
    for (int m = 0; m < 12; ++m) Ut[12 * i + m] = V[m * 12 + best];
  }
  // ComputeL6x10
  double* L = w + kApWsL;
  {
    int a = 0, b = 1;
    for (int j = 0; j < 6; ++j) {
      double dv[4][3];
      for (int i = 0; i < 4; ++i)
        for (int m = 0; m < 3; ++m) dv[i][m] = Ut[12 * i + 3 * a + m] - Ut[12 * i + 3 * b + m];
      auto dot = [&](int f, int g) { return dv[f][0] * dv[g][0] + dv[f][1] * dv[g][1] + dv[f][2] * dv[g][2]; };
      double* l = L + 10 * j;
      l[0] = dot(0, 0);
      l[1] = 2.0 * dot(0, 1);
      l[2] = dot(1, 1);
      l[3] = 2.0 * dot(0, 2);
      l[4] = 2.0 * dot(1, 2);
      l[5] = dot(2, 2);
      l[6] = 2.0 * dot(0, 3);
      l[7] = 2.0 * dot(1, 3);
      l[8] = 2.0 * dot(2, 3);
      l[9] = dot(3, 3);
      b += 1;
      if (b > 3) {
        a += 1;
        b = a + 1;
      }
    }
  }
  // ComputeRho
  double* rho = w + kApWsRho;
  const double* cws = w + kApWsCws;
  {
    int e2 = 0;
    for (int a = 0; a < 4; ++a)
      for (int b = a + 1; b < 4; ++b) {
        double s = 0.0;
        for (int m = 0; m < 3; ++m) s += (cws[3 * a + m] - cws[3 * b + m]) * (cws[3 * a + m] - cws[3 * b + m]);
        rho[e2++] = s;
      }
  }
  double* ls = w + kApWsLs;
  double* betas = w + kApWsBetas;
  // FindBetasApprox1: columns 0, 1, 3, 6
  {
    const int cols[4] = {0, 1, 3, 6};
    for (int i = 0; i < 6; ++i) {
      for (int c = 0; c < 4; ++c) ls[i * 5 + c] = L[10 * i + cols[c]];
      ls[30 + i] = rho[i];
    }
    double b4[4];
    ap_lstsq6(ls, 4, b4);
    double* bt = betas;
    if (b4[0] < 0) {
      bt[0] = sqrt(-b4[0]);
      bt[1] = -b4[1] / bt[0];
      bt[2] = -b4[2] / bt[0];
      bt[3] = -b4[3] / bt[0];
    } else {
      bt[0] = sqrt(b4[0]);
      bt[1] = b4[1] / bt[0];
      bt[2] = b4[2] / bt[0];
      bt[3] = b4[3] / bt[0];
    }
    ap_gauss_newton(w, bt);
  }
  // FindBetasApprox2: columns 0, 1, 2
  {
    for (int i = 0; i < 6; ++i) {
      for (int c = 0; c < 3; ++c) ls[i * 5 + c] = L[10 * i + c];
      ls[30 + i] = rho[i];
    }
    double b3[3];
    ap_lstsq6(ls, 3, b3);
    double* bt = betas + 4;
    if (b3[0] < 0) {
      bt[0] = sqrt(-b3[0]);
      bt[1] = (b3[2] < 0) ? sqrt(-b3[2]) : 0.0;
    } else {
      bt[0] = sqrt(b3[0]);
      bt[1] = (b3[2] > 0) ? sqrt(b3[2]) : 0.0;
    }
    if (b3[1] < 0) bt[0] = -bt[0];
    bt[2] = 0.0;
    bt[3] = 0.0;
    ap_gauss_newton(w, bt);
  }
  // FindBetasApprox3: columns 0 .. 4
  {
    for (int i = 0; i < 6; ++i) {
      for (int c = 0; c < 5; ++c) ls[i * 5 + c] = L[10 * i + c];
      ls[30 + i] = rho[i];
    }
    double b5[5];
    ap_lstsq6(ls, 5, b5);
    double* bt = betas + 8;
    if (b5[0] < 0) {
      bt[0] = sqrt(-b5[0]);
      bt[1] = (b5[2] < 0) ? sqrt(-b5[2]) : 0.0;
    } else {
      bt[0] = sqrt(b5[0]);
      bt[1] = (b5[2] > 0) ? sqrt(b5[2]) : 0.0;
    }
    if (b5[1] < 0) bt[0] = -bt[0];
    bt[2] = b5[3] / bt[0];
    bt[3] = 0.0;
    ap_gauss_newton(w, bt);
  }
}

// EstimateRT's decomposition (absolute_pose.cc:569-590) into w + kApWsRt.
MI_AP_FN void ap_epnp_rt(double* w) {
  const double* abt = w + kApWsIn;
  const double* pc0 = w + kApWsIn + 9;
  const double* pw0 = w + kApWsIn + 12;
  double R[9];
  ap_rotation_from_covariance(abt, R);
  double* out = w + kApWsRt;
  for (int m = 0; m < 9; ++m) out[m] = R[m];
  for (int i = 0; i < 3; ++i) out[9 + i] = pc0[i] - (R[3 * i] * pw0[0] + R[3 * i + 1] * pw0[1] + R[3 * i + 2] * pw0[2]);
}

// The barycentric coordinates of X (absolute_pose.cc:297-304).
MI_HD void ap_epnp_alphas(const double c0[3], const double I[9], const double X[3], double al[4]) {
  MI_UNROLL
  for (int j = 0; j < 3; ++j)
    al[1 + j] = I[3 * j] * (X[0] - c0[0]) + I[3 * j + 1] * (X[1] - c0[1]) + I[3 * j + 2] * (X[2] - c0[2]);
  al[0] = 1.0 - al[1] - al[2] - al[3];
}

// EPNPEstimator::Estimate on a set (absolute_pose.cc:183-609): false for no
// model.  Set: count(), first(f) (f at the first member), leader(), sync() and
// sum<K>(out, f(x, y, X, acc)) over its members.  w: kApWsSize doubles that
// every member of the set's team sees.
template <typename Set>
MI_HD bool ap_epnp(const Set& set, double* w, double P[12]) {
  const double count = (double)set.count();
  // ChooseControlPoints
  double c0[3];
  set.template sum<3>(c0, [](double, double, const double X[3], double* acc) {
    acc[0] += X[0];
    acc[1] += X[1];
    acc[2] += X[2];
  });
  MI_UNROLL
  for (int m = 0; m < 3; ++m) c0[m] /= count;
  double S[6];
  set.template sum<6>(S, [&](double, double, const double X[3], double* acc) {
    const double d0 = X[0] - c0[0], d1 = X[1] - c0[1], d2 = X[2] - c0[2];
    acc[0] += d0 * d0;
    acc[1] += d0 * d1;
    acc[2] += d0 * d2;
    acc[3] += d1 * d1;
    acc[4] += d1 * d2;
    acc[5] += d2 * d2;
  });
  set.sync();
  if (set.leader()) {
    MI_UNROLL
    for (int m = 0; m < 3; ++m) w[kApWsIn + m] = c0[m];
    MI_UNROLL
    for (int m = 0; m < 6; ++m) w[kApWsIn + 3 + m] = S[m];
    ap_epnp_control_points(w, count);
  }
  set.sync();
  if (w[kApWsOk] == 0.0) return false;
  double I[9];
  MI_UNROLL
  for (int m = 0; m < 9; ++m) I[m] = w[kApWsCCinv + m];
  // M'M
  {
    double T[40];
    set.template sum<40>(T, [&](double x, double y, const double X[3], double* acc) {
      double al[4];
      ap_epnp_alphas(c0, I, X, al);
      const double rr = x * x + y * y;
      int e = 0;
      MI_UNROLL
      for (int j = 0; j < 4; ++j) {
        MI_UNROLL
        for (int k = j; k < 4; ++k) {
          const double aa = al[j] * al[k];
          acc[4 * e] += aa;
          acc[4 * e + 1] += aa * x;
          acc[4 * e + 2] += aa * y;
          acc[4 * e + 3] += aa * rr;
          ++e;
        }
      }
    });
    set.sync();
    if (set.leader()) {
      MI_UNROLL
      for (int m = 0; m < 40; ++m) w[kApWsIn + m] = T[m];
      ap_epnp_betas(w);
    }
    set.sync();
  }
  // ComputeRT for the three betas; the smallest sum of sqrt(residual) wins
  double best_err = 0.0;
  MI_AP_NOUNROLL
  for (int which = 0; which < 3; ++which) {
    // ComputeCcs
    double ccs[4][3];
    MI_UNROLL
    for (int j = 0; j < 4; ++j) {
      MI_UNROLL
      for (int k = 0; k < 3; ++k) {
        double s = 0.0;
        MI_UNROLL
        for (int i = 0; i < 4; ++i) s += w[kApWsBetas + 4 * which + i] * w[kApWsUt + 12 * i + 3 * j + k];
        ccs[j][k] = s;
      }
    }
    // SolveForSign on pcs_[0], the first member
    {
      const double z = set.first([&](double, double, const double X[3]) {
        double al[4];
        ap_epnp_alphas(c0, I, X, al);
        return al[0] * ccs[0][2] + al[1] * ccs[1][2] + al[2] * ccs[2][2] + al[3] * ccs[3][2];
      });
      if (z < 0.0) {
        MI_UNROLL
        for (int j = 0; j < 4; ++j) {
          MI_UNROLL
          for (int k = 0; k < 3; ++k) ccs[j][k] = -ccs[j][k];
        }
      }
    }
    // EstimateRT
    double pc0[3];
    set.template sum<3>(pc0, [&](double, double, const double X[3], double* acc) {
      double al[4];
      ap_epnp_alphas(c0, I, X, al);
      MI_UNROLL
      for (int k = 0; k < 3; ++k) acc[k] += al[0] * ccs[0][k] + al[1] * ccs[1][k] + al[2] * ccs[2][k] + al[3] * ccs[3][k];
    });
    MI_UNROLL
    for (int m = 0; m < 3; ++m) pc0[m] /= count;
    double abt[9];
    set.template sum<9>(abt, [&](double, double, const double X[3], double* acc) {
      double al[4];
      ap_epnp_alphas(c0, I, X, al);
      MI_UNROLL
      for (int j = 0; j < 3; ++j) {
        const double pc = al[0] * ccs[0][j] + al[1] * ccs[1][j] + al[2] * ccs[2][j] + al[3] * ccs[3][j];
        acc[3 * j] += (pc - pc0[j]) * (X[0] - c0[0]);
        acc[3 * j + 1] += (pc - pc0[j]) * (X[1] - c0[1]);
        acc[3 * j + 2] += (pc - pc0[j]) * (X[2] - c0[2]);
      }
    });
    set.sync();
    if (set.leader()) {
      MI_UNROLL
      for (int m = 0; m < 9; ++m) w[kApWsIn + m] = abt[m];
      MI_UNROLL
      for (int m = 0; m < 3; ++m) {
        w[kApWsIn + 9 + m] = pc0[m];
        w[kApWsIn + 12 + m] = c0[m];
      }
      ap_epnp_rt(w);
    }
    set.sync();
    double Q[12];
    MI_UNROLL
    for (int i = 0; i < 3; ++i) {
      MI_UNROLL
      for (int j = 0; j < 3; ++j) Q[4 * i + j] = w[kApWsRt + 3 * i + j];
      Q[4 * i + 3] = w[kApWsRt + 9 + i];
    }
    // ComputeTotalReprojectionError
    double err[1];
    set.template sum<1>(err, [&](double x, double y, const double X[3], double* acc) {
      acc[0] += sqrt(ap_squared_error(x, y, X, Q));
    });
    if (which == 0 || err[0] < best_err) {
      best_err = err[0];
      MI_UNROLL
      for (int m = 0; m < 12; ++m) P[m] = Q[m];
    }
  }
  return true;
}

// ---- the host's sets ----
// The members of a problem whose residual under the model `prev` is within
// max_residual, in order; prev == nullptr: every correspondence.
template <typename Rec>
struct ApHostSet {
  Rec rec;
  int64_t n;
  const double* prev;
  double max_residual;
  bool in(int64_t i) const { return !prev || ap_residual(rec, i, prev) <= max_residual; }
  bool leader() const { return true; }
  void sync() const {}
  int64_t count() const {
    int64_t c = 0;
    for (int64_t i = 0; i < n; ++i) c += in(i) ? 1 : 0;
    return c;
  }
  template <typename F>
  double first(F f) const {
    for (int64_t i = 0; i < n; ++i)
      if (in(i)) {
        const double X[3] = {rec.at(i, kApW), rec.at(i, kApW + 1), rec.at(i, kApW + 2)};
        return f(rec.at(i, kApX), rec.at(i, kApY), X);
      }
    return 0.0;
  }
  template <int K, typename F>
  void sum(double (&out)[K], F f) const {
    for (int k = 0; k < K; ++k) out[k] = 0.0;
    for (int64_t i = 0; i < n; ++i) {
      if (!in(i)) continue;
      const double X[3] = {rec.at(i, kApW), rec.at(i, kApW + 1), rec.at(i, kApW + 2)};
      f(rec.at(i, kApX), rec.at(i, kApY), X, out);
    }
  }
};

// Where the reference's abort test stands for trial t (loransac.h:213-217).
MI_HD bool ap_abort(int64_t t, int64_t dyn, int64_t min_num_trials) { return t >= dyn && t >= min_num_trials; }

// The outputs of a problem from its best model (pose.cc:150-155): a NaN in
// qvec or tvec is failure.
MI_HD void ap_finish(ApResult* out, const double best[12], int64_t num_trials, int64_t best_n, bool best_local) {
  out->num_trials = num_trials;
  out->num_inliers = (int32_t)best_n;
  out->best_is_local = best_local ? 1 : 0;
  out->success = best_n >= 3 ? 1 : 0;
  if (!out->success) return;
  MI_UNROLL
  for (int m = 0; m < 12; ++m) out->P[m] = best[m];
  ap_rotation_to_quaternion(best, out->qvec);
  out->tvec[0] = best[3];
  out->tvec[1] = best[7];
  out->tvec[2] = best[11];
  bool nan = false;
  MI_UNROLL
  for (int m = 0; m < 4; ++m) nan = nan || out->qvec[m] != out->qvec[m];
  MI_UNROLL
  for (int m = 0; m < 3; ++m) nan = nan || out->tvec[m] != out->tvec[m];
  if (nan) out->success = 0;
}

// LORANSAC<P3PEstimator, EPNPEstimator, InlierSupportMeasurer,
// RandomSampler>::Estimate (loransac.h:88-249) on one problem of n records,
// with the sampler above.  mask (n bytes) is written on success only.
//
// The residual-buffer swaps of loransac.h:186-204: EPnP returns at most one
// model.  If it is accepted, the first swap parks its residuals in
// best_local_residuals; the recursion continues only if the inlier count grew,
// and the second swap then brings them back.  If it is not accepted its
// residuals stay in `residuals` and the loop ends.  So every recursion takes
// its inlier set from the model evaluated last; the set recomputes those
// residuals (same bits: every build of this header is made with
// -ffp-contract=off, the kernel's object and the host programs alike).
template <typename Rec>
inline void ap_loransac(const ApOptions& o, int64_t min_num_trials, uint64_t seed, const Rec& rec, int64_t n,
                        ApResult* out, uint8_t* mask) {
  out->success = 0;
  out->num_trials = 0;
  out->num_inliers = 0;
  out->best_is_local = 0;
  if (n < 3) return;
  double w[kApWsSize];
  const int64_t max_trials = o.max_num_trials;  // RandomSampler::MaxNumSamples is size_t's maximum
  int64_t dyn = max_trials, best_n = 0, num_trials = 0;
  double best_sum = DBL_MAX, best[12];
  for (int m = 0; m < 12; ++m) best[m] = 0.0;
  bool best_local = false, abort = false;
  for (num_trials = 0; num_trials < max_trials; ++num_trials) {
    if (abort) {
      num_trials += 1;
      break;
    }
    int64_t idx[3];
    ap_sample(seed, num_trials, n, idx);
    ApP3P s;
    ap_p3p_roots(rec, idx[0], idx[1], idx[2], &s);
    for (int k = 0; k < s.count; ++k) {
      double M[12], sum;
      int64_t ni;
      ap_p3p_model(s, s.x[k], M);
      ap_support(rec, n, M, o.max_residual, &ni, &sum);
      if (ap_better(ni, sum, best_n, best_sum)) {
        best_n = ni;
        best_sum = sum;
        best_local = false;
        for (int m = 0; m < 12; ++m) best[m] = M[m];
        if (ni > 3 && ni >= 4) {
          double prev_model[12];
          for (int m = 0; m < 12; ++m) prev_model[m] = M[m];
          for (int local = 0; local < kApMaxLocalTrials; ++local) {
            const int64_t prev = best_n;
            double L[12], lsum;
            int64_t ln;
            const ApHostSet<Rec> set{rec, n, prev_model, o.max_residual};
            if (ap_epnp(set, w, L)) {
              ap_support(rec, n, L, o.max_residual, &ln, &lsum);
              if (ap_better(ln, lsum, best_n, best_sum)) {
                best_n = ln;
                best_sum = lsum;
                best_local = true;
                for (int m = 0; m < 12; ++m) best[m] = L[m];
              }
              for (int m = 0; m < 12; ++m) prev_model[m] = L[m];
            }
            if (best_n <= prev) break;
          }
        }
        dyn = ap_compute_num_trials(best_n, n, o.confidence, o.dyn_num_trials_multiplier);
      }
      if (ap_abort(num_trials, dyn, min_num_trials)) {
        abort = true;
        break;
      }
    }
  }
  ap_finish(out, best, num_trials, best_n, best_local);
  if (!(best_n >= 3)) return;
  if (mask)
    for (int64_t k = 0; k < n; ++k) mask[k] = ap_residual(rec, k, best) <= o.max_residual ? 1 : 0;
}

// Camera::FocalLengthIdxs: the models with fx, fy and those with one f.
MI_HD bool ap_two_focals(int model) {
  return model == kPinhole || model == kOpenCV || model == kOpenCVFisheye || model == kFOV;
}

// EstimateAbsolutePoseKernel's preparation (pose.cc:56-72): the camera with
// its focal parameters scaled; returns (max_error / MeanFocalLength)^2.
MI_HD double ap_scaled_camera(int model, const double prm_in[8], double factor, double max_error, double prm[8]) {
  MI_UNROLL
  for (int m = 0; m < 8; ++m) prm[m] = prm_in[m];
  prm[0] *= factor;
  double mean = prm[0];
  if (ap_two_focals(model)) {
    prm[1] *= factor;
    mean = (prm[0] + prm[1]) / 2.0;
  }
  const double e = max_error / mean;
  return e * e;
}

}  // namespace miba
