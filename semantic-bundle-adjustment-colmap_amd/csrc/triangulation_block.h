// triangulation_block.h — host/device math of the robust triangulation
// (EstimateTriangulation, src/estimators/triangulation.{h,cc}): the two-view
// and multi-view solves and the triangulation angle of src/base/triangulation.cc,
// the depth test and the residuals of src/base/projection.cc,
// TriangulationEstimator::Estimate / Residuals, RANSAC's ComputeNumTrials
// (src/optim/ransac.h:159-180) and, for the host, the whole LO-RANSAC of
// src/optim/loransac.h:88-249 as one sequential function.  Included by
// triangulation.hip and, compiled for the host, by
// tests/cpp/triangulation_block_test.cc and include/colmap_amd/triangulation.h.
//
// The reference's JacobiSVD and SelfAdjointEigenSolver are not restated: the
// two-view null vector comes from a one-sided (Hestenes) Jacobi on the 4 x 4
// A itself (A'A is never formed), the multi-view one from a cyclic Jacobi on
// the symmetric 4 x 4.  acos is not clamped anywhere, as in the reference: an
// operand that rounding pushes past 1 gives NaN, and every comparison with
// NaN is false (the observation is no inlier, the angle is not sufficient).
#pragma once

#include <cfloat>
#include <cstdint>

#include "ba_math.h"

#if defined(__HIPCC__)
#define MI_TRI_NOUNROLL _Pragma("unroll 1")
#else
#define MI_TRI_NOUNROLL
#endif

namespace miba {

// One observation of a track: 24 doubles.
enum {
  kTriP = 0,        // 3 x 4 projection matrix, row-major
  kTriCenter = 12,  // projection centre
  kTriPn = 15,      // point_normalized
  kTriRay = 17,     // (point_normalized, 1) / |.|
  kTriPixel = 20,   // point, in pixels (reprojection residual only)
  kTriCam = 22,     // camera index
  kTriFlag = 23,    // scratch of the local optimisation: 1 = in the inlier set
  kTriRecord = 24
};
enum { kTriAngular = 0, kTriReprojection = 1 };  // TriangulationEstimator::ResidualType
constexpr double kTriPi = 3.14159265358979323846;
constexpr int64_t kTriMaxTrials = INT64_MAX;  // stands for size_t's maximum

// The records of one track, an array of records with a compile-time stride:
// field f of observation i.  The functions below take any type with this
// at(); the kernel has one more, over LDS with a padded stride.
struct TriRecords {
  double* base;
  MI_HD double& at(int64_t i, int f) const { return base[i * kTriRecord + f]; }
};

struct TriCameras {
  const double* params;  // [C][8]
  const int32_t* model;  // [C]
};

// RANSACOptions and EstimateTriangulationOptions; max_num_trials after the
// constructor's cap (tri_constructor_cap).
struct TriOptions {
  double min_tri_angle, max_residual, confidence, dyn_num_trials_multiplier;
  int64_t max_num_trials;
  int32_t residual_type;
};

// RANSAC::ComputeNumTrials for kMinNumSamples = 2.  size_t's maximum is
// kTriMaxTrials.  A negative or non-finite product (a negative multiplier)
// converts to a huge size_t on x86-64; so it does here.
MI_HD int64_t tri_compute_num_trials(int64_t num_inliers, int64_t num_samples, double confidence, double multiplier) {
  const double inlier_ratio = (double)num_inliers / (double)num_samples;
  const double nom = 1.0 - confidence;
  if (nom <= 0.0) return kTriMaxTrials;
  const double denom = 1.0 - inlier_ratio * inlier_ratio;
  if (denom <= 0.0) return 1;
  if (denom == 1.0) return kTriMaxTrials;
  const double x = ceil(log(nom) / log(denom) * multiplier);
  if (!(x >= 0.0) || !(x < 9.2e18)) return kTriMaxTrials;
  return (int64_t)x;
}

// The constructor's cap of max_num_trials (ransac.h:146-156).
MI_HD int64_t tri_constructor_cap(int64_t max_num_trials, double min_inlier_ratio, double confidence, double multiplier) {
  const int64_t dyn = tri_compute_num_trials((int64_t)(min_inlier_ratio * 100000.0), 100000, confidence, multiplier);
  return dyn < max_num_trials ? dyn : max_num_trials;
}

// Trial t of CombinationSampler: the pairs (0,1), (0,2), ..., (n-2,n-1) in
// lexicographic order.  LORANSAC caps the trials by C(n, 2), so the sampler
// never wraps and t < C(n, 2) always.
MI_HD void tri_unrank_pair(int64_t t, int64_t n, int64_t* i, int64_t* j) {
  // row i starts at i (2n - i - 1) / 2
  const double b = 2.0 * (double)n - 1.0;
  int64_t r = (int64_t)((b - sqrt(b * b - 8.0 * (double)t)) * 0.5);
  if (r < 0) r = 0;
  if (r > n - 2) r = n - 2;
  while (r + 1 <= n - 2 && (r + 1) * (2 * n - r - 2) / 2 <= t) ++r;
  while (r > 0 && r * (2 * n - r - 1) / 2 > t) --r;
  *i = r;
  *j = r + 1 + (t - r * (2 * n - r - 1) / 2);
}

// x / x[3] of the right singular vector of U's smallest singular value;
// U is overwritten.  One-sided Jacobi: columns p, q are rotated until every
// pair is orthogonal to working precision; the singular values are the column
// norms.  At most kTriSweeps sweeps (a 4 x 4 converges in five or six).
constexpr int kTriSweeps = 30;
MI_HD void tri_null_vector_svd4(double (&U)[4][4], double X[3]) {
  double V[4][4];
  MI_UNROLL
  for (int r = 0; r < 4; ++r) {
    MI_UNROLL
    for (int c = 0; c < 4; ++c) V[r][c] = r == c ? 1.0 : 0.0;
  }
  bool rotated = true;
  MI_TRI_NOUNROLL
  for (int sweep = 0; sweep < kTriSweeps && rotated; ++sweep) {
    rotated = false;
    MI_UNROLL
    for (int p = 0; p < 3; ++p) {
      MI_UNROLL
      for (int q = p + 1; q < 4; ++q) {
        double alpha = 0.0, beta = 0.0, gamma = 0.0;
        MI_UNROLL
        for (int k = 0; k < 4; ++k) {
          alpha += U[k][p] * U[k][p];
          beta += U[k][q] * U[k][q];
          gamma += U[k][p] * U[k][q];
        }
        if (fabs(gamma) > DBL_EPSILON * sqrt(alpha * beta)) {
          rotated = true;
          const double zeta = (beta - alpha) / (2.0 * gamma);
          const double t = (zeta >= 0.0 ? 1.0 : -1.0) / (fabs(zeta) + sqrt(1.0 + zeta * zeta));
          const double c = 1.0 / sqrt(1.0 + t * t), s = c * t;
          MI_UNROLL
          for (int k = 0; k < 4; ++k) {
            const double up = U[k][p], uq = U[k][q], vp = V[k][p], vq = V[k][q];
            U[k][p] = c * up - s * uq;
            U[k][q] = s * up + c * uq;
            V[k][p] = c * vp - s * vq;
            V[k][q] = s * vp + c * vq;
          }
        }
      }
    }
  }
  double best = 0.0, v[4] = {0.0, 0.0, 0.0, 0.0};
  MI_UNROLL
  for (int c = 0; c < 4; ++c) {
    double nc = 0.0;
    MI_UNROLL
    for (int k = 0; k < 4; ++k) nc += U[k][c] * U[k][c];
    if (c == 0 || nc < best) {
      best = nc;
      MI_UNROLL
      for (int k = 0; k < 4; ++k) v[k] = V[k][c];
    }
  }
  X[0] = v[0] / v[3];
  X[1] = v[1] / v[3];
  X[2] = v[2] / v[3];
}

// x / x[3] of the eigenvector of the symmetric A's smallest eigenvalue; A is
// overwritten.  Cyclic Jacobi; an off-diagonal entry is rotated away while it
// is above DBL_EPSILON sqrt|a_pp a_qq|.
MI_HD void tri_null_vector_sym4(double (&A)[4][4], double X[3]) {
  double V[4][4];
  MI_UNROLL
  for (int r = 0; r < 4; ++r) {
    MI_UNROLL
    for (int c = 0; c < 4; ++c) V[r][c] = r == c ? 1.0 : 0.0;
  }
  bool rotated = true;
  MI_TRI_NOUNROLL
  for (int sweep = 0; sweep < kTriSweeps && rotated; ++sweep) {
    rotated = false;
    MI_UNROLL
    for (int p = 0; p < 3; ++p) {
      MI_UNROLL
      for (int q = p + 1; q < 4; ++q) {
        const double apq = A[p][q];
        if (fabs(apq) > DBL_EPSILON * sqrt(fabs(A[p][p] * A[q][q]))) {
          rotated = true;
          const double theta = (A[q][q] - A[p][p]) / (2.0 * apq);
          const double t = (theta >= 0.0 ? 1.0 : -1.0) / (fabs(theta) + sqrt(1.0 + theta * theta));
          const double c = 1.0 / sqrt(1.0 + t * t), s = c * t;
          MI_UNROLL
          for (int k = 0; k < 4; ++k) {
            const double akp = A[k][p], akq = A[k][q];
            A[k][p] = c * akp - s * akq;
            A[k][q] = s * akp + c * akq;
          }
          MI_UNROLL
          for (int k = 0; k < 4; ++k) {
            const double apk = A[p][k], aqk = A[q][k];
            A[p][k] = c * apk - s * aqk;
            A[q][k] = s * apk + c * aqk;
          }
          MI_UNROLL
          for (int k = 0; k < 4; ++k) {
            const double vp = V[k][p], vq = V[k][q];
            V[k][p] = c * vp - s * vq;
            V[k][q] = s * vp + c * vq;
          }
        }
      }
    }
  }
  double best = 0.0, v[4] = {0.0, 0.0, 0.0, 0.0};
  MI_UNROLL
  for (int c = 0; c < 4; ++c) {
    if (c == 0 || A[c][c] < best) {
      best = A[c][c];
      MI_UNROLL
      for (int k = 0; k < 4; ++k) v[k] = V[k][c];
    }
  }
  X[0] = v[0] / v[3];
  X[1] = v[1] / v[3];
  X[2] = v[2] / v[3];
}

// TriangulatePoint (triangulation.cc:39-53).
MI_HD void tri_triangulate_point(const double P1[12], const double P2[12], double x1, double y1, double x2, double y2,
                                 double X[3]) {
  double A[4][4];
  MI_UNROLL
  for (int c = 0; c < 4; ++c) {
    A[0][c] = x1 * P1[8 + c] - P1[c];
    A[1][c] = y1 * P1[8 + c] - P1[4 + c];
    A[2][c] = x2 * P2[8 + c] - P2[c];
    A[3][c] = y2 * P2[8 + c] - P2[4 + c];
  }
  tri_null_vector_svd4(A, X);
}

// One view's term of TriangulateMultiViewPoint (triangulation.cc:79-84) added
// to the upper triangle S (row-major, 10 entries) of A: T = P - p p' P with the
// unit ray p, A += T' T.
MI_HD void tri_multiview_accumulate(const double P[12], const double p[3], double (&S)[10]) {
  double w[4], T[3][4];
  MI_UNROLL
  for (int c = 0; c < 4; ++c) w[c] = p[0] * P[c] + p[1] * P[4 + c] + p[2] * P[8 + c];
  MI_UNROLL
  for (int r = 0; r < 3; ++r) {
    MI_UNROLL
    for (int c = 0; c < 4; ++c) T[r][c] = P[4 * r + c] - p[r] * w[c];
  }
  int e = 0;
  MI_UNROLL
  for (int a = 0; a < 4; ++a) {
    MI_UNROLL
    for (int b = a; b < 4; ++b) S[e++] += T[0][a] * T[0][b] + T[1][a] * T[1][b] + T[2][a] * T[2][b];
  }
}

// The eigenvector step of TriangulateMultiViewPoint on the summed triangle.
MI_HD void tri_multiview_solve(const double (&S)[10], double X[3]) {
  double A[4][4];
  int e = 0;
  MI_UNROLL
  for (int a = 0; a < 4; ++a) {
    MI_UNROLL
    for (int b = a; b < 4; ++b) {
      A[a][b] = S[e];
      A[b][a] = S[e];
      ++e;
    }
  }
  tri_null_vector_sym4(A, X);
}

// CalculateTriangulationAngle (triangulation.cc:122-145).
MI_HD double tri_angle(const double c1[3], const double c2[3], const double X[3]) {
  double b2 = 0.0, r1 = 0.0, r2 = 0.0;
  MI_UNROLL
  for (int m = 0; m < 3; ++m) {
    b2 += (c1[m] - c2[m]) * (c1[m] - c2[m]);
    r1 += (X[m] - c1[m]) * (X[m] - c1[m]);
    r2 += (X[m] - c2[m]) * (X[m] - c2[m]);
  }
  const double denominator = 2.0 * sqrt(r1 * r2);
  if (denominator == 0.0) return 0.0;
  const double angle = fabs(acos((r1 + r2 - b2) / denominator));
  const double other = kTriPi - angle;
  return other < angle ? other : angle;  // std::min(angle, M_PI - angle)
}

// HasPointPositiveDepth (projection.cc:191-195).
MI_HD bool tri_positive_depth(const double P[12], const double X[3]) {
  return P[8] * X[0] + P[9] * X[1] + P[10] * X[2] + P[11] >= DBL_EPSILON;
}

// CalculateNormalizedAngularError, projection-matrix overload
// (projection.cc:177-183), with ray1 already of unit length.
MI_HD double tri_angular_error(const double ray1[3], const double P[12], const double X[3]) {
  double r[3];
  MI_UNROLL
  for (int m = 0; m < 3; ++m) r[m] = P[4 * m] * X[0] + P[4 * m + 1] * X[1] + P[4 * m + 2] * X[2] + P[4 * m + 3];
  const double n2 = r[0] * r[0] + r[1] * r[1] + r[2] * r[2];
  if (n2 > 0.0) {  // Eigen's normalized() leaves a zero vector as it is
    const double n = sqrt(n2);
    r[0] /= n;
    r[1] /= n;
    r[2] /= n;
  }
  return acos(ray1[0] * r[0] + ray1[1] * r[1] + ray1[2] * r[2]);
}

// CalculateSquaredReprojectionError, projection-matrix overload
// (projection.cc:130-149): a point behind the camera gives DBL_MAX, the
// camera-frame point is scaled by the reciprocal of its depth.  (The
// quaternion overload of projection.hip divides instead, so its bits differ
// and the two bodies stay apart.)
MI_HD double tri_squared_reprojection_error(double px, double py, const double P[12], const double X[3], int model,
                                            const double* prm) {
  const double z = P[8] * X[0] + P[9] * X[1] + P[10] * X[2] + P[11];
  if (z < DBL_EPSILON) return DBL_MAX;
  const double x = P[0] * X[0] + P[1] * X[1] + P[2] * X[2] + P[3];
  const double y = P[4] * X[0] + P[5] * X[1] + P[6] * X[2] + P[7];
  const double inv = 1.0 / z;
  double u, v;
  world_to_image_all(model, prm, inv * x, inv * y, &u, &v);
  return (u - px) * (u - px) + (v - py) * (v - py);
}

template <typename Rec>
MI_HD void tri_load(const Rec& rec, int64_t i, int f, int count, double* dst) {
  for (int m = 0; m < count; ++m) dst[m] = rec.at(i, f + m);
}

// TriangulationEstimator::Residuals for one observation (triangulation.cc:111-130).
template <typename Rec>
MI_HD double tri_residual(int residual_type, const Rec& rec, int64_t i, const double X[3],
                          const TriCameras& cams) {
  double P[12];
  MI_UNROLL
  for (int m = 0; m < 12; ++m) P[m] = rec.at(i, kTriP + m);
  if (residual_type == kTriReprojection) {
    const int cam = (int)rec.at(i, kTriCam);
    double prm[8];
    MI_UNROLL
    for (int m = 0; m < 8; ++m) prm[m] = cams.params[8 * (size_t)cam + m];
    return tri_squared_reprojection_error(rec.at(i, kTriPixel), rec.at(i, kTriPixel + 1), P, X, cams.model[cam], prm);
  }
  const double ray[3] = {rec.at(i, kTriRay), rec.at(i, kTriRay + 1), rec.at(i, kTriRay + 2)};
  const double e = tri_angular_error(ray, P, X);
  return e * e;
}

// InlierSupportMeasurer::Evaluate of the model X over the whole track, summed
// in observation order.
template <typename Rec>
MI_HD void tri_support(const TriOptions& o, const Rec& rec, int64_t n, const double X[3],
                       const TriCameras& cams, int64_t* num_inliers, double* residual_sum) {
  int64_t ni = 0;
  double sum = 0.0;
  MI_TRI_NOUNROLL
  for (int64_t i = 0; i < n; ++i) {
    const double r = tri_residual(o.residual_type, rec, i, X, cams);
    if (r <= o.max_residual) {
      ni += 1;
      sum += r;
    }
  }
  *num_inliers = ni;
  *residual_sum = sum;
}

// InlierSupportMeasurer::Compare.
MI_HD bool tri_better(int64_t n1, double s1, int64_t n2, double s2) { return n1 > n2 || (n1 == n2 && s1 < s2); }

// TriangulationEstimator::Estimate on the pair (i, j) (triangulation.cc:61-74).
template <typename Rec>
MI_HD bool tri_estimate_two(const TriOptions& o, const Rec& rec, int64_t i, int64_t j, double X[3]) {
  double P1[12], P2[12];
  MI_UNROLL
  for (int m = 0; m < 12; ++m) {
    P1[m] = rec.at(i, kTriP + m);
    P2[m] = rec.at(j, kTriP + m);
  }
  tri_triangulate_point(P1, P2, rec.at(i, kTriPn), rec.at(i, kTriPn + 1), rec.at(j, kTriPn), rec.at(j, kTriPn + 1), X);
  if (!tri_positive_depth(P1, X) || !tri_positive_depth(P2, X)) return false;
  const double c1[3] = {rec.at(i, kTriCenter), rec.at(i, kTriCenter + 1), rec.at(i, kTriCenter + 2)};
  const double c2[3] = {rec.at(j, kTriCenter), rec.at(j, kTriCenter + 1), rec.at(j, kTriCenter + 2)};
  return tri_angle(c1, c2, X) >= o.min_tri_angle;
}

// (point_normalized, 1) / |.| as Eigen's homogeneous().normalized().
MI_HD void tri_unit_ray(double x, double y, double ray[3]) {
  const double n = sqrt(x * x + y * y + 1.0);
  ray[0] = x / n;
  ray[1] = y / n;
  ray[2] = 1.0 / n;
}

// ---- the host's sequential estimator ----

// TriangulationEstimator::Estimate on the flagged observations, more than two
// of them (triangulation.cc:75-106).
template <typename Rec>
inline bool tri_estimate_flagged(const TriOptions& o, const Rec& rec, int64_t n, double X[3]) {
  double S[10] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
  for (int64_t i = 0; i < n; ++i) {
    if (rec.at(i, kTriFlag) == 0.0) continue;
    double P[12], ray[3];
    tri_load(rec, i, kTriP, 12, P);
    tri_load(rec, i, kTriRay, 3, ray);
    tri_multiview_accumulate(P, ray, S);
  }
  tri_multiview_solve(S, X);
  for (int64_t i = 0; i < n; ++i) {
    if (rec.at(i, kTriFlag) == 0.0) continue;
    double P[12];
    tri_load(rec, i, kTriP, 12, P);
    if (!tri_positive_depth(P, X)) return false;
  }
  for (int64_t i = 0; i < n; ++i) {
    if (rec.at(i, kTriFlag) == 0.0) continue;
    double ci[3];
    tri_load(rec, i, kTriCenter, 3, ci);
    for (int64_t j = 0; j < i; ++j) {
      if (rec.at(j, kTriFlag) == 0.0) continue;
      double cj[3];
      tri_load(rec, j, kTriCenter, 3, cj);
      if (tri_angle(ci, cj, X) >= o.min_tri_angle) return true;
    }
  }
  return false;
}

struct TriResult {
  double xyz[3];
  int64_t num_trials;
  int32_t success, num_inliers, best_is_local, pad;
};

// LORANSAC<TriangulationEstimator, TriangulationEstimator,
// InlierSupportMeasurer, CombinationSampler>::Estimate on one track of n >= 2
// records.  mask (n bytes) is written on success only.
//
// The residual-buffer swaps of loransac.h:186-204: a recursion continues only
// after the local model was accepted with more inliers, and the two swaps then
// leave that local model's residuals in `residuals`; in every other case the
// loop ends and `residuals` is overwritten before it is read again.  So each
// recursion takes its inlier set from the model evaluated last, which is what
// the flags hold here.
template <typename Rec>
inline void tri_loransac(const TriOptions& o, int64_t min_num_trials, const Rec& rec, int64_t n,
                         const TriCameras& cams, TriResult* out, uint8_t* mask) {
  const int64_t pairs = n * (n - 1) / 2;
  const int64_t max_trials = o.max_num_trials < pairs ? o.max_num_trials : pairs;
  int64_t dyn = max_trials, best_n = 0, num_trials = 0;
  double best_sum = DBL_MAX, best[3] = {0.0, 0.0, 0.0};
  bool best_local = false, abort = false;
  for (num_trials = 0; num_trials < max_trials; ++num_trials) {
    if (abort) {
      num_trials += 1;
      break;
    }
    int64_t i, j, ni;
    double X[3], sum;
    tri_unrank_pair(num_trials, n, &i, &j);
    if (!tri_estimate_two(o, rec, i, j, X)) continue;
    tri_support(o, rec, n, X, cams, &ni, &sum);
    if (tri_better(ni, sum, best_n, best_sum)) {
      best_n = ni;
      best_sum = sum;
      best_local = false;
      for (int m = 0; m < 3; ++m) best[m] = X[m];
      if (ni > 2) {
        for (int64_t k = 0; k < n; ++k)
          rec.at(k, kTriFlag) = tri_residual(o.residual_type, rec, k, X, cams) <= o.max_residual ? 1.0 : 0.0;
        for (int local = 0; local < 10; ++local) {
          const int64_t prev = best_n;
          double L[3], lsum = 0.0;
          if (!tri_estimate_flagged(o, rec, n, L)) break;
          int64_t ln = 0;
          for (int64_t k = 0; k < n; ++k) {
            const double r = tri_residual(o.residual_type, rec, k, L, cams);
            const bool in = r <= o.max_residual;
            rec.at(k, kTriFlag) = in ? 1.0 : 0.0;
            if (in) {
              ln += 1;
              lsum += r;
            }
          }
          if (tri_better(ln, lsum, best_n, best_sum)) {
            best_n = ln;
            best_sum = lsum;
            best_local = true;
            for (int m = 0; m < 3; ++m) best[m] = L[m];
          }
          if (best_n <= prev) break;
        }
      }
      dyn = tri_compute_num_trials(best_n, n, o.confidence, o.dyn_num_trials_multiplier);
    }
    if (num_trials >= dyn && num_trials >= min_num_trials) abort = true;
  }
  out->num_trials = num_trials;
  out->num_inliers = (int32_t)best_n;
  out->best_is_local = best_local ? 1 : 0;
  out->success = best_n >= 2 ? 1 : 0;
  if (!out->success) return;
  for (int m = 0; m < 3; ++m) out->xyz[m] = best[m];
  if (mask)
    for (int64_t k = 0; k < n; ++k)
      mask[k] = tri_residual(o.residual_type, rec, k, best, cams) <= o.max_residual ? 1 : 0;
}

// Fills one record from PoseData (P, C, the camera's index) and PointData
// (pixel, point_normalized).
MI_HD void tri_fill_record(double* r, const double* P, const double* C, double px, double py, double nx, double ny,
                           int cam) {
  MI_UNROLL
  for (int m = 0; m < 12; ++m) r[kTriP + m] = P[m];
  MI_UNROLL
  for (int m = 0; m < 3; ++m) r[kTriCenter + m] = C[m];
  r[kTriPn] = nx;
  r[kTriPn + 1] = ny;
  tri_unit_ray(nx, ny, r + kTriRay);
  r[kTriPixel] = px;
  r[kTriPixel + 1] = py;
  r[kTriCam] = (double)cam;
  r[kTriFlag] = 0.0;
}

}  // namespace miba
