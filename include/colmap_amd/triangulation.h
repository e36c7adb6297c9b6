// triangulation.h — the reference's triangulation (src/base/triangulation.h,
// src/estimators/triangulation.h) on the MI355X.
//
// Header-only facade, plain array types like the other facades.
//   EstimateTriangulation(options, point_data, pose_data, &inlier_mask, &xyz)
//       the reference's signature and return value, one track on the device;
//   EstimateTriangulations
//       many tracks in one launch (mi_ba_estimate_triangulation_batch: one
//       wavefront per track, the whole LO-RANSAC on the device);
//   TriangulatePoints, CalculateTriangulationAngles
//       the two-view batch on the device (mi_ba_triangulate_points);
//   TriangulatePoint, TriangulateMultiViewPoint, CalculateTriangulationAngle
//       single items: the host build of the kernel's own math
//       (csrc/triangulation_block.h); they never launch the device.
// Where the reference CHECKs (options, sizes, fewer than two observations),
// this throws std::invalid_argument; device errors throw std::runtime_error.
//
// Difference to the reference: PoseData::camera may be shared by pointer
// between observations and tracks; cameras are told apart by address.
#pragma once

#include <array>
#include <cstdint>
#include <limits>
#include <map>
#include <stdexcept>
#include <string>
#include <vector>

#include "../../semantic-bundle-adjustment-colmap_amd/csrc/triangulation_block.h"
#include "../mi_ba.h"
#include "reconstruction.h"

namespace colmap_amd {

using Matrix3x4d = std::array<double, 12>;  // row-major

struct RANSACOptions {
  double max_error = 0.0;
  double min_inlier_ratio = 0.1;
  double confidence = 0.99;
  double dyn_num_trials_multiplier = 3.0;
  size_t min_num_trials = 0;
  size_t max_num_trials = std::numeric_limits<size_t>::max();

  void Check() const {
    if (!(max_error > 0)) throw std::invalid_argument("max_error must be > 0");
    if (!(min_inlier_ratio >= 0 && min_inlier_ratio <= 1)) throw std::invalid_argument("min_inlier_ratio not in [0, 1]");
    if (!(confidence >= 0 && confidence <= 1)) throw std::invalid_argument("confidence not in [0, 1]");
    if (min_num_trials > max_num_trials) throw std::invalid_argument("min_num_trials > max_num_trials");
  }
};

class TriangulationEstimator {
 public:
  enum class ResidualType { ANGULAR_ERROR, REPROJECTION_ERROR };
  struct PointData {
    PointData() {}
    PointData(const std::array<double, 2>& point_, const std::array<double, 2>& point_N_)
        : point(point_), point_normalized(point_N_) {}
    std::array<double, 2> point{{0, 0}};             // pixels; REPROJECTION_ERROR only
    std::array<double, 2> point_normalized{{0, 0}};  // must always be set
  };
  struct PoseData {
    PoseData() {}
    PoseData(const Matrix3x4d& proj_matrix_, const std::array<double, 3>& pose_, const Camera* camera_)
        : proj_matrix(proj_matrix_), proj_center(pose_), camera(camera_) {}
    Matrix3x4d proj_matrix{};
    std::array<double, 3> proj_center{{0, 0, 0}};
    const Camera* camera = nullptr;
  };
  static const int kMinNumSamples = 2;
};

struct EstimateTriangulationOptions {
  double min_tri_angle = 0.0;
  TriangulationEstimator::ResidualType residual_type = TriangulationEstimator::ResidualType::ANGULAR_ERROR;
  RANSACOptions ransac_options;
  int device = 0;  // HIP device ordinal (build addition)

  void Check() const {
    if (!(min_tri_angle >= 0.0)) throw std::invalid_argument("min_tri_angle must be >= 0");
    ransac_options.Check();
  }
};

// One track of EstimateTriangulations: the arguments of EstimateTriangulation.
// min_num_trials < 0: the options' value.
struct TriangulationProblem {
  const std::vector<TriangulationEstimator::PointData>* point_data = nullptr;
  const std::vector<TriangulationEstimator::PoseData>* pose_data = nullptr;
  std::vector<char>* inlier_mask = nullptr;
  std::array<double, 3>* xyz = nullptr;
  int64_t min_num_trials = -1;
};

// Estimates every track in one launch; returns per track what
// EstimateTriangulation returns.  A failed track leaves its inlier_mask and
// xyz untouched, as the reference does.  num_trials (nullable) receives the
// report's trial counts.
inline std::vector<bool> EstimateTriangulations(const EstimateTriangulationOptions& options,
                                                const std::vector<TriangulationProblem>& problems,
                                                std::vector<int64_t>* num_trials = nullptr) {
  options.Check();
  const int n = (int)problems.size();
  std::vector<int64_t> off(n + 1, 0), min_trials(n);
  for (int k = 0; k < n; ++k) {
    const TriangulationProblem& p = problems[k];
    if (!p.point_data || !p.pose_data || !p.inlier_mask || !p.xyz)
      throw std::invalid_argument("EstimateTriangulation: null argument");
    if (p.point_data->size() < 2) throw std::invalid_argument("point_data.size() < 2");
    if (p.point_data->size() != p.pose_data->size()) throw std::invalid_argument("point_data.size() != pose_data.size()");
    off[k + 1] = off[k] + (int64_t)p.point_data->size();
    min_trials[k] = p.min_num_trials < 0 ? (int64_t)options.ransac_options.min_num_trials : p.min_num_trials;
  }
  std::vector<bool> ok(n, false);
  if (num_trials) num_trials->assign(n, 0);
  if (n == 0) return ok;
  const size_t N = (size_t)off[n];
  const bool reproj = options.residual_type == TriangulationEstimator::ResidualType::REPROJECTION_ERROR;
  std::vector<int32_t> view(N), view_cam(N), models;
  std::vector<double> pts(2 * N), ptn(2 * N), proj(12 * N), cen(3 * N), prm;
  std::vector<int64_t> prm_off(1, 0);
  std::map<const Camera*, int> cam_of;
  const Camera pinhole{};  // stands in for a null camera of an angular track
  for (int k = 0; k < n; ++k) {
    const TriangulationProblem& p = problems[k];
    for (size_t i = 0; i < p.point_data->size(); ++i) {
      const size_t o = (size_t)off[k] + i;
      const auto& x = (*p.point_data)[i];
      const auto& y = (*p.pose_data)[i];
      if (reproj && !y.camera) throw std::invalid_argument("REPROJECTION_ERROR needs PoseData::camera");
      const Camera* cam = y.camera ? y.camera : &pinhole;
      auto it = cam_of.find(cam);
      if (it == cam_of.end()) {
        it = cam_of.emplace(cam, (int)models.size()).first;
        models.push_back(y.camera ? cam->model_id : MI_BA_SIMPLE_PINHOLE);
        if (y.camera) prm.insert(prm.end(), cam->params.begin(), cam->params.end());
        else prm.insert(prm.end(), {1.0, 0.0, 0.0});
        prm_off.push_back((int64_t)prm.size());
      }
      view[o] = (int32_t)o;
      view_cam[o] = it->second;
      for (int m = 0; m < 2; ++m) {
        pts[2 * o + m] = x.point[m];
        ptn[2 * o + m] = x.point_normalized[m];
      }
      for (int m = 0; m < 12; ++m) proj[12 * o + m] = y.proj_matrix[m];
      for (int m = 0; m < 3; ++m) cen[3 * o + m] = y.proj_center[m];
    }
  }
  mi_ba_triangulation_options o;
  mi_ba_default_triangulation_options(&o);
  o.min_tri_angle = options.min_tri_angle;
  o.residual_type = reproj ? MI_BA_TRIANGULATION_REPROJECTION_ERROR : MI_BA_TRIANGULATION_ANGULAR_ERROR;
  o.max_error = options.ransac_options.max_error;
  o.min_inlier_ratio = options.ransac_options.min_inlier_ratio;
  o.confidence = options.ransac_options.confidence;
  o.dyn_num_trials_multiplier = options.ransac_options.dyn_num_trials_multiplier;
  const size_t big = (size_t)INT64_MAX;
  o.min_num_trials = (int64_t)(options.ransac_options.min_num_trials < big ? options.ransac_options.min_num_trials : big);
  o.max_num_trials = (int64_t)(options.ransac_options.max_num_trials < big ? options.ransac_options.max_num_trials : big);
  o.device = options.device;
  mi_ba_triangulation_batch b{};
  b.num_problems = n;
  b.obs_offsets = off.data();
  b.view_index = view.data();
  b.points = pts.data();
  b.points_normalized = ptn.data();
  b.num_views = (int32_t)N;
  b.proj_matrices = proj.data();
  b.proj_centers = cen.data();
  b.camera_index = view_cam.data();
  b.num_cameras = (int32_t)models.size();
  b.camera_model_ids = models.data();
  b.camera_param_offsets = prm_off.data();
  b.camera_params = prm.data();
  b.min_num_trials = min_trials.data();
  std::vector<double> xyz(3 * (size_t)n);
  std::vector<uint8_t> mask(N);
  std::vector<int32_t> success(n);
  std::vector<int64_t> trials(n);
  const mi_ba_status st = mi_ba_estimate_triangulation_batch(&o, &b, xyz.data(), mask.data(), success.data(),
                                                             trials.data(), nullptr, nullptr);
  if (st == MI_BA_ERR_INVALID_ARGUMENT) throw std::invalid_argument("EstimateTriangulation: invalid argument");
  if (st != MI_BA_OK) throw std::runtime_error(std::string("EstimateTriangulation: ") + mi_ba_status_string(st));
  for (int k = 0; k < n; ++k) {
    if (num_trials) (*num_trials)[k] = trials[k];
    if (!success[k]) continue;
    ok[k] = true;
    const TriangulationProblem& p = problems[k];
    p.inlier_mask->assign(mask.begin() + off[k], mask.begin() + off[k + 1]);
    for (int m = 0; m < 3; ++m) (*p.xyz)[m] = xyz[3 * (size_t)k + m];
  }
  return ok;
}

// EstimateTriangulation (src/estimators/triangulation.h:143-147).
inline bool EstimateTriangulation(const EstimateTriangulationOptions& options,
                                  const std::vector<TriangulationEstimator::PointData>& point_data,
                                  const std::vector<TriangulationEstimator::PoseData>& pose_data,
                                  std::vector<char>* inlier_mask, std::array<double, 3>* xyz) {
  TriangulationProblem p;
  p.point_data = &point_data;
  p.pose_data = &pose_data;
  p.inlier_mask = inlier_mask;
  p.xyz = xyz;
  return EstimateTriangulations(options, {p})[0];
}

// ---- src/base/triangulation.h ----

inline std::array<double, 3> TriangulatePoint(const Matrix3x4d& proj_matrix1, const Matrix3x4d& proj_matrix2,
                                              const std::array<double, 2>& point1,
                                              const std::array<double, 2>& point2) {
  std::array<double, 3> X;
  miba::tri_triangulate_point(proj_matrix1.data(), proj_matrix2.data(), point1[0], point1[1], point2[0], point2[1],
                              X.data());
  return X;
}

inline std::array<double, 3> TriangulateMultiViewPoint(const std::vector<Matrix3x4d>& proj_matrices,
                                                       const std::vector<std::array<double, 2>>& points) {
  if (proj_matrices.size() != points.size()) throw std::invalid_argument("proj_matrices.size() != points.size()");
  double S[10] = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0};
  for (size_t i = 0; i < points.size(); ++i) {
    double ray[3];
    miba::tri_unit_ray(points[i][0], points[i][1], ray);
    miba::tri_multiview_accumulate(proj_matrices[i].data(), ray, S);
  }
  std::array<double, 3> X;
  miba::tri_multiview_solve(S, X.data());
  return X;
}

inline double CalculateTriangulationAngle(const std::array<double, 3>& proj_center1,
                                          const std::array<double, 3>& proj_center2,
                                          const std::array<double, 3>& point3D) {
  return miba::tri_angle(proj_center1.data(), proj_center2.data(), point3D.data());
}

inline std::vector<std::array<double, 3>> TriangulatePoints(const Matrix3x4d& proj_matrix1,
                                                            const Matrix3x4d& proj_matrix2,
                                                            const std::vector<std::array<double, 2>>& points1,
                                                            const std::vector<std::array<double, 2>>& points2,
                                                            int device = 0) {
  if (points1.size() != points2.size()) throw std::invalid_argument("points1.size() != points2.size()");
  std::vector<std::array<double, 3>> points3D(points1.size());
  const mi_ba_status st = mi_ba_triangulate_points(
      proj_matrix1.data(), proj_matrix2.data(), (int64_t)points1.size(), points1.empty() ? nullptr : points1[0].data(),
      points2.empty() ? nullptr : points2[0].data(), nullptr, nullptr, device,
      points3D.empty() ? nullptr : points3D[0].data(), nullptr);
  if (st != MI_BA_OK) throw std::runtime_error(std::string("TriangulatePoints: ") + mi_ba_status_string(st));
  return points3D;
}

inline std::vector<double> CalculateTriangulationAngles(const std::array<double, 3>& proj_center1,
                                                        const std::array<double, 3>& proj_center2,
                                                        const std::vector<std::array<double, 3>>& points3D,
                                                        int device = 0) {
  std::vector<double> angles(points3D.size());
  std::vector<std::array<double, 3>> xyz(points3D);
  const mi_ba_status st = mi_ba_triangulate_points(nullptr, nullptr, (int64_t)xyz.size(), nullptr, nullptr,
                                                   proj_center1.data(), proj_center2.data(), device,
                                                   xyz.empty() ? nullptr : xyz[0].data(), angles.data());
  if (st != MI_BA_OK) throw std::runtime_error(std::string("CalculateTriangulationAngles: ") + mi_ba_status_string(st));
  return angles;
}

}  // namespace colmap_amd
