// triangulation_test.cc — EstimateTriangulation / EstimateTriangulations and
// the functions of base/triangulation.h through the colmap_amd facade
// (include/colmap_amd/triangulation.h) on libmi_ba.so.
//
//   ./triangulation_test host        defaults, Check(), the size checks and the
//                                    known answers of the reference's
//                                    triangulation_test.cc on the single-item
//                                    functions (no GPU)
//   ./triangulation_test gpu FILE    the track of FILE (the text form
//                                    test_triangulation.py writes) alone and
//                                    inside a batch; its result is printed as
//                                    hex floats after "RESULT"
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <fstream>
#include <stdexcept>
#include <string>
#include <vector>

#include "colmap_amd/triangulation.h"

using namespace colmap_amd;

static int g_failures = 0;
#define CHECK_T(cond)                                                        \
  do {                                                                       \
    if (!(cond)) {                                                           \
      std::printf("  FAILED %s:%d: %s\n", __FILE__, __LINE__, #cond);        \
      ++g_failures;                                                          \
    }                                                                        \
  } while (0)

template <typename E, typename F>
static bool Throws(F&& f) {
  try {
    f();
  } catch (const E&) {
    return true;
  } catch (...) {
  }
  return false;
}

// [R(q / |q|) | t], row-major (SimilarityTransform3 with scale 1).
static Matrix3x4d Pose(double w, double x, double y, double z, double tx, double ty, double tz) {
  const double n = std::sqrt(w * w + x * x + y * y + z * z);
  w /= n; x /= n; y /= n; z /= n;
  return {{1 - 2 * (y * y + z * z), 2 * (x * y - w * z), 2 * (x * z + w * y), tx,
           2 * (x * y + w * z), 1 - 2 * (x * x + z * z), 2 * (y * z - w * x), ty,
           2 * (x * z - w * y), 2 * (y * z + w * x), 1 - 2 * (x * x + y * y), tz}};
}

static std::array<double, 2> Project(const Matrix3x4d& P, const std::array<double, 3>& X) {
  double p[3];
  for (int r = 0; r < 3; ++r) p[r] = P[4 * r] * X[0] + P[4 * r + 1] * X[1] + P[4 * r + 2] * X[2] + P[4 * r + 3];
  return {{p[0] / p[2], p[1] / p[2]}};
}

static void TestHost() {
  std::printf("Options\n");
  EstimateTriangulationOptions o;
  CHECK_T(o.min_tri_angle == 0.0 && o.residual_type == TriangulationEstimator::ResidualType::ANGULAR_ERROR);
  CHECK_T(o.ransac_options.max_error == 0.0 && o.ransac_options.min_inlier_ratio == 0.1 &&
          o.ransac_options.confidence == 0.99 && o.ransac_options.dyn_num_trials_multiplier == 3.0 &&
          o.ransac_options.min_num_trials == 0 &&
          o.ransac_options.max_num_trials == std::numeric_limits<size_t>::max());
  CHECK_T(Throws<std::invalid_argument>([&] { o.Check(); }));  // max_error 0
  o.ransac_options.max_error = 1.0;
  o.Check();
  auto bad = o;
  bad.min_tri_angle = -1;
  CHECK_T(Throws<std::invalid_argument>([&] { bad.Check(); }));
  bad = o;
  bad.ransac_options.confidence = 1.5;
  CHECK_T(Throws<std::invalid_argument>([&] { bad.Check(); }));
  bad = o;
  bad.ransac_options.min_num_trials = 5;
  bad.ransac_options.max_num_trials = 4;
  CHECK_T(Throws<std::invalid_argument>([&] { bad.Check(); }));
  // the size checks come before any device is touched
  std::vector<TriangulationEstimator::PointData> one(1);
  std::vector<TriangulationEstimator::PoseData> pose1(1), pose2(2);
  std::vector<char> mask;
  std::array<double, 3> xyz;
  CHECK_T(Throws<std::invalid_argument>([&] { EstimateTriangulation(o, one, pose1, &mask, &xyz); }));
  std::vector<TriangulationEstimator::PointData> three(3);
  CHECK_T(Throws<std::invalid_argument>([&] { EstimateTriangulation(o, three, pose2, &mask, &xyz); }));
  std::printf("  %s\n", g_failures ? "FAIL" : "PASS");

  std::printf("TestTriangulatePoint\n");
  const int before = g_failures;
  const std::array<double, 3> pts[6] = {{{0, 0.1, 0.1}}, {{0, 1, 3}}, {{0, 1, 2}}, {{0.01, 0.2, 3}}, {{-1, 0.1, 1}},
                                        {{0.1, 0.1, 0.2}}};
  const Matrix3x4d P1 = {{1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0}};
  int cells = 0;
  for (double qz = 0; qz < 1; qz += 0.2) {
    for (double tx = 0; tx < 10; tx += 2) {
      const Matrix3x4d P2 = Pose(0.2, 0.3, 0.4, qz, tx, 2, 3);
      for (const auto& X : pts) {
        const auto got = TriangulatePoint(P1, P2, Project(P1, X), Project(P2, X));
        const double d = std::sqrt((got[0] - X[0]) * (got[0] - X[0]) + (got[1] - X[1]) * (got[1] - X[1]) +
                                   (got[2] - X[2]) * (got[2] - X[2]));
        CHECK_T(d < 1e-10);
        // three views of the same point: the multi-view solve finds it too
        const Matrix3x4d P3 = Pose(0.9, -0.1, 0.2, 0.1, -1, 0.5, 2);
        const auto multi = TriangulateMultiViewPoint({P1, P2, P3}, {Project(P1, X), Project(P2, X), Project(P3, X)});
        CHECK_T(std::fabs(multi[0] - X[0]) < 1e-10 && std::fabs(multi[1] - X[1]) < 1e-10 &&
                std::fabs(multi[2] - X[2]) < 1e-10);
        ++cells;
      }
    }
  }
  CHECK_T(cells == 150);
  std::printf("  %s\n", g_failures == before ? "PASS" : "FAIL");

  std::printf("TestCalculateTriangulationAngle\n");
  const int before2 = g_failures;
  // BOOST_CHECK_CLOSE(..., 1e-8): a relative 1e-10
  CHECK_T(std::fabs(CalculateTriangulationAngle({{0, 0, 0}}, {{0, 1, 0}}, {{0, 0, 100}}) / 0.009999666687 - 1) <= 1e-10);
  CHECK_T(std::fabs(CalculateTriangulationAngle({{0, 0, 0}}, {{0, 1, 0}}, {{0, 0, 50}}) / 0.019997333973 - 1) <= 1e-10);
  CHECK_T(CalculateTriangulationAngle({{0, 0, 0}}, {{0, 1, 0}}, {{0, 0, 0}}) == 0.0);  // denominator == 0
  std::printf("  %s\n", g_failures == before2 ? "PASS" : "FAIL");
}

struct Track {
  EstimateTriangulationOptions options;
  std::vector<Camera> cameras;
  std::vector<TriangulationEstimator::PointData> points;
  std::vector<TriangulationEstimator::PoseData> poses;
};

static Track ReadTrack(const char* path) {
  std::ifstream f(path);
  if (!f) throw std::runtime_error(std::string("cannot read ") + path);
  std::vector<double> v;
  std::string tok;
  while (f >> tok) v.push_back(std::strtod(tok.c_str(), nullptr));
  size_t at = 0;
  Track t;
  t.options.residual_type = v[at++] != 0 ? TriangulationEstimator::ResidualType::REPROJECTION_ERROR
                                         : TriangulationEstimator::ResidualType::ANGULAR_ERROR;
  t.options.min_tri_angle = v[at++];
  t.options.ransac_options.max_error = v[at++];
  t.options.ransac_options.confidence = v[at++];
  t.options.ransac_options.min_inlier_ratio = v[at++];
  t.options.ransac_options.max_num_trials = (size_t)v[at++];
  t.options.ransac_options.min_num_trials = (size_t)v[at++];
  const int C = (int)v[at++];
  t.cameras.resize(C);
  for (int c = 0; c < C; ++c) {
    t.cameras[c].model_id = (int)v[at++];
    const int np = (int)v[at++];
    t.cameras[c].params.assign(v.begin() + at, v.begin() + at + np);
    at += np;
  }
  const int n = (int)v[at++];
  t.points.resize(n);
  t.poses.resize(n);
  for (int i = 0; i < n; ++i) {
    t.poses[i].camera = &t.cameras[(int)v[at++]];
    t.points[i].point = {{v[at], v[at + 1]}};
    t.points[i].point_normalized = {{v[at + 2], v[at + 3]}};
    at += 4;
    for (int m = 0; m < 12; ++m) t.poses[i].proj_matrix[m] = v[at++];
    for (int m = 0; m < 3; ++m) t.poses[i].proj_center[m] = v[at++];
  }
  return t;
}

static void TestGpu(const char* path) {
  std::printf("EstimateTriangulation\n");
  Track t = ReadTrack(path);
  std::vector<char> mask;
  std::array<double, 3> xyz{{7, 7, 7}};
  const bool ok = EstimateTriangulation(t.options, t.points, t.poses, &mask, &xyz);
  // inside a batch, between a two-view track of its first two observations and a copy
  std::vector<TriangulationEstimator::PointData> two_x(t.points.begin(), t.points.begin() + 2);
  std::vector<TriangulationEstimator::PoseData> two_y(t.poses.begin(), t.poses.begin() + 2);
  std::vector<char> m0, m1, m2;
  std::array<double, 3> x0{{7, 7, 7}}, x1{{7, 7, 7}}, x2{{7, 7, 7}};
  std::vector<TriangulationProblem> batch(3);
  batch[0] = TriangulationProblem{&two_x, &two_y, &m0, &x0, -1};
  batch[1] = TriangulationProblem{&t.points, &t.poses, &m1, &x1, -1};
  batch[2] = TriangulationProblem{&t.points, &t.poses, &m2, &x2, -1};
  std::vector<int64_t> trials;
  const auto oks = EstimateTriangulations(t.options, batch, &trials);
  CHECK_T(oks[1] == ok && oks[2] == ok && trials[1] == trials[2]);
  CHECK_T(!ok || (mask == m1 && mask == m2 && xyz == x1 && xyz == x2));
  CHECK_T(ok || (mask.empty() && xyz[0] == 7));  // a failed track leaves its outputs untouched
  // the two-view entry on the device and the single-item function on the host agree
  const auto dev = TriangulatePoints(t.poses[0].proj_matrix, t.poses[1].proj_matrix, {t.points[0].point_normalized},
                                     {t.points[1].point_normalized});
  const auto host = TriangulatePoint(t.poses[0].proj_matrix, t.poses[1].proj_matrix, t.points[0].point_normalized,
                                     t.points[1].point_normalized);
  for (int m = 0; m < 3; ++m) CHECK_T(std::fabs(dev[0][m] - host[m]) <= 1e-12 * (1 + std::fabs(host[m])));
  const auto angles = CalculateTriangulationAngles(t.poses[0].proj_center, t.poses[1].proj_center, dev);
  CHECK_T(std::fabs(angles[0] - CalculateTriangulationAngle(t.poses[0].proj_center, t.poses[1].proj_center, dev[0])) <=
          1e-12);
  std::printf("RESULT %d %lld %a %a %a ", ok ? 1 : 0, (long long)trials[1], xyz[0], xyz[1], xyz[2]);
  for (char c : mask) std::printf("%d", c ? 1 : 0);
  std::printf("\n  %s\n", g_failures ? "FAIL" : "PASS");
}

int main(int argc, char** argv) {
  try {
    if (argc >= 2 && !std::strcmp(argv[1], "host")) TestHost();
    else if (argc >= 3 && !std::strcmp(argv[1], "gpu")) TestGpu(argv[2]);
    else {
      std::printf("usage: %s host | gpu FILE\n", argv[0]);
      return 2;
    }
  } catch (const std::exception& e) {
    std::printf("  FAILED: exception: %s\n", e.what());
    ++g_failures;
  }
  std::printf("%d failure(s)\n", g_failures);
  return g_failures ? 1 : 0;
}
