// pose_refinement_test.cc — RefineAbsolutePose / RefineAbsolutePoses through
// the colmap_amd facade (include/colmap_amd/pose.h) on libmi_ba.so.
//
//   ./pose_refinement_test host   options, Check() and the size checks (no GPU)
//   ./pose_refinement_test gpu    one SIMPLE_RADIAL problem with its
//                                 covariance, alone and inside a batch
#include <cmath>
#include <cstdio>
#include <cstring>
#include <random>
#include <stdexcept>
#include <vector>

#include "colmap_amd/pose.h"

using namespace colmap_amd;

static int g_failures = 0;
#define CHECK_T(cond)                                                        \
  do {                                                                       \
    if (!(cond)) {                                                           \
      std::printf("  FAILED %s:%d: %s\n", __FILE__, __LINE__, #cond);        \
      ++g_failures;                                                          \
    }                                                                        \
  } while (0)

template <typename F>
static bool ThrowsInvalid(F&& f) {
  try {
    f();
  } catch (const std::invalid_argument&) {
    return true;
  }
  return false;
}

struct Problem {
  std::vector<char> inlier_mask;
  std::vector<std::array<double, 2>> points2D;
  std::vector<std::array<double, 3>> points3D;
  std::array<double, 4> qvec{{1, 0, 0, 0}};
  std::array<double, 3> tvec{{0, 0, 0}};
  Camera camera;
};

// n points in front of a SIMPLE_RADIAL camera at (0.1, -0.2, 5), half-pixel
// noise, every tenth correspondence a 40 px outlier masked out; the start is
// off the true pose and focal length.
static Problem Generate(int n, unsigned seed) {
  std::mt19937 prng(seed);
  std::uniform_real_distribution<double> U(-1.0, 1.0);
  std::normal_distribution<double> N(0.0, 0.5);
  Problem p;
  p.camera.model_id = MI_BA_SIMPLE_RADIAL;
  p.camera.params = {1200, 500, 500, 0.02};
  const double t[3] = {0.1, -0.2, 5.0};
  for (int i = 0; i < n; ++i) {
    const std::array<double, 3> X{{1.5 * U(prng), 1.5 * U(prng), U(prng)}};
    const std::array<double, 2> xy = p.camera.WorldToImage({{(X[0] + t[0]) / (X[2] + t[2]), (X[1] + t[1]) / (X[2] + t[2])}});
    const bool outlier = i % 10 == 9;
    p.points2D.push_back({{xy[0] + N(prng) + (outlier ? 40.0 : 0.0), xy[1] + N(prng)}});
    p.points3D.push_back(X);
    p.inlier_mask.push_back(outlier ? 0 : 1);
  }
  p.qvec = {{0.9999, 0.01, -0.005, 0.008}};  // not of unit length: normalised first
  p.tvec = {{0.13, -0.17, 5.05}};
  p.camera.params = {1220, 500, 500, 0.03};
  return p;
}

static void TestHost() {
  std::printf("Options\n");
  AbsolutePoseRefinementOptions o;
  CHECK_T(o.gradient_tolerance == 1.0 && o.max_num_iterations == 100 && o.loss_function_scale == 1.0);
  CHECK_T(o.refine_focal_length && o.refine_extra_params && o.print_summary && o.device == 0);
  o.Check();
  AbsolutePoseRefinementOptions bad = o;
  bad.gradient_tolerance = -1;
  CHECK_T(ThrowsInvalid([&] { bad.Check(); }));
  bad = o;
  bad.max_num_iterations = -1;
  CHECK_T(ThrowsInvalid([&] { bad.Check(); }));
  bad = o;
  bad.loss_function_scale = -1;
  CHECK_T(ThrowsInvalid([&] { bad.Check(); }));
  std::printf("PASS Options\n");

  std::printf("SizeChecks\n");
  Problem p = Generate(20, 1);
  o.print_summary = false;
  {
    Problem q = p;
    q.inlier_mask.pop_back();
    CHECK_T(ThrowsInvalid([&] { RefineAbsolutePose(o, q.inlier_mask, q.points2D, q.points3D, &q.qvec, &q.tvec, &q.camera); }));
  }
  {
    Problem q = p;
    q.points3D.pop_back();
    CHECK_T(ThrowsInvalid([&] { RefineAbsolutePose(o, q.inlier_mask, q.points2D, q.points3D, &q.qvec, &q.tvec, &q.camera); }));
  }
  {
    Problem q = p;
    q.camera.params.pop_back();
    CHECK_T(ThrowsInvalid([&] { RefineAbsolutePose(o, q.inlier_mask, q.points2D, q.points3D, &q.qvec, &q.tvec, &q.camera); }));
  }
  {
    Problem q = p;
    bad = o;
    bad.max_num_iterations = -3;
    CHECK_T(ThrowsInvalid([&] { RefineAbsolutePose(bad, q.inlier_mask, q.points2D, q.points3D, &q.qvec, &q.tvec, &q.camera); }));
    CHECK_T(q.qvec == p.qvec && q.camera.params == p.camera.params);
  }
  std::printf("PASS SizeChecks\n");
}

static void TestGpu() {
  std::printf("RefineAbsolutePose\n");
  AbsolutePoseRefinementOptions o;
  o.print_summary = false;
  const Problem start = Generate(200, 3);
  Problem a = start;
  std::array<double, 36> cov_a;
  cov_a.fill(-1.0);
  const bool ok = RefineAbsolutePose(o, a.inlier_mask, a.points2D, a.points3D, &a.qvec, &a.tvec, &a.camera, &cov_a);
  CHECK_T(ok);
  const double nq = std::sqrt(a.qvec[0] * a.qvec[0] + a.qvec[1] * a.qvec[1] + a.qvec[2] * a.qvec[2] + a.qvec[3] * a.qvec[3]);
  CHECK_T(std::fabs(nq - 1.0) < 1e-12);
  // back at the generating pose and intrinsics within the noise
  CHECK_T(std::fabs(a.tvec[0] - 0.1) < 0.02 && std::fabs(a.tvec[1] + 0.2) < 0.02 && std::fabs(a.tvec[2] - 5.0) < 0.1);
  CHECK_T(std::fabs(a.qvec[1]) < 5e-3 && std::fabs(a.qvec[2]) < 5e-3 && std::fabs(a.qvec[3]) < 5e-3);
  CHECK_T(std::fabs(a.camera.params[0] - 1200) < 25 && std::fabs(a.camera.params[3] - 0.02) < 0.02);
  CHECK_T(a.camera.params[1] == 500 && a.camera.params[2] == 500);  // principal point fixed
  for (int i = 0; i < 6; ++i) {
    CHECK_T(cov_a[7 * i] > 0);
    for (int j = 0; j < 6; ++j) CHECK_T(std::fabs(cov_a[6 * i + j] - cov_a[6 * j + i]) <= 1e-12 * std::fabs(cov_a[7 * i]) + 1e-300);
  }
  std::printf("PASS RefineAbsolutePose\n");

  std::printf("RefineAbsolutePoses\n");
  Problem b0 = Generate(37, 4), b1 = start, b2 = Generate(64, 5);
  std::array<double, 36> cov_b;
  cov_b.fill(-1.0);
  std::vector<AbsolutePoseProblem> batch(3);
  Problem* ps[3] = {&b0, &b1, &b2};
  for (int k = 0; k < 3; ++k) {
    batch[k].inlier_mask = &ps[k]->inlier_mask;
    batch[k].points2D = &ps[k]->points2D;
    batch[k].points3D = &ps[k]->points3D;
    batch[k].qvec = &ps[k]->qvec;
    batch[k].tvec = &ps[k]->tvec;
    batch[k].camera = &ps[k]->camera;
  }
  batch[1].rot_tvec_covariance = &cov_b;
  std::vector<SolverSummary> sums;
  const std::vector<bool> usable = RefineAbsolutePoses(o, batch, &sums);
  CHECK_T(usable.size() == 3 && usable[0] && usable[1] && usable[2]);
  CHECK_T(sums.size() == 3 && sums[1].num_residuals_reduced == 2 * 180 && sums[1].num_effective_parameters_reduced == 8);
  CHECK_T(sums[1].termination_type == SolverSummary::CONVERGENCE && sums[1].final_cost < sums[1].initial_cost);
  // the same problem alone and inside the batch: the same bits
  CHECK_T(b1.qvec == a.qvec && b1.tvec == a.tvec && b1.camera.params == a.camera.params && cov_b == cov_a);
  std::printf("PASS RefineAbsolutePoses\n");
}

int main(int argc, char** argv) {
  const bool gpu = argc > 1 && std::strcmp(argv[1], "gpu") == 0;
  if (gpu)
    TestGpu();
  else
    TestHost();
  std::printf("%d failure(s)\n", g_failures);
  return g_failures == 0 ? 0 : 1;
}
