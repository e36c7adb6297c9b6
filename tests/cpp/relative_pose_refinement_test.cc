// relative_pose_refinement_test.cc — RefineRelativePose / RefineRelativePoses /
// EssentialMatrixFromPose through the colmap_amd facade
// (include/colmap_amd/pose.h) on libmi_ba.so.
//
//   ./relative_pose_refinement_test host        defaults, Check(), the size check
//                                               and EssentialMatrixFromPose (no GPU)
//   ./relative_pose_refinement_test gpu FILE    the problem of FILE (the text form
//                                               test_relative_pose.py writes) alone
//                                               and inside a batch; its result is
//                                               printed as hex floats after "RESULT"
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <fstream>
#include <stdexcept>
#include <string>
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

struct Problem {
  std::vector<std::array<double, 2>> points1, points2;
  std::array<double, 4> qvec{{1, 0, 0, 0}};
  std::array<double, 3> tvec{{1, 0, 0}};
};

// The scene of the reference's TestRefineEssentialMatrix: points on z = 1, R = I, t = (1, 0, 0).
static Problem Scene() {
  Problem p;
  for (int i = 0; i < 50; ++i) {
    const double X[3][2] = {{i * 0.01, 0.0}, {0.0, i * 0.01}, {i * 0.01, i * 0.01}};
    for (const auto& x : X) {
      p.points1.push_back({{x[0], x[1]}});
      p.points2.push_back({{x[0] + 1.0, x[1]}});
    }
  }
  const double n = std::sqrt(1.02 * 1.02 + 2 * 0.02 * 0.02);
  p.tvec = {{1.02 / n, 0.02 / n, 0.02 / n}};
  return p;
}

static void TestHost() {
  std::printf("Options\n");
  RelativePoseRefinementOptions o;
  CHECK_T(o.max_num_iterations == 50 && o.function_tolerance == 1e-6 && o.gradient_tolerance == 1e-10 &&
          o.parameter_tolerance == 1e-8);
  CHECK_T(o.loss_function_scale == 1.0 && o.device == 0);
  o.Check();
  const Problem p = Scene();
  for (int f = 0; f < 5; ++f) {
    RelativePoseRefinementOptions bad = o;
    if (f == 0) bad.max_num_iterations = -1;
    if (f == 1) bad.function_tolerance = -1;
    if (f == 2) bad.gradient_tolerance = -1;
    if (f == 3) bad.parameter_tolerance = -1;
    if (f == 4) bad.loss_function_scale = -1;
    CHECK_T(Throws<std::invalid_argument>([&] { bad.Check(); }));
    Problem q = p;
    CHECK_T(Throws<std::invalid_argument>([&] { RefineRelativePose(bad, q.points1, q.points2, &q.qvec, &q.tvec); }));
    CHECK_T(q.qvec == p.qvec && q.tvec == p.tvec);
  }
  std::printf("PASS Options\n");

  std::printf("SizeCheck\n");
  {
    Problem q = p;  // CHECK_EQ(points1.size(), points2.size())
    q.points2.pop_back();
    CHECK_T(Throws<std::invalid_argument>([&] { RefineRelativePose(o, q.points1, q.points2, &q.qvec, &q.tvec); }));
    CHECK_T(Throws<std::invalid_argument>([&] { RefineRelativePose(o, q.points1, q.points1, nullptr, &q.tvec); }));
  }
  std::printf("PASS SizeCheck\n");

  std::printf("EssentialMatrixFromPose\n");
  {
    // R = I, t = (0, 0, 2): [t / |t|]x = (0 -1 0; 1 0 0; 0 0 0)
    const std::array<double, 9> I{{1, 0, 0, 0, 1, 0, 0, 0, 1}};
    const std::array<double, 9> E = EssentialMatrixFromPose(I, {{0, 0, 2}});
    const std::array<double, 9> want{{0, -1, 0, 1, 0, 0, 0, 0, 0}};
    CHECK_T(E == want);
    // a quarter turn about z, t = (1, 0, 0): R = (0 -1 0; 1 0 0; 0 0 1), E = [e1]x R = (0 0 0; 0 0 -1; 1 0 0)
    const double h = std::sqrt(0.5);
    const std::array<double, 9> Eq = EssentialMatrixFromPose(std::array<double, 4>{{2 * h, 0, 0, 2 * h}}, {{3, 0, 0}});
    const std::array<double, 9> want_q{{0, 0, 0, 0, 0, -1, 1, 0, 0}};
    for (int m = 0; m < 9; ++m) CHECK_T(std::fabs(Eq[m] - want_q[m]) <= 4e-16);
  }
  std::printf("PASS EssentialMatrixFromPose\n");
}

static Problem Read(const char* path) {
  std::ifstream in(path);
  if (!in) throw std::runtime_error(std::string("cannot read ") + path);
  auto num = [&]() {
    std::string tok;
    in >> tok;
    return std::strtod(tok.c_str(), nullptr);
  };
  Problem p;
  for (int m = 0; m < 4; ++m) p.qvec[m] = num();
  for (int m = 0; m < 3; ++m) p.tvec[m] = num();
  const int n = (int)num();
  for (int i = 0; i < n; ++i) {
    const double x1 = num(), y1 = num(), x2 = num(), y2 = num();
    p.points1.push_back({{x1, y1}});
    p.points2.push_back({{x2, y2}});
  }
  return p;
}

static double Distance(const std::array<double, 9>& a, const std::array<double, 9>& b) {
  double s = 0.0;
  for (int m = 0; m < 9; ++m) s += (a[m] - b[m]) * (a[m] - b[m]);
  return std::sqrt(s);
}

static void TestGpu(const char* file) {
  std::printf("RefineRelativePose\n");
  RelativePoseRefinementOptions o;
  const Problem start = Scene();
  Problem a = start;
  CHECK_T(RefineRelativePose(o, a.points1, a.points2, &a.qvec, &a.tvec));
  // essential_matrix_test.cc:204: the refined E is not farther from the truth than the perturbed one
  const std::array<double, 9> E = EssentialMatrixFromPose(std::array<double, 4>{{1, 0, 0, 0}}, {{1, 0, 0}});
  CHECK_T(Distance(E, EssentialMatrixFromPose(a.qvec, a.tvec)) <= Distance(E, EssentialMatrixFromPose(start.qvec, start.tvec)));
  const double nt = std::sqrt(a.tvec[0] * a.tvec[0] + a.tvec[1] * a.tvec[1] + a.tvec[2] * a.tvec[2]);
  CHECK_T(std::fabs(nt - 1.0) <= 1e-14);
  std::printf("PASS RefineRelativePose\n");

  std::printf("RefineRelativePoses\n");
  Problem f = Read(file), b0 = start, b1 = f, b2 = start;
  const bool ok = RefineRelativePose(o, f.points1, f.points2, &f.qvec, &f.tvec);
  std::vector<RelativePoseProblem> batch(3);
  Problem* ps[3] = {&b0, &b1, &b2};
  for (int k = 0; k < 3; ++k) {
    batch[k].points1 = &ps[k]->points1;
    batch[k].points2 = &ps[k]->points2;
    batch[k].qvec = &ps[k]->qvec;
    batch[k].tvec = &ps[k]->tvec;
  }
  std::vector<SolverSummary> sums;
  const std::vector<bool> usable = RefineRelativePoses(o, batch, &sums);
  CHECK_T(usable.size() == 3 && usable[0] && usable[1] == ok && usable[2]);
  CHECK_T(sums.size() == 3 && sums[1].num_residuals_reduced == (int64_t)f.points1.size() &&
          sums[1].num_effective_parameters_reduced == 5);
  // alone and inside the batch: the same bits
  CHECK_T(b1.qvec == f.qvec && b1.tvec == f.tvec && b0.qvec == a.qvec && b0.tvec == a.tvec && b2.tvec == a.tvec);
  std::printf("PASS RefineRelativePoses\n");
  std::printf("RESULT %d", ok ? 1 : 0);
  for (double v : f.qvec) std::printf(" %a", v);
  for (double v : f.tvec) std::printf(" %a", v);
  for (double v : b1.qvec) std::printf(" %a", v);
  for (double v : b1.tvec) std::printf(" %a", v);
  std::printf("\n");
}

int main(int argc, char** argv) {
  if (argc > 2 && std::strcmp(argv[1], "gpu") == 0)
    TestGpu(argv[2]);
  else
    TestHost();
  std::printf("%d failure(s)\n", g_failures);
  return g_failures == 0 ? 0 : 1;
}
