// relative_pose_block_test.cc — the host build of csrc/relative_pose_block.h
// (the arithmetic of relative_pose_kernel), no device and no library.
//
//   ./relative_pose_block_test rows FILE   FILE: q(4) t(3) n, then n lines of
//                                          x1 y1 x2 y2, all hex floats; prints
//                                          "ROW r J0 .. J4" per correspondence
//                                          (hex floats, not loss-corrected)
//   ./relative_pose_block_test chart       SphereManifold<3> on every branch of
//                                          its Householder vector
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <fstream>
#include <string>
#include <vector>

#include "../../semantic-bundle-adjustment-colmap_amd/csrc/relative_pose_block.h"

using namespace miba;

static int g_failures = 0;
#define CHECK_T(cond)                                                        \
  do {                                                                       \
    if (!(cond)) {                                                           \
      std::printf("  FAILED %s:%d: %s\n", __FILE__, __LINE__, #cond);        \
      ++g_failures;                                                          \
    }                                                                        \
  } while (0)

static int Rows(const char* path) {
  std::ifstream in(path);
  if (!in) {
    std::printf("cannot read %s\n", path);
    return 1;
  }
  auto num = [&]() {
    std::string tok;
    in >> tok;
    return std::strtod(tok.c_str(), nullptr);
  };
  double q[4], t[3];
  for (double& v : q) v = num();
  for (double& v : t) v = num();
  const int n = (int)num();
  RelPoseFrame f;
  relpose_frame(q, t, true, &f);
  for (int i = 0; i < n; ++i) {
    const double x1 = num(), y1 = num(), x2 = num(), y2 = num();
    double J[5];
    const double r = relpose_residual_jacobian(f, x1, y1, x2, y2, J);
    CHECK_T(r == relpose_residual(f.E, x1, y1, x2, y2));
    std::printf("ROW %a %a %a %a %a %a\n", r, J[0], J[1], J[2], J[3], J[4]);
  }
  return 0;
}

static double Norm(const double x[3]) { return std::sqrt(x[0] * x[0] + x[1] * x[1] + x[2] * x[2]); }

static void Chart(const char* name, const double x[3], bool expect_sigma_branch, double expect_beta) {
  std::printf("%s\n", name);
  double v[3], beta;
  sphere_householder(x, v, &beta);
  const double sigma = x[0] * x[0] + x[1] * x[1];
  CHECK_T((sigma <= kSphereEpsilon) == expect_sigma_branch);
  if (expect_beta >= 0.0) CHECK_T(beta == expect_beta);
  const double nx = Norm(x);
  // H x = |x| e3
  const double vx = beta * (v[0] * x[0] + v[1] * x[1] + v[2] * x[2]);
  const double Hx[3] = {x[0] - vx * v[0], x[1] - vx * v[1], x[2] - vx * v[2]};
  CHECK_T(std::fabs(Hx[0]) <= 1e-15 * nx && std::fabs(Hx[1]) <= 1e-15 * nx && std::fabs(Hx[2] - nx) <= 1e-15 * nx);
  // Plus(x, 0) = x, bit for bit
  const double zero[2] = {0.0, 0.0};
  double p[3];
  sphere_plus(x, zero, p);
  CHECK_T(p[0] == x[0] && p[1] == x[1] && p[2] == x[2]);
  // |Plus(x, d)| = |x|
  const double steps[3][2] = {{0.3, -0.2}, {1e-3, 2e-3}, {-1.4, 2.5}};
  for (const auto& d : steps) {
    sphere_plus(x, d, p);
    CHECK_T(std::fabs(Norm(p) - nx) <= 4e-16 * nx);
  }
  // PlusJacobian against a central difference of Plus at 0
  double J[6];
  sphere_plus_jacobian(x, J);
  const double h = 1e-6;
  for (int i = 0; i < 2; ++i) {
    double dp[2] = {0.0, 0.0}, dm[2] = {0.0, 0.0}, pp[3], pm[3];
    dp[i] = h;
    dm[i] = -h;
    sphere_plus(x, dp, pp);
    sphere_plus(x, dm, pm);
    for (int r = 0; r < 3; ++r) CHECK_T(std::fabs((pp[r] - pm[r]) / (2 * h) - J[r * 2 + i]) <= 1e-7 * nx);
  }
  std::printf("PASS %s\n", name);
}

int main(int argc, char** argv) {
  if (argc > 2 && std::strcmp(argv[1], "rows") == 0) {
    if (Rows(argv[2]) != 0) return 1;
  } else {
    const double a[3] = {0.0, 0.0, -1.0}, b[3] = {0.0, 0.0, -0.1}, c[3] = {0.0, 0.0, 7.0}, d[3] = {0.0, 0.0, 1.0};
    const double e[3] = {0.3, -0.5, -0.81}, f[3] = {0.6, 0.0, 0.0}, g[3] = {-0.2, 0.4, 0.89}, h[3] = {2.1, -3.5, 4.2};
    Chart("SigmaSmallNegative", a, true, 2.0);
    Chart("SigmaSmallNegativeShort", b, true, 2.0);
    Chart("SigmaSmallPositiveLong", c, true, 0.0);
    Chart("SigmaSmallPositive", d, true, 0.0);
    Chart("NegativeZ", e, false, -1.0);
    Chart("ZeroZ", f, false, -1.0);
    Chart("PositiveZ", g, false, -1.0);
    Chart("PositiveZLong", h, false, -1.0);
  }
  std::printf("%d failure(s)\n", g_failures);
  return g_failures == 0 ? 0 : 1;
}
