// The facade of the robust absolute pose (include/colmap_amd/pose.h:
// AbsolutePoseEstimationOptions, EstimateAbsolutePose) against libmi_ba.so.
//
//   absolute_pose_test check                  options Check() and the argument checks (no device)
//   absolute_pose_test factors N MIN MAX      the sweep's focal length factors as hex floats (no device)
//   absolute_pose_test sweep IN               EstimateAbsolutePose with estimate_focal_length on the one
//                                             problem of the batch file IN (tests/test_absolute_pose.py)
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "colmap_amd/pose.h"

using namespace colmap_amd;

namespace {

int failures = 0;
#define EXPECT(cond)                                                \
  do {                                                              \
    if (!(cond)) {                                                  \
      std::printf("FAILED %s:%d %s\n", __FILE__, __LINE__, #cond); \
      ++failures;                                                   \
    }                                                               \
  } while (0)

template <typename F>
bool Throws(F f) {
  try {
    f();
  } catch (const std::invalid_argument&) {
    return true;
  }
  return false;
}

void Check() {
  AbsolutePoseEstimationOptions o;
  // the reference's defaults (estimators/pose.h:51-70)
  EXPECT(!o.estimate_focal_length && o.num_focal_length_samples == 30 && o.min_focal_length_ratio == 0.2 &&
         o.max_focal_length_ratio == 5.0);
  EXPECT(Throws([&] { o.Check(); }));  // max_error has no default
  o.ransac_options.max_error = 12.0;
  EXPECT(!Throws([&] { o.Check(); }));
  for (int which = 0; which < 4; ++which) {
    AbsolutePoseEstimationOptions b = o;
    if (which == 0) b.num_focal_length_samples = 0;
    if (which == 1) b.min_focal_length_ratio = 0.0;
    if (which == 2) b.max_focal_length_ratio = -1.0;
    if (which == 3) b.min_focal_length_ratio = 6.0;
    EXPECT(Throws([&] { b.Check(); }));
  }
  // the size check and a null argument, before any device is touched
  std::vector<std::array<double, 2>> p2(4);
  std::vector<std::array<double, 3>> p3(5);
  std::array<double, 4> q{};
  std::array<double, 3> t{};
  Camera cam;
  cam.model_id = MI_BA_SIMPLE_PINHOLE;
  cam.params = {1000.0, 500.0, 500.0};
  size_t inliers = 0;
  std::vector<char> mask;
  EXPECT(Throws([&] { EstimateAbsolutePose(o, p2, p3, &q, &t, &cam, &inliers, &mask); }));
  p3.resize(4);
  EXPECT(Throws([&] { EstimateAbsolutePose(o, p2, p3, &q, &t, nullptr, &inliers, &mask); }));
  // the unbounded-trials case is an invalid argument of the library
  AbsolutePoseEstimationOptions u = o;
  u.ransac_options.confidence = 1.0;
  EXPECT(Throws([&] { EstimateAbsolutePose(u, p2, p3, &q, &t, &cam, &inliers, &mask); }));
  EXPECT(EstimateAbsolutePoses(o, {}).empty());
}

template <typename T>
bool ReadVec(std::FILE* f, std::vector<T>* v, size_t n) {
  v->resize(n);
  return n == 0 || std::fread(v->data(), sizeof(T), n, f) == n;
}

int Sweep(const char* path) {
  std::FILE* f = std::fopen(path, "rb");
  if (!f) return 1;
  int64_t head[4], trials[2];
  double opt[4];
  std::vector<int64_t> off;
  std::vector<double> x2, x3, prm8, factor;
  std::vector<int32_t> models, set_index, camera_index;
  std::vector<uint64_t> seed;
  bool ok = std::fread(head, 8, 4, f) == 4 && std::fread(opt, 8, 4, f) == 4 && std::fread(trials, 8, 2, f) == 2;
  ok = ok && head[0] == 1 && ReadVec(f, &off, (size_t)head[1] + 1) && ReadVec(f, &x2, 2 * (size_t)head[2]) &&
       ReadVec(f, &x3, 3 * (size_t)head[2]) && ReadVec(f, &models, (size_t)head[3]) &&
       ReadVec(f, &prm8, 8 * (size_t)head[3]) && ReadVec(f, &set_index, 1) && ReadVec(f, &camera_index, 1) &&
       ReadVec(f, &factor, 1) && ReadVec(f, &seed, 1);
  std::fclose(f);
  if (!ok) return 1;
  AbsolutePoseEstimationOptions o;
  o.estimate_focal_length = true;
  o.ransac_options.max_error = opt[0];
  o.ransac_options.min_inlier_ratio = opt[1];
  o.ransac_options.confidence = opt[2];
  o.ransac_options.dyn_num_trials_multiplier = opt[3];
  o.ransac_options.min_num_trials = (size_t)trials[0];
  o.ransac_options.max_num_trials = (size_t)trials[1];
  o.seed = seed[0];
  const size_t n = (size_t)head[2];
  std::vector<std::array<double, 2>> p2(n);
  std::vector<std::array<double, 3>> p3(n);
  for (size_t i = 0; i < n; ++i) {
    p2[i] = {{x2[2 * i], x2[2 * i + 1]}};
    p3[i] = {{x3[3 * i], x3[3 * i + 1], x3[3 * i + 2]}};
  }
  Camera cam;
  cam.model_id = models[0];
  cam.params.assign(prm8.begin(), prm8.begin() + mi_ba_num_params(models[0]));
  std::array<double, 4> q{};
  std::array<double, 3> t{};
  size_t inliers = 0;
  std::vector<char> mask;
  const bool success = EstimateAbsolutePose(o, p2, p3, &q, &t, &cam, &inliers, &mask);
  std::string m;
  for (char c : mask) m += c ? '1' : '0';
  std::printf("SWEEP %d %zu %a %s\n", success ? 1 : 0, inliers, cam.params[0], m.empty() ? "-" : m.c_str());
  return 0;
}

}  // namespace

int main(int argc, char** argv) {
  if (argc >= 2 && std::strcmp(argv[1], "check") == 0) {
    Check();
  } else if (argc >= 5 && std::strcmp(argv[1], "factors") == 0) {
    AbsolutePoseEstimationOptions o;
    o.estimate_focal_length = true;
    o.num_focal_length_samples = (size_t)std::atoll(argv[2]);
    o.min_focal_length_ratio = std::atof(argv[3]);
    o.max_focal_length_ratio = std::atof(argv[4]);
    std::printf("FACTORS");
    for (double f : internal::FocalLengthFactors(o)) std::printf(" %a", f);
    std::printf("\n");
    o.estimate_focal_length = false;
    EXPECT(internal::FocalLengthFactors(o) == std::vector<double>({1.0}));
  } else if (argc >= 3 && std::strcmp(argv[1], "sweep") == 0) {
    if (Sweep(argv[2]) != 0) {
      std::printf("cannot run %s\n", argv[2]);
      return 1;
    }
  } else {
    std::printf("usage: absolute_pose_test check | factors N MIN MAX | sweep IN\n");
    return 1;
  }
  std::printf("%d failure(s)\n", failures);
  return failures == 0 ? 0 : 1;
}
