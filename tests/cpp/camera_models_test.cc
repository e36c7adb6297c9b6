// camera_models_test.cc — fisheye cameras through the colmap_amd facade.
//
//   ./camera_models_test host   Camera::WorldToImage / ImageToWorld round trips,
//                               parameter counts, FULL_OPENCV refused (no GPU)
//   ./camera_models_test gpu    BundleAdjuster::Solve of a small reconstruction
//                               with OPENCV_FISHEYE cameras on the MI355X
#include <cmath>
#include <cstdio>
#include <random>
#include <string>
#include <vector>

#include "colmap_amd/bundle_adjustment.h"

using namespace colmap_amd;

static int g_failures = 0;
#define CHECK_T(cond)                                                        \
  do {                                                                       \
    if (!(cond)) {                                                           \
      std::printf("  FAILED %s:%d: %s\n", __FILE__, __LINE__, #cond);        \
      ++g_failures;                                                          \
    }                                                                        \
  } while (0)

static const std::vector<double> kFisheyeParams = {600, 598, 500, 500, -0.05, 0.01, -0.001, 0.001};

// Points in [-1, 1]^3 seen by cameras 3 units away (field radius up to ~0.9),
// observations projected by the camera itself plus U(-1, 1) px noise.
static Reconstruction GenerateReconstruction(int model, const std::vector<double>& params, int num_images,
                                             int num_points) {
  std::mt19937 prng(0);
  auto real = [&](double a, double b) { return std::uniform_real_distribution<double>(a, b)(prng); };
  Reconstruction rec;
  std::vector<point3D_t> ids;
  for (int i = 0; i < num_points; ++i) {
    double xyz[3] = {real(-1, 1), real(-1, 1), real(-1, 1)};
    ids.push_back(rec.AddPoint3D(xyz));
  }
  for (int i = 0; i < num_images; ++i) {
    Camera cam;
    cam.camera_id = (camera_t)i;
    cam.model_id = model;
    cam.params = params;
    rec.AddCamera(cam);
    Image im;
    im.image_id = (image_t)i;
    im.camera_id = (camera_t)i;
    im.name = std::to_string(i);
    im.tvec[0] = real(-0.5, 0.5);
    im.tvec[1] = real(-0.5, 0.5);
    im.tvec[2] = 3;
    for (point3D_t id : ids) {
      const double* X = rec.GetPoint3D(id).xyz;
      const double pz = X[2] + im.tvec[2];
      Point2D p2;
      if (mi_ba_num_params(model) > 0) {
        const auto xy = cam.WorldToImage({{(X[0] + im.tvec[0]) / pz, (X[1] + im.tvec[1]) / pz}});
        p2.xy[0] = xy[0] + real(-1.0, 1.0);
        p2.xy[1] = xy[1] + real(-1.0, 1.0);
      }
      im.points2D.push_back(p2);
    }
    rec.AddImage(im);
  }
  for (int i = 0; i < num_images; ++i) {
    point2D_t idx = 0;
    for (point3D_t id : ids) rec.AddObservation(id, TrackElement{(image_t)i, idx++});
  }
  return rec;
}

static BundleAdjustmentConfig ThreeViewConfig() {
  BundleAdjustmentConfig config;
  config.AddImage(0);
  config.AddImage(1);
  config.AddImage(2);
  config.SetConstantPose(0);
  config.SetConstantTvec(1, {0});
  return config;
}

static void Host() {
  std::printf("TestParameterCounts\n");
  CHECK_T(mi_ba_num_params(MI_BA_OPENCV_FISHEYE) == 8);
  CHECK_T(mi_ba_num_params(MI_BA_FOV) == 5);
  CHECK_T(mi_ba_num_params(MI_BA_SIMPLE_RADIAL_FISHEYE) == 4);
  CHECK_T(mi_ba_num_params(MI_BA_RADIAL_FISHEYE) == 5);
  CHECK_T(mi_ba_num_params(6) == -1);
  CHECK_T(mi_ba_num_params(10) == -1);
  std::printf("  PASS\n");

  std::printf("TestCameraRoundTrip\n");
  {
    Camera cam;
    cam.model_id = MI_BA_OPENCV_FISHEYE;
    cam.params = kFisheyeParams;
    CHECK_T(cam.params.size() == 8);
    for (double u = -0.5; u <= 0.5; u += 0.1)
      for (double v = -0.5; v <= 0.5; v += 0.1) {
        const auto xy = cam.WorldToImage({{u, v}});
        const auto uv = cam.ImageToWorld(xy);
        CHECK_T(std::fabs(uv[0] - u) < 1e-6 && std::fabs(uv[1] - v) < 1e-6);
      }
    const auto c = cam.WorldToImage({{0.0, 0.0}});
    CHECK_T(c[0] == 500 && c[1] == 500);
    Camera full;
    full.model_id = 6;  // FULL_OPENCV
    full.params.assign(12, 0.0);
    bool threw = false;
    try {
      full.WorldToImage({{0.1, 0.1}});
    } catch (const std::domain_error&) {
      threw = true;
    }
    CHECK_T(threw);
  }
  std::printf("  PASS\n");

  std::printf("TestSetUpCounts\n");
  {
    Reconstruction rec = GenerateReconstruction(MI_BA_OPENCV_FISHEYE, kFisheyeParams, 3, 60);
    BundleAdjustmentOptions options;
    options.print_summary = false;
    BundleAdjuster ba(options, ThreeViewConfig());
    const mi_ba_setup_info info = ba.SetUpInfo(rec);
    CHECK_T(info.num_residuals_reduced == 2 * 3 * 60);
    CHECK_T(info.camera_tangent_size == 6);  // fx fy k1..k4
    // 2 variable poses (6 + 5), 3 cameras x 6, 60 points x 3
    CHECK_T(info.num_effective_parameters_reduced == 11 + 18 + 180);
  }
  std::printf("  PASS\n");

  std::printf("TestFullOpenCVRefused\n");
  {
    Reconstruction rec = GenerateReconstruction(6, std::vector<double>(12, 0.0), 3, 10);
    BundleAdjustmentOptions options;
    options.print_summary = false;
    BundleAdjuster ba(options, ThreeViewConfig());
    bool threw = false;
    try {
      ba.Solve(&rec);
    } catch (const std::domain_error&) {
      threw = true;
    }
    CHECK_T(threw);
  }
  std::printf("  PASS\n");
}

static void Gpu() {
  std::printf("TestFisheyeSolve\n");
  Reconstruction rec = GenerateReconstruction(MI_BA_OPENCV_FISHEYE, kFisheyeParams, 3, 60);
  // start away from the optimum: perturbed points
  std::mt19937 prng(1);
  for (auto& p : rec.points3D)
    for (int k = 0; k < 3; ++k) p.second.xyz[k] += std::normal_distribution<double>(0.0, 0.01)(prng);
  const Reconstruction orig = rec;
  BundleAdjustmentOptions options;
  options.print_summary = false;
  BundleAdjuster ba(options, ThreeViewConfig());
  CHECK_T(ba.Solve(&rec));
  CHECK_T(ba.Summary().num_residuals_reduced == 2 * 3 * 60);
  CHECK_T(ba.Summary().num_effective_parameters_reduced == 11 + 18 + 180);
  CHECK_T(ba.Summary().final_cost < ba.Summary().initial_cost);
  // U(-1, 1) px noise on 360 residuals: the optimum's cost is near 360 / 6
  CHECK_T(ba.Summary().final_cost < 360.0 / 3.0);
  CHECK_T(rec.GetCamera(0).params.size() == 8);
  CHECK_T(rec.GetCamera(1).params[0] != orig.cameras.at(1).params[0]);  // focal refined
  CHECK_T(rec.GetCamera(1).params[4] != orig.cameras.at(1).params[4]);  // k1 refined
  CHECK_T(rec.GetCamera(1).params[2] == orig.cameras.at(1).params[2]);  // principal point constant
  std::printf("  initial %.6g final %.6g\n", ba.Summary().initial_cost, ba.Summary().final_cost);
  std::printf("  PASS\n");
}

int main(int argc, char** argv) {
  const std::string mode = argc > 1 ? argv[1] : "host";
  if (mode == "gpu")
    Gpu();
  else
    Host();
  std::printf("%d failure(s)\n", g_failures);
  return g_failures == 0 ? 0 : 1;
}
