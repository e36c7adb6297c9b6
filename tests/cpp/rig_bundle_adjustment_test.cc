// rig_bundle_adjustment_test.cc — the reference's RigBundleAdjuster tests
// (src/optim/bundle_adjustment_test.cc:755-969: TestRigTwoView,
// TestRigFourView, TestConstantRigFourView, TestRigFourViewPartial) and
// CameraRig checks, through the colmap_amd facade
// (include/colmap_amd/camera_rig.h) on libmi_ba.so.
//
//   ./rig_bundle_adjustment_test host   CameraRig + structural counts (no GPU)
//   ./rig_bundle_adjustment_test gpu    full Solve on the MI355X + the
//                                       CheckVariable* / CheckConstant* assertions
#include <cmath>
#include <cstdio>
#include <cstring>
#include <functional>
#include <random>
#include <string>
#include <vector>

#include "colmap_amd/camera_rig.h"

using namespace colmap_amd;

static int g_failures = 0;
#define CHECK_T(cond)                                                        \
  do {                                                                       \
    if (!(cond)) {                                                           \
      std::printf("  FAILED %s:%d: %s\n", __FILE__, __LINE__, #cond);        \
      ++g_failures;                                                          \
    }                                                                        \
  } while (0)

static std::mt19937* g_prng = nullptr;
static double RandomReal(double a, double b) { return std::uniform_real_distribution<double>(a, b)(*g_prng); }

// GenerateReconstruction (bundle_adjustment_test.cc:123-184), SIMPLE_RADIAL,
// f = 1.2 * 1000, identity rotations, tvec = (U, U, 10), U(-2, 2) noise.
static Reconstruction GenerateReconstruction(int num_images, int num_points) {
  std::mt19937 prng(0);
  g_prng = &prng;
  Reconstruction rec;
  std::vector<point3D_t> ids;
  for (int i = 0; i < num_points; ++i) {
    double xyz[3];
    xyz[0] = RandomReal(-1, 1);
    xyz[1] = RandomReal(-1, 1);
    xyz[2] = RandomReal(-1, 1);
    ids.push_back(rec.AddPoint3D(xyz));
  }
  for (int i = 0; i < num_images; ++i) {
    Camera cam;
    cam.camera_id = (camera_t)i;
    cam.model_id = MI_BA_SIMPLE_RADIAL;
    cam.params = {1.2 * 1000, 500, 500, 0};
    rec.AddCamera(cam);
    Image im;
    im.image_id = (image_t)i;
    im.camera_id = (camera_t)i;
    im.name = std::to_string(i);
    im.tvec[0] = RandomReal(-1.0, 1.0);
    im.tvec[1] = RandomReal(-1.0, 1.0);
    im.tvec[2] = 10;
    for (point3D_t id : ids) {
      const double* X = rec.GetPoint3D(id).xyz;
      const double px = X[0] + im.tvec[0], py = X[1] + im.tvec[1], pz = X[2] + im.tvec[2];
      const double u = px / pz, v = py / pz;  // SIMPLE_RADIAL with k = 0
      Point2D p2;
      p2.xy[0] = 1200 * u + 500 + RandomReal(-2.0, 2.0);
      p2.xy[1] = 1200 * v + 500 + RandomReal(-2.0, 2.0);
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

static bool Same(const double* a, const double* b, int n) { return std::memcmp(a, b, sizeof(double) * n) == 0; }
static void CheckVariableCamera(Reconstruction& r, const Reconstruction& o, camera_t c) {
  CHECK_T(r.GetCamera(c).params[0] != o.cameras.at(c).params[0]);
  CHECK_T(r.GetCamera(c).params[3] != o.cameras.at(c).params[3]);
}
static void CheckVariableImage(Reconstruction& r, const Reconstruction& o, image_t i) {
  CHECK_T(!Same(r.GetImage(i).qvec, o.GetImage(i).qvec, 4));
  CHECK_T(!Same(r.GetImage(i).tvec, o.GetImage(i).tvec, 3));
}
static void CheckConstantCameraRig(const CameraRig& r, const CameraRig& o, camera_t c) {
  CHECK_T(Same(r.RelativeQvec(c), o.RelativeQvec(c), 4));
  CHECK_T(Same(r.RelativeTvec(c), o.RelativeTvec(c), 3));
}
static void CheckVariableCameraRig(const CameraRig& r, const CameraRig& o, camera_t c) {
  if (r.RefCameraId() == c) {
    CheckConstantCameraRig(r, o, c);
  } else {
    CHECK_T(!Same(r.RelativeQvec(c), o.RelativeQvec(c), 4));
    CHECK_T(!Same(r.RelativeTvec(c), o.RelativeTvec(c), 3));
  }
}

static CameraRig TwoCameraRig(const std::vector<std::vector<image_t>>& snapshots) {
  const double q[4] = {1, 0, 0, 0}, t[3] = {0, 0, 0};  // ComposeIdentityQuaternion(), (0, 0, 0)
  CameraRig rig;
  rig.AddCamera(0, q, t);
  rig.AddCamera(1, q, t);
  for (const auto& s : snapshots) rig.AddSnapshot(s);
  rig.SetRefCameraId(0);
  return rig;
}

template <typename F>
static bool Throws(F&& f) {
  try {
    f();
  } catch (const std::invalid_argument&) {
    return true;
  }
  return false;
}

struct RigCase {
  std::string name;
  int images;
  std::vector<std::vector<image_t>> snapshots;
  bool refine_relative_poses;
  int64_t residuals, params;
};

static void RunRigCase(const RigCase& c, bool solve) {
  Reconstruction rec = GenerateReconstruction(c.images, 100);
  if (c.images == 4) {
    rec.images.at(2).camera_id = 0;
    rec.images.at(3).camera_id = 1;
  }
  const Reconstruction orig = rec;
  BundleAdjustmentConfig config;
  for (int i = 0; i < c.images; ++i) config.AddImage((image_t)i);
  std::vector<CameraRig> rigs{TwoCameraRig(c.snapshots)};
  const std::vector<CameraRig> orig_rigs = rigs;
  BundleAdjustmentOptions options;
  RigBundleAdjuster::Options rig_options;
  rig_options.refine_relative_poses = c.refine_relative_poses;
  RigBundleAdjuster ba(options, rig_options, config);
  const mi_ba_setup_info info = ba.SetUpInfo(rec, rigs);
  CHECK_T(info.num_residuals_reduced == c.residuals);
  CHECK_T(info.num_effective_parameters_reduced == c.params);
  if (!solve) return;
  CHECK_T(ba.Solve(&rec, &rigs));
  CHECK_T(ba.Summary().num_residuals_reduced == c.residuals);
  CHECK_T(ba.Summary().num_effective_parameters_reduced == c.params);
  CHECK_T(ba.Summary().final_cost < ba.Summary().initial_cost);
  CheckVariableCamera(rec, orig, 0);
  CheckVariableImage(rec, orig, 0);
  CheckVariableCamera(rec, orig, 1);
  CheckVariableImage(rec, orig, 1);
  for (camera_t cam = 0; cam < 2; ++cam) {
    if (c.refine_relative_poses) CheckVariableCameraRig(rigs[0], orig_rigs[0], cam);
    else CheckConstantCameraRig(rigs[0], orig_rigs[0], cam);
  }
  for (const auto& p : rec.points3D) CHECK_T(!Same(p.second.xyz, orig.points3D.at(p.first).xyz, 3));
  // TearDown: every snapshot image's pose is the concatenation of the rig's pose
  // (not exposed by the reference's API either) and its relative pose, so two
  // images of a snapshot differ by their cameras' relative poses alone
  if (!c.refine_relative_poses) {
    for (const auto& s : c.snapshots)
      if (s.size() == 2) {
        CHECK_T(std::fabs(rec.GetImage(s[0]).tvec[0] - rec.GetImage(s[1]).tvec[0]) < 1e-12);
        CHECK_T(std::fabs(rec.GetImage(s[0]).qvec[1] - rec.GetImage(s[1]).qvec[1]) < 1e-12);
      }
  }
  bool threw = false;
  try {
    ba.Solve(&rec, &rigs);
  } catch (const std::logic_error&) {
    threw = true;
  }
  CHECK_T(threw);  // "Cannot use the same BundleAdjuster multiple times"
}

static void TestCameraRigHost() {
  Reconstruction rec = GenerateReconstruction(4, 10);
  rec.images.at(2).camera_id = 0;
  rec.images.at(3).camera_id = 1;
  const double q[4] = {1, 0, 0, 0}, t[3] = {0, 0, 0};
  CameraRig rig = TwoCameraRig({{0, 1}, {2, 3}});
  rig.Check(rec);
  CHECK_T(rig.NumCameras() == 2 && rig.NumSnapshots() == 2 && rig.HasCamera(1) && !rig.HasCamera(2));
  CHECK_T(Throws([&] { rig.AddCamera(0, q, t); }));          // twice
  CHECK_T(Throws([&] { rig.AddCamera(5, q, t); }));          // after a snapshot
  CHECK_T(Throws([&] { rig.AddSnapshot({}); }));             // empty
  CHECK_T(Throws([&] { rig.AddSnapshot({0, 1, 2}); }));      // more images than cameras
  CHECK_T(Throws([&] { rig.AddSnapshot({1, 1}); }));         // duplicate
  CHECK_T(Throws([&] { rig.SetRefCameraId(7); }));           // not in the rig
  CHECK_T(Throws([&] { CameraRig r; r.AddCamera(0, q, t); r.Check(rec); }));                       // no reference camera
  CHECK_T(Throws([&] { TwoCameraRig({{0, 1}, {0, 3}}).Check(rec); }));                              // image in two snapshots
  CHECK_T(Throws([&] { TwoCameraRig({{0, 1}, {3}}).Check(rec); }));                                 // snapshot without the reference camera
  CHECK_T(Throws([&] { Reconstruction r2 = rec; r2.images.at(3).camera_id = 2; TwoCameraRig({{0, 1}, {2, 3}}).Check(r2); }));
  // the library's own checks through the adjuster: a camera in two rigs, a
  // rig image with a constant pose
  {
    BundleAdjustmentConfig config;
    for (int i = 0; i < 4; ++i) config.AddImage((image_t)i);
    std::vector<CameraRig> rigs{TwoCameraRig({{0, 1}}), TwoCameraRig({{2, 3}})};
    RigBundleAdjuster ba(BundleAdjustmentOptions(), RigBundleAdjuster::Options(), config);
    CHECK_T(Throws([&] { ba.SetUpInfo(rec, rigs); }));
    config.SetConstantPose(1);
    std::vector<CameraRig> one{TwoCameraRig({{0, 1}, {2, 3}})};
    RigBundleAdjuster ba2(BundleAdjustmentOptions(), RigBundleAdjuster::Options(), config);
    CHECK_T(Throws([&] { ba2.SetUpInfo(rec, one); }));
  }
  // ComputeAbsolutePose: images that share one rig pose exactly return it
  {
    const double rq[4] = {0.9, 0.1, -0.2, 0.3}, rt[3] = {0.5, -1.0, 2.0};
    const double lq[4] = {0.99, 0.05, 0.02, -0.03}, lt[3] = {0.3, 0.0, -0.1};
    CameraRig r;
    r.AddCamera(0, q, t);
    r.AddCamera(1, lq, lt);
    r.AddSnapshot({0, 1});
    r.SetRefCameraId(0);
    Reconstruction r2 = rec;
    ConcatenatePoses(rq, rt, q, t, r2.images.at(0).qvec, r2.images.at(0).tvec);
    ConcatenatePoses(rq, rt, lq, lt, r2.images.at(1).qvec, r2.images.at(1).tvec);
    double aq[4], at[3], nq[4];
    r.ComputeAbsolutePose(0, r2, aq, at);
    internal::NormalizeQuat(rq, nq);
    for (int k = 0; k < 4; ++k) CHECK_T(std::fabs(aq[k] - nq[k]) < 1e-14);
    for (int k = 0; k < 3; ++k) CHECK_T(std::fabs(at[k] - rt[k]) < 1e-14);
  }
  // ... and two poses that disagree by a small rotation return
  // AverageQuaternions' result.  By hand for q1 = (1, 0, 0, 0), q2 = (c, s, 0,
  // 0): A = (q1 q1' + q2 q2') / 2 acts on the (w, x) plane, its dominant
  // eigenvector is the bisector (cos(a / 2), sin(a / 2), 0, 0), c = cos a.
  {
    const double a = 0.02;
    Reconstruction r2 = rec;
    const double q2[4] = {std::cos(a), std::sin(a), 0, 0};
    std::copy(q, q + 4, r2.images.at(0).qvec);
    std::copy(q2, q2 + 4, r2.images.at(1).qvec);
    for (int k = 0; k < 3; ++k) {
      r2.images.at(0).tvec[k] = 1.0 + k;
      r2.images.at(1).tvec[k] = 3.0 + k;
    }
    CameraRig r = TwoCameraRig({{0, 1}});
    double aq[4], at[3];
    r.ComputeAbsolutePose(0, r2, aq, at);
    const double want[4] = {std::cos(a / 2), std::sin(a / 2), 0, 0};
    for (int k = 0; k < 4; ++k) CHECK_T(std::fabs(aq[k] - want[k]) < 1e-14);
    for (int k = 0; k < 3; ++k) CHECK_T(std::fabs(at[k] - (2.0 + k)) < 1e-14);
  }
}

int main(int argc, char** argv) {
  const std::string mode = argc > 1 ? argv[1] : "host";
  const bool solve = mode == "gpu";
  const std::vector<RigCase> cases = {
      {"TestRigTwoView", 2, {{0, 1}}, true, 400, 316},
      {"TestRigFourView", 4, {{0, 1}, {2, 3}}, true, 800, 322},
      {"TestConstantRigFourView", 4, {{0, 1}, {2, 3}}, false, 800, 316},
      {"TestRigFourViewPartial", 4, {{0, 1}, {2}}, true, 800, 328},
  };
  if (!solve) {
    const int before = g_failures;
    TestCameraRigHost();
    std::printf("%s CameraRig\n", g_failures == before ? "PASS" : "FAIL");
  }
  for (const RigCase& c : cases) {
    const int before = g_failures;
    RunRigCase(c, solve);
    std::printf("%s %s\n", g_failures == before ? "PASS" : "FAIL", c.name.c_str());
  }
  std::printf("%d failure(s)\n", g_failures);
  return g_failures == 0 ? 0 : 1;
}
