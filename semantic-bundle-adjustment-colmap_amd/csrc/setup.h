// setup.h — host-side problem assembly (product code).
//
// Array-based restatement of BundleAdjuster::SetUp / AddImageToProblem /
// AddPointToProblem / ParameterizeCameras / ParameterizePoints
// (src/optim/bundle_adjustment.cc:326-530) plus Ceres' reduced-program rule
// (residual blocks whose parameter blocks are all constant are dropped and
// their cost is reported as fixed_cost).  Linear in the number of
// observations (CSR by image and by point) so it scales to 10M observations.
#pragma once

#include <cstdint>
#include <vector>

#include "../../include/mi_ba.h"

namespace miba {

struct HostSetup {
  int model = 0;       // the problem's camera model, or kMixedModels
  int np = 0;          // params per camera (the largest, mixed models)
  int ct = 0;          // refined intrinsics slots per camera (the largest, mixed models)
  int cam_tan_idx[8] = {0, 0, 0, 0, 0, 0, 0, 0};  // single-model problems
  // per camera: model id, offset of its params in mi_ba_problem::camera_params,
  // refined intrinsics (its slots ct_c..ct-1 are padding: zero Jacobian columns)
  std::vector<int32_t> cam_model;
  std::vector<int64_t> cam_off;
  std::vector<uint8_t> cam_ct;
  std::vector<int64_t> reduced_obs;   // observation index of each reduced block (program order)
  std::vector<int64_t> fixed_obs;     // blocks dropped from the reduced program
  std::vector<uint8_t> img_var;       // pose is a variable parameter block
  std::vector<uint8_t> img_tvec_mask; // SubsetManifold(3, idxs) on tvec
  std::vector<uint8_t> cam_var;
  std::vector<uint8_t> pt_var;
  int64_t num_residual_blocks = 0;
  int64_t num_residuals_reduced = 0;
  int64_t num_effective_parameters_reduced = 0;
};

// Model id of camera c (camera_model_ids, else camera_model).
inline int problem_camera_model(const mi_ba_problem* p, int c) {
  return p->camera_model_ids ? p->camera_model_ids[c] : p->camera_model;
}

// Validates the problem, normalises config qvecs in place (Image::NormalizeQvec
// at bundle_adjustment.cc:355) and fills `s`.
// obs_skip (nullable, [num_obs]): observations of config images that are not
// added to the problem (the rig set-up's reprojection-error filter).
// pose_const_by_config_only: a pose is constant by the config alone
// (RigBundleAdjuster::AddImageToProblem, bundle_adjustment.cc:915, does not
// read refine_extrinsics).
mi_ba_status build_setup(const mi_ba_options& o, mi_ba_problem* p, HostSetup* s, const uint8_t* obs_skip = nullptr,
                         bool pose_const_by_config_only = false);

// Camera rigs (RigBundleAdjuster::Solve / SetUp / AddImageToProblem,
// bundle_adjustment.cc:794-1058; CameraRig::Check, camera_rig.cc:86-110).
struct RigSetup {
  std::vector<int32_t> img_snapshot;  // [I] snapshot of a rig image, -1: in no rig
  std::vector<int32_t> img_rel;       // [I] position of its camera in the rig's camera list (rel_qvec / rel_tvec), -1
  std::vector<int32_t> img_rig;       // [I] rig, -1
  std::vector<uint8_t> obs_skip;      // [N] dropped by max_reproj_error at the concatenated pose
  std::vector<uint8_t> snapshot_used; // [num_snapshots] its rig pose carries an observation
  std::vector<uint8_t> rel_used;      // [rig cameras] the relative pose carries an observation
  std::vector<uint8_t> rel_var;       // ... and is variable (refine_relative_poses, not the reference camera)
  int64_t num_filtered = 0;
};

// ConcatenatePoses(rig, rel) (src/base/pose.cc:97-108,183-190): q = normalised
// (q_rel * q_rig) of the normalised inputs, t = t_rel + R(q_rel) t_rig.
void rig_concatenate_poses(const double rig_q[4], const double rig_t[3], const double rel_q[4],
                           const double rel_t[3], double q[4], double t[3]);

// Validates the rigs against the problem (MI_BA_ERR_INVALID_ARGUMENT where
// the reference CHECKs), filters the rig images' observations, runs
// build_setup and replaces the rig images' pose parameters by the snapshot
// and relative poses in the reduced-program counts of `s`.
mi_ba_status build_rig_setup(const mi_ba_options& o, mi_ba_problem* p, const mi_ba_rig& rig, HostSetup* s,
                             RigSetup* rs);

}  // namespace miba
