// setup.cpp — host-side problem assembly (product code); see setup.h.
#include "setup.h"

#include <algorithm>
#include <cmath>
#include <limits>

#include "ba_math.h"

namespace miba {

namespace {

void param_groups(int model, std::vector<int>* f, std::vector<int>* pp, std::vector<int>* ex) {
  // camera_models.h *::Initialize{FocalLength,PrincipalPoint,ExtraParams}Idxs
  switch (model) {
    case kSimplePinhole: *f = {0}; *pp = {1, 2}; *ex = {}; break;
    case kPinhole: *f = {0, 1}; *pp = {2, 3}; *ex = {}; break;
    case kSimpleRadial: *f = {0}; *pp = {1, 2}; *ex = {3}; break;
    case kRadial: *f = {0}; *pp = {1, 2}; *ex = {3, 4}; break;
    case kOpenCV: *f = {0, 1}; *pp = {2, 3}; *ex = {4, 5, 6, 7}; break;
    case kOpenCVFisheye: *f = {0, 1}; *pp = {2, 3}; *ex = {4, 5, 6, 7}; break;
    case kFOV: *f = {0, 1}; *pp = {2, 3}; *ex = {4}; break;
    case kSimpleRadialFisheye: *f = {0}; *pp = {1, 2}; *ex = {3}; break;
    case kRadialFisheye: *f = {0}; *pp = {1, 2}; *ex = {3, 4}; break;
    default: break;
  }
}

// CSR adjacency: items grouped by key, preserving original order.
void csr(const int32_t* key, int64_t n, int64_t nkeys, std::vector<int64_t>* off, std::vector<int64_t>* items) {
  off->assign(nkeys + 1, 0);
  for (int64_t k = 0; k < n; ++k) (*off)[key[k] + 1]++;
  for (int64_t k = 0; k < nkeys; ++k) (*off)[k + 1] += (*off)[k];
  items->resize(n);
  std::vector<int64_t> pos(off->begin(), off->end() - 1);
  for (int64_t k = 0; k < n; ++k) (*items)[pos[key[k]]++] = k;
}

}  // namespace

mi_ba_status build_setup(const mi_ba_options& o, mi_ba_problem* p, HostSetup* s, const uint8_t* obs_skip,
                         bool pose_const_by_config_only) {
  if (!p) return MI_BA_ERR_INVALID_ARGUMENT;
  if (p->num_images < 0 || p->num_cameras < 0 || p->num_points < 0 || p->num_obs < 0)
    return MI_BA_ERR_INVALID_ARGUMENT;
  if (p->num_obs > 0 && (!p->obs_xy || !p->obs_image || !p->obs_point)) return MI_BA_ERR_INVALID_ARGUMENT;
  if (p->num_images > 0 && (!p->qvec || !p->tvec || !p->image_camera)) return MI_BA_ERR_INVALID_ARGUMENT;
  if (p->num_cameras > 0 && !p->camera_params) return MI_BA_ERR_INVALID_ARGUMENT;
  if (p->num_points > 0 && !p->xyz) return MI_BA_ERR_INVALID_ARGUMENT;
  if (o.loss_function_scale < 0) return MI_BA_ERR_INVALID_ARGUMENT;  // BundleAdjustmentOptions::Check
  if (p->num_obs >= (int64_t)0xffffffffLL || p->num_points >= (int64_t)0xffffffffLL)
    return MI_BA_ERR_UNSUPPORTED;
  const int I = p->num_images, C = p->num_cameras;
  const int64_t P = p->num_points, N = p->num_obs;
  for (int i = 0; i < I; ++i)
    if (p->image_camera[i] < 0 || p->image_camera[i] >= C) return MI_BA_ERR_INVALID_ARGUMENT;
  for (int64_t k = 0; k < N; ++k)
    if (p->obs_image[k] < 0 || p->obs_image[k] >= I || p->obs_point[k] < 0 || p->obs_point[k] >= P)
      return MI_BA_ERR_INVALID_ARGUMENT;
  for (int i = 0; i < I; ++i) {
    // BundleAdjustmentConfig::SetConstantPose / SetConstantTvec CHECKs
    // (bundle_adjustment.cc:165-186): tvec subset and constant pose exclusive.
    const bool cp = p->image_constant_pose && p->image_constant_pose[i];
    const uint8_t tm = p->image_constant_tvec ? p->image_constant_tvec[i] : 0;
    if ((tm & ~7u) != 0) return MI_BA_ERR_INVALID_ARGUMENT;
    if (cp && tm) return MI_BA_ERR_INVALID_ARGUMENT;
  }
  // per-camera models (camera_models.h:117-141: unknown ids throw
  // std::domain_error, :140-141)
  if (!p->camera_model_ids && num_params(p->camera_model) < 0) return MI_BA_ERR_UNSUPPORTED;
  s->cam_model.assign(C, 0);
  s->cam_off.assign(C + 1, 0);
  bool mixed = false;
  int np = num_params(p->camera_model);
  for (int c = 0; c < C; ++c) {
    const int m = problem_camera_model(p, c);
    if (num_params(m) < 0) return MI_BA_ERR_UNSUPPORTED;
    s->cam_model[c] = m;
    s->cam_off[c + 1] = s->cam_off[c] + num_params(m);
    if (c == 0) np = num_params(m);
    if (m != s->cam_model[0]) mixed = true;
    np = std::max(np, num_params(m));
  }
  // a mixed problem with a fisheye or FOV camera takes the nine-model
  // run-time kernels, every other mixed problem the five-model ones
  bool wide = false;
  for (int c = 0; c < C; ++c) wide = wide || is_wide_angle_model(s->cam_model[c]);
  s->model = mixed ? (wide ? kMixedAllModels : kMixedModels) : (C > 0 ? s->cam_model[0] : p->camera_model);
  s->np = np;

  std::vector<int64_t> img_off, img_items, pt_off, pt_items;
  csr(p->obs_image, N, I, &img_off, &img_items);
  csr(p->obs_point, N, P, &pt_off, &pt_items);

  auto in_cfg = [&](int i) { return p->image_in_config ? p->image_in_config[i] != 0 : true; };
  std::vector<uint8_t> cam_in(C, 0), cam_const(C, 0);
  for (int c = 0; c < C; ++c) cam_const[c] = p->camera_constant ? (p->camera_constant[c] != 0) : 0;
  std::vector<int64_t> pt_nobs(P, 0);
  std::vector<int64_t> blocks;
  blocks.reserve(N);
  s->img_var.assign(I, 0);
  s->img_tvec_mask.assign(I, 0);

  // AddImageToProblem (bundle_adjustment.cc:348-427)
  for (int i = 0; i < I; ++i) {
    if (!in_cfg(i)) continue;
    double* q = p->qvec + 4 * (size_t)i;  // NormalizeQuaternion (pose.cc:82-91)
    const double norm = std::sqrt(q[0] * q[0] + q[1] * q[1] + q[2] * q[2] + q[3] * q[3]);
    if (norm == 0) {
      q[0] = 1.0;
    } else {
      for (int m = 0; m < 4; ++m) q[m] = q[m] / norm;
    }
    const bool cpose = (!o.refine_extrinsics && !pose_const_by_config_only) ||
                       (p->image_constant_pose && p->image_constant_pose[i]);
    int64_t nobs = 0;
    for (int64_t m = img_off[i]; m < img_off[i + 1]; ++m) {
      const int64_t k = img_items[m];
      if (obs_skip && obs_skip[k]) continue;
      ++nobs;
      pt_nobs[p->obs_point[k]] += 1;
      blocks.push_back(k);
    }
    if (nobs > 0) {
      cam_in[p->image_camera[i]] = 1;
      if (!cpose) {
        s->img_var[i] = 1;
        s->img_tvec_mask[i] = p->image_constant_tvec ? p->image_constant_tvec[i] : 0;
      }
    }
  }
  // AddPointToProblem (:429-478): variable points, then constant points.
  if (p->point_config) {
    for (int pass = 1; pass <= 2; ++pass) {
      for (int64_t pt = 0; pt < P; ++pt) {
        if (p->point_config[pt] != pass) continue;
        if (pt_nobs[pt] == pt_off[pt + 1] - pt_off[pt]) continue;
        for (int64_t m = pt_off[pt]; m < pt_off[pt + 1]; ++m) {
          const int64_t k = pt_items[m];
          const int img = p->obs_image[k];
          if (in_cfg(img)) continue;
          pt_nobs[pt] += 1;
          const int cam = p->image_camera[img];
          if (!cam_in[cam]) {
            cam_in[cam] = 1;
            cam_const[cam] = 1;  // config_.SetConstantCamera
          }
          blocks.push_back(k);
        }
      }
    }
  }
  // ParameterizeCameras (:480-516): SubsetManifold over the params the
  // refine flags hold constant, per camera model.
  auto tangent = [&](int model, int* idx) {
    std::vector<int> f, pp, ex;
    param_groups(model, &f, &pp, &ex);
    const int n = num_params(model);
    std::vector<uint8_t> is_const(n, 0);
    if (!o.refine_focal_length) for (int k : f) is_const[k] = 1;
    if (!o.refine_principal_point) for (int k : pp) is_const[k] = 1;
    if (!o.refine_extra_params) for (int k : ex) is_const[k] = 1;
    int ct = 0;
    for (int k = 0; k < n; ++k)
      if (!is_const[k]) {
        if (idx) idx[ct] = k;
        ++ct;
      }
    return ct;
  };
  s->ct = tangent(is_mixed(s->model) ? kOpenCV : s->model, s->cam_tan_idx);
  s->cam_ct.assign(C, 0);
  if (is_mixed(s->model)) {
    s->ct = 0;
    for (int c = 0; c < C; ++c) {
      s->cam_ct[c] = (uint8_t)tangent(s->cam_model[c], nullptr);
      s->ct = std::max<int>(s->ct, s->cam_ct[c]);
    }
  } else {
    for (int c = 0; c < C; ++c) s->cam_ct[c] = (uint8_t)s->ct;
  }
  const bool constant_camera = !o.refine_focal_length && !o.refine_principal_point && !o.refine_extra_params;
  s->cam_var.assign(C, 0);
  for (int c = 0; c < C; ++c)
    s->cam_var[c] = cam_in[c] && !constant_camera && !cam_const[c] && s->cam_ct[c] > 0;
  // ParameterizePoints (:518-530)
  s->pt_var.assign(P, 0);
  for (int64_t pt = 0; pt < P; ++pt) {
    if (pt_nobs[pt] == 0) continue;
    bool constant = (pt_off[pt + 1] - pt_off[pt]) > pt_nobs[pt];
    if (p->point_config && p->point_config[pt] == 2) constant = true;
    s->pt_var[pt] = !constant;
  }
  // Reduced program.
  s->num_residual_blocks = (int64_t)blocks.size();
  s->reduced_obs.clear();
  s->fixed_obs.clear();
  std::vector<uint8_t> used_img(I, 0), used_cam(C, 0);
  int64_t used_pts = 0;
  std::vector<uint8_t> used_pt(P, 0);
  for (int64_t k : blocks) {
    const int img = p->obs_image[k];
    const int cam = p->image_camera[img];
    const int64_t pt = p->obs_point[k];
    const bool vpose = s->img_var[img];
    if (!(vpose || s->cam_var[cam] || s->pt_var[pt])) {
      s->fixed_obs.push_back(k);
      continue;
    }
    s->reduced_obs.push_back(k);
    if (vpose) used_img[img] = 1;
    if (s->cam_var[cam]) used_cam[cam] = 1;
    if (s->pt_var[pt] && !used_pt[pt]) { used_pt[pt] = 1; ++used_pts; }
  }
  s->num_residuals_reduced = 2 * (int64_t)s->reduced_obs.size();
  int64_t ne = 3 * used_pts;
  for (int i = 0; i < I; ++i)
    if (used_img[i]) {
      int masked = 0;
      for (int k = 0; k < 3; ++k) masked += (s->img_tvec_mask[i] >> k) & 1;
      ne += 6 - masked;
    }
  for (int c = 0; c < C; ++c)
    if (used_cam[c]) ne += s->cam_ct[c];
  s->num_effective_parameters_reduced = ne;
  return MI_BA_OK;
}

namespace {

void normalize_quat(const double q[4], double out[4]) {  // NormalizeQuaternion (pose.cc:82-91)
  const double norm = std::sqrt(q[0] * q[0] + q[1] * q[1] + q[2] * q[2] + q[3] * q[3]);
  if (norm == 0) {
    out[0] = 1.0; out[1] = q[1]; out[2] = q[2]; out[3] = q[3];
  } else {
    for (int m = 0; m < 4; ++m) out[m] = q[m] / norm;
  }
}

}  // namespace

void rig_concatenate_poses(const double rig_q[4], const double rig_t[3], const double rel_q[4],
                           const double rel_t[3], double q[4], double t[3]) {
  double a[4], b[4], c[4], rt[3];
  normalize_quat(rig_q, a);
  normalize_quat(rel_q, b);
  // Eigen quat2 * quat1 with quat2 = rel, quat1 = rig
  c[0] = b[0] * a[0] - b[1] * a[1] - b[2] * a[2] - b[3] * a[3];
  c[1] = b[0] * a[1] + b[1] * a[0] + b[2] * a[3] - b[3] * a[2];
  c[2] = b[0] * a[2] + b[2] * a[0] + b[3] * a[1] - b[1] * a[3];
  c[3] = b[0] * a[3] + b[3] * a[0] + b[1] * a[2] - b[2] * a[1];
  normalize_quat(c, q);
  unit_quat_rotate(b, rig_t, rt);
  for (int k = 0; k < 3; ++k) t[k] = rel_t[k] + rt[k];
}

mi_ba_status build_rig_setup(const mi_ba_options& o, mi_ba_problem* p, const mi_ba_rig& rig, HostSetup* s,
                             RigSetup* rs) {
  if (!p || p->num_images < 0 || p->num_cameras < 0 || p->num_obs < 0 || p->num_points < 0)
    return MI_BA_ERR_INVALID_ARGUMENT;
  const int I = p->num_images, C = p->num_cameras, R = rig.num_rigs;
  if (I > 0 && !p->image_camera) return MI_BA_ERR_INVALID_ARGUMENT;
  if (R < 0 || rig.num_snapshots < 0 || rig.max_reproj_error < 0) return MI_BA_ERR_INVALID_ARGUMENT;
  if (R > 0 && (!rig.rig_camera_off || !rig.rig_ref_camera || !rig.rig_snapshot_off))
    return MI_BA_ERR_INVALID_ARGUMENT;
  for (int i = 0; i < I; ++i)
    if (p->image_camera[i] < 0 || p->image_camera[i] >= C) return MI_BA_ERR_INVALID_ARGUMENT;
  rs->img_snapshot.assign(I, -1);
  rs->img_rel.assign(I, -1);
  rs->img_rig.assign(I, -1);
  const int ncam = R > 0 ? rig.rig_camera_off[R] : 0;
  if (R > 0 && (rig.rig_camera_off[0] != 0 || rig.rig_snapshot_off[0] != 0 || ncam < 0 ||
                rig.rig_snapshot_off[R] != rig.num_snapshots))
    return MI_BA_ERR_INVALID_ARGUMENT;
  if (ncam > 0 && (!rig.rig_camera || !rig.rel_qvec || !rig.rel_tvec)) return MI_BA_ERR_INVALID_ARGUMENT;
  if (rig.num_snapshots > 0 && (!rig.snapshot_off || !rig.snapshot_qvec || !rig.snapshot_tvec || rig.snapshot_off[0] != 0))
    return MI_BA_ERR_INVALID_ARGUMENT;
  const int nsi = rig.num_snapshots > 0 ? rig.snapshot_off[rig.num_snapshots] : 0;
  if (nsi < 0 || (nsi > 0 && !rig.snapshot_image)) return MI_BA_ERR_INVALID_ARGUMENT;
  for (int sn = 0; sn < rig.num_snapshots; ++sn)
    if (rig.snapshot_off[sn + 1] < rig.snapshot_off[sn]) return MI_BA_ERR_INVALID_ARGUMENT;
  // Solve (:800-817) + CameraRig::Check
  std::vector<int32_t> cam_rig(C, -1), cam_pos(C, -1);
  for (int r = 0; r < R; ++r) {
    const int c0 = rig.rig_camera_off[r], c1 = rig.rig_camera_off[r + 1];
    const int s0 = rig.rig_snapshot_off[r], s1 = rig.rig_snapshot_off[r + 1];
    if (c1 < c0 || c1 > ncam || s1 < s0 || s1 > rig.num_snapshots) return MI_BA_ERR_INVALID_ARGUMENT;
    for (int k = c0; k < c1; ++k) {
      const int c = rig.rig_camera[k];
      if (c < 0 || c >= C) return MI_BA_ERR_INVALID_ARGUMENT;  // reconstruction.ExistsCamera
      if (cam_rig[c] >= 0) return MI_BA_ERR_INVALID_ARGUMENT;  // a camera in two rigs (or twice in one)
      cam_rig[c] = r;
      cam_pos[c] = k;
    }
    const int ref = rig.rig_ref_camera[r];
    if (ref < 0 || ref >= C || cam_rig[ref] != r) return MI_BA_ERR_INVALID_ARGUMENT;  // HasCamera(ref_camera_id_)
    for (int sn = s0; sn < s1; ++sn) {
      const int i0 = rig.snapshot_off[sn], i1 = rig.snapshot_off[sn + 1];
      if (i1 == i0 || i1 - i0 > c1 - c0) return MI_BA_ERR_INVALID_ARGUMENT;
      bool has_ref = false;
      for (int m = i0; m < i1; ++m) {
        const int img = rig.snapshot_image[m];
        if (img < 0 || img >= I) return MI_BA_ERR_INVALID_ARGUMENT;        // ExistsImage
        if (rs->img_snapshot[img] >= 0) return MI_BA_ERR_INVALID_ARGUMENT;  // in two snapshots / two rigs
        const int c = p->image_camera[img];
        if (cam_rig[c] != r) return MI_BA_ERR_INVALID_ARGUMENT;             // HasCamera(image.CameraId())
        for (int m2 = i0; m2 < m; ++m2)  // one image per camera and snapshot
          if (p->image_camera[rig.snapshot_image[m2]] == c) return MI_BA_ERR_INVALID_ARGUMENT;
        rs->img_snapshot[img] = sn;
        rs->img_rel[img] = cam_pos[c];
        rs->img_rig[img] = r;
        has_ref = has_ref || c == ref;
      }
      if (!has_ref) return MI_BA_ERR_INVALID_ARGUMENT;
    }
  }
  auto in_cfg = [&](int i) { return p->image_in_config ? p->image_in_config[i] != 0 : true; };
  // AddImageToProblem (:926-930)
  for (int i = 0; i < I; ++i) {
    if (rs->img_snapshot[i] < 0 || !in_cfg(i)) continue;
    if (p->image_constant_pose && p->image_constant_pose[i]) return MI_BA_ERR_INVALID_ARGUMENT;
    if (p->image_constant_tvec && p->image_constant_tvec[i]) return MI_BA_ERR_INVALID_ARGUMENT;
  }
  // the observation filter (:937-946, :970-975) needs the problem's arrays
  const int64_t N = p->num_obs;
  if (N > 0 && (!p->obs_xy || !p->obs_image || !p->obs_point || !p->xyz || !p->camera_params))
    return MI_BA_ERR_INVALID_ARGUMENT;
  std::vector<int64_t> cam_off(C + 1, 0);
  for (int c = 0; c < C; ++c) {
    const int n = num_params(problem_camera_model(p, c));
    if (n < 0) return MI_BA_ERR_UNSUPPORTED;
    cam_off[c + 1] = cam_off[c] + n;
  }
  std::vector<double> proj(12 * (size_t)I, 0.0);
  for (int i = 0; i < I; ++i) {
    if (rs->img_snapshot[i] < 0 || !in_cfg(i)) continue;
    double q[4], t[3];
    const int sn = rs->img_snapshot[i], k = rs->img_rel[i];
    rig_concatenate_poses(rig.snapshot_qvec + 4 * (size_t)sn, rig.snapshot_tvec + 3 * (size_t)sn,
                          rig.rel_qvec + 4 * (size_t)k, rig.rel_tvec + 3 * (size_t)k, q, t);
    double* P = proj.data() + 12 * (size_t)i;  // ComposeProjectionMatrix
    unit_quat_matrix(q, P);
    P[9] = t[0]; P[10] = t[1]; P[11] = t[2];
  }
  const double max_sq = rig.max_reproj_error * rig.max_reproj_error;
  rs->obs_skip.assign(N, 0);
  rs->num_filtered = 0;
  std::vector<int64_t> img_kept(I, 0);
  for (int64_t k = 0; k < N; ++k) {
    const int img = p->obs_image[k];
    if (img < 0 || img >= I || p->obs_point[k] < 0 || p->obs_point[k] >= p->num_points)
      return MI_BA_ERR_INVALID_ARGUMENT;
    if (rs->img_snapshot[img] < 0 || !in_cfg(img)) continue;
    // CalculateSquaredReprojectionError with the projection matrix (projection.cc:130-150)
    const double* P = proj.data() + 12 * (size_t)img;
    const double* X = p->xyz + 3 * (size_t)p->obs_point[k];
    const double pz = P[6] * X[0] + P[7] * X[1] + P[8] * X[2] + P[11];
    double sq = std::numeric_limits<double>::max();
    if (!(pz < std::numeric_limits<double>::epsilon())) {
      const double px = P[0] * X[0] + P[1] * X[1] + P[2] * X[2] + P[9];
      const double py = P[3] * X[0] + P[4] * X[1] + P[5] * X[2] + P[10];
      const double inv = 1.0 / pz;
      const int cam = p->image_camera[img];
      double x = 0, y = 0;
      world_to_image_all(problem_camera_model(p, cam), p->camera_params + cam_off[cam], inv * px, inv * py, &x, &y);
      const double dx = x - p->obs_xy[2 * k], dy = y - p->obs_xy[2 * k + 1];
      sq = dx * dx + dy * dy;
    }
    if (sq > max_sq) {
      rs->obs_skip[k] = 1;
      rs->num_filtered += 1;
    } else {
      img_kept[img] += 1;
    }
  }
  const mi_ba_status st = build_setup(o, p, s, rs->obs_skip.data(), true);
  if (st != MI_BA_OK) return st;
  // The rig images' poses are no parameter blocks: their blocks hang on the
  // snapshot's rig pose (always variable) and the camera's relative pose
  // (constant for the reference camera or without refine_relative_poses,
  // :1041-1048), 6 tangent dimensions each (QuaternionManifold + tvec).
  rs->snapshot_used.assign(rig.num_snapshots, 0);
  rs->rel_used.assign(ncam, 0);
  rs->rel_var.assign(ncam, 0);
  int64_t ne = s->num_effective_parameters_reduced;
  for (int i = 0; i < I; ++i) {
    if (rs->img_snapshot[i] < 0 || !in_cfg(i) || img_kept[i] == 0) continue;
    ne -= 6;  // counted by build_setup as a free variable pose
    const int sn = rs->img_snapshot[i], k = rs->img_rel[i];
    if (!rs->snapshot_used[sn]) {
      rs->snapshot_used[sn] = 1;
      ne += 6;
    }
    rs->rel_used[k] = 1;
    const bool var = rig.refine_relative_poses && p->image_camera[i] != rig.rig_ref_camera[rs->img_rig[i]];
    if (var && !rs->rel_var[k]) {
      rs->rel_var[k] = 1;
      ne += 6;
    }
  }
  s->num_effective_parameters_reduced = ne;
  return MI_BA_OK;
}

}  // namespace miba
