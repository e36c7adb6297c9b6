// colmap_amd/camera_rig.h — CameraRig and RigBundleAdjuster with the
// reference's API (src/base/camera_rig.{h,cc}, src/optim/bundle_adjustment.h:
// 270-327, bundle_adjustment.cc:789-1140), routed to mi_ba_rig_solve.
//
//   colmap::CameraRig          -> colmap_amd::CameraRig
//   colmap::RigBundleAdjuster  -> colmap_amd::RigBundleAdjuster
//
// Not restated (rig calibration from a reconstruction): CameraRig::
// ComputeRelativePoses / ComputeScale.  Error convention as
// bundle_adjustment.h: where the reference CHECKs, std::invalid_argument.
#pragma once

#include <array>
#include <cmath>
#include <limits>
#include <map>
#include <stdexcept>
#include <unordered_map>
#include <unordered_set>
#include <vector>

#include "bundle_adjustment.h"

namespace colmap_amd {

namespace internal {

inline void NormalizeQuat(const double q[4], double out[4]) {  // NormalizeQuaternion (pose.cc:82-91)
  const double n = std::sqrt(q[0] * q[0] + q[1] * q[1] + q[2] * q[2] + q[3] * q[3]);
  if (n == 0) {
    out[0] = 1.0; out[1] = q[1]; out[2] = q[2]; out[3] = q[3];
  } else {
    for (int k = 0; k < 4; ++k) out[k] = q[k] / n;
  }
}

// ConcatenateQuaternions(q1, q2) (pose.cc:97-108): normalised q2 * q1.
inline void ConcatenateQuats(const double q1[4], const double q2[4], double out[4]) {
  double a[4], b[4], c[4];
  NormalizeQuat(q1, a);
  NormalizeQuat(q2, b);
  c[0] = b[0] * a[0] - b[1] * a[1] - b[2] * a[2] - b[3] * a[3];
  c[1] = b[0] * a[1] + b[1] * a[0] + b[2] * a[3] - b[3] * a[2];
  c[2] = b[0] * a[2] + b[2] * a[0] + b[3] * a[1] - b[1] * a[3];
  c[3] = b[0] * a[3] + b[3] * a[0] + b[1] * a[2] - b[2] * a[1];
  NormalizeQuat(c, out);
}

// QuaternionRotatePoint (pose.cc:110-116): rotation by the normalised q.
inline void RotatePoint(const double q[4], const double p[3], double out[3]) {
  double n[4];
  NormalizeQuat(q, n);
  const double w = n[0], x = n[1], y = n[2], z = n[3];
  const double R[9] = {1 - 2 * (y * y + z * z), 2 * (x * y - w * z),     2 * (x * z + w * y),
                       2 * (x * y + w * z),     1 - 2 * (x * x + z * z), 2 * (y * z - w * x),
                       2 * (x * z - w * y),     2 * (y * z + w * x),     1 - 2 * (x * x + y * y)};
  for (int r = 0; r < 3; ++r) out[r] = R[3 * r] * p[0] + R[3 * r + 1] * p[1] + R[3 * r + 2] * p[2];
}

// AverageQuaternions (pose.cc:118-143): the eigenvector of the largest
// eigenvalue of sum w q q^T / sum w (cyclic Jacobi on the 4 x 4 symmetric
// matrix).  An eigenvector's sign is free; it is taken towards the first
// quaternion.
inline void AverageQuats(const std::vector<std::array<double, 4>>& qs, const std::vector<double>& ws, double out[4]) {
  if (qs.empty() || qs.size() != ws.size()) throw std::invalid_argument("AverageQuaternions: sizes");
  if (qs.size() == 1) {
    for (int k = 0; k < 4; ++k) out[k] = qs[0][k];
    return;
  }
  double A[4][4] = {}, V[4][4] = {}, wsum = 0;
  for (size_t i = 0; i < qs.size(); ++i) {
    if (!(ws[i] > 0)) throw std::invalid_argument("AverageQuaternions: weight");
    double q[4];
    NormalizeQuat(qs[i].data(), q);
    for (int r = 0; r < 4; ++r)
      for (int c = 0; c < 4; ++c) A[r][c] += ws[i] * q[r] * q[c];
    wsum += ws[i];
  }
  for (int r = 0; r < 4; ++r) {
    V[r][r] = 1.0;
    for (int c = 0; c < 4; ++c) A[r][c] /= wsum;
  }
  for (int sweep = 0; sweep < 64; ++sweep) {
    double off = 0;
    for (int r = 0; r < 4; ++r)
      for (int c = r + 1; c < 4; ++c) off += A[r][c] * A[r][c];
    if (off < 1e-300) break;
    for (int p = 0; p < 4; ++p)
      for (int q = p + 1; q < 4; ++q) {
        if (A[p][q] == 0) continue;
        const double theta = (A[q][q] - A[p][p]) / (2 * A[p][q]);
        const double t = (theta >= 0 ? 1.0 : -1.0) / (std::fabs(theta) + std::sqrt(theta * theta + 1));
        const double c = 1 / std::sqrt(t * t + 1), s = t * c;
        for (int k = 0; k < 4; ++k) {  // A <- A J
          const double akp = A[k][p], akq = A[k][q];
          A[k][p] = c * akp - s * akq;
          A[k][q] = s * akp + c * akq;
        }
        for (int k = 0; k < 4; ++k) {  // A <- J^T A
          const double apk = A[p][k], aqk = A[q][k];
          A[p][k] = c * apk - s * aqk;
          A[q][k] = s * apk + c * aqk;
        }
        for (int k = 0; k < 4; ++k) {
          const double vkp = V[k][p], vkq = V[k][q];
          V[k][p] = c * vkp - s * vkq;
          V[k][q] = s * vkp + c * vkq;
        }
      }
  }
  int best = 0;
  for (int k = 1; k < 4; ++k)
    if (A[k][k] > A[best][best]) best = k;
  double dot = 0, q0[4];
  NormalizeQuat(qs[0].data(), q0);
  for (int k = 0; k < 4; ++k) dot += V[k][best] * q0[k];
  for (int k = 0; k < 4; ++k) out[k] = dot < 0 ? -V[k][best] : V[k][best];
}

}  // namespace internal

// ConcatenatePoses (pose.cc:183-190).
inline void ConcatenatePoses(const double qvec1[4], const double tvec1[3], const double qvec2[4],
                             const double tvec2[3], double qvec12[4], double tvec12[3]) {
  internal::ConcatenateQuats(qvec1, qvec2, qvec12);
  double r[3];
  internal::RotatePoint(qvec2, tvec1, r);
  for (int k = 0; k < 3; ++k) tvec12[k] = tvec2[k] + r[k];
}

// ---------------------------------------------------------------------------
// CameraRig (camera_rig.h:48-130)
// ---------------------------------------------------------------------------
class CameraRig {
 public:
  static constexpr camera_t kInvalidCameraId = std::numeric_limits<camera_t>::max();

  size_t NumCameras() const { return rig_cameras_.size(); }
  size_t NumSnapshots() const { return snapshots_.size(); }
  bool HasCamera(camera_t camera_id) const { return rig_cameras_.count(camera_id) > 0; }
  camera_t RefCameraId() const { return ref_camera_id_; }
  void SetRefCameraId(camera_t camera_id) {
    if (!HasCamera(camera_id)) throw std::invalid_argument("SetRefCameraId: camera is not in the rig");
    ref_camera_id_ = camera_id;
  }
  std::vector<camera_t> GetCameraIds() const {
    std::vector<camera_t> ids;
    for (const auto& c : rig_cameras_) ids.push_back(c.first);
    return ids;
  }
  const std::vector<std::vector<image_t>>& Snapshots() const { return snapshots_; }

  void AddCamera(camera_t camera_id, const double rel_qvec[4], const double rel_tvec[3]) {
    if (HasCamera(camera_id)) throw std::invalid_argument("AddCamera: camera is in the rig already");
    if (NumSnapshots() != 0) throw std::invalid_argument("AddCamera: after a snapshot");
    RigCamera c;
    for (int k = 0; k < 4; ++k) c.rel_qvec[k] = rel_qvec[k];
    for (int k = 0; k < 3; ++k) c.rel_tvec[k] = rel_tvec[k];
    rig_cameras_.emplace(camera_id, c);
  }
  void AddSnapshot(const std::vector<image_t>& image_ids) {
    if (image_ids.empty()) throw std::invalid_argument("AddSnapshot: empty");
    if (image_ids.size() > NumCameras()) throw std::invalid_argument("AddSnapshot: more images than cameras");
    if (std::unordered_set<image_t>(image_ids.begin(), image_ids.end()).size() != image_ids.size())
      throw std::invalid_argument("AddSnapshot: duplicate image");
    snapshots_.push_back(image_ids);
  }

  // CameraRig::Check (camera_rig.cc:86-110)
  void Check(const Reconstruction& reconstruction) const {
    if (!HasCamera(ref_camera_id_)) throw std::invalid_argument("CameraRig: no reference camera");
    for (const auto& c : rig_cameras_)
      if (!reconstruction.cameras.count(c.first)) throw std::invalid_argument("CameraRig: camera does not exist");
    std::unordered_set<image_t> all;
    for (const auto& snapshot : snapshots_) {
      if (snapshot.empty() || snapshot.size() > NumCameras()) throw std::invalid_argument("CameraRig: snapshot size");
      bool has_ref = false;
      for (image_t id : snapshot) {
        if (!reconstruction.images.count(id)) throw std::invalid_argument("CameraRig: image does not exist");
        if (!all.insert(id).second) throw std::invalid_argument("CameraRig: image in two snapshots");
        const camera_t cam = reconstruction.images.at(id).camera_id;
        if (!HasCamera(cam)) throw std::invalid_argument("CameraRig: image's camera is not in the rig");
        has_ref = has_ref || cam == ref_camera_id_;
      }
      if (!has_ref) throw std::invalid_argument("CameraRig: snapshot without the reference camera");
    }
  }

  double* RelativeQvec(camera_t camera_id) { return rig_cameras_.at(camera_id).rel_qvec; }
  const double* RelativeQvec(camera_t camera_id) const { return rig_cameras_.at(camera_id).rel_qvec; }
  double* RelativeTvec(camera_t camera_id) { return rig_cameras_.at(camera_id).rel_tvec; }
  const double* RelativeTvec(camera_t camera_id) const { return rig_cameras_.at(camera_id).rel_tvec; }

  // CameraRig::ComputeAbsolutePose (camera_rig.cc:230-258): the snapshot's
  // images taken back through their relative poses; quaternions averaged
  // (AverageQuaternions), translations averaged.
  void ComputeAbsolutePose(size_t snapshot_idx, const Reconstruction& reconstruction, double abs_qvec[4],
                           double abs_tvec[3]) const {
    const auto& snapshot = snapshots_.at(snapshot_idx);
    std::vector<std::array<double, 4>> qs;
    double tsum[3] = {0, 0, 0};
    for (image_t id : snapshot) {
      const Image& image = reconstruction.images.at(id);
      const double* rq = RelativeQvec(image.camera_id);
      const double* rt = RelativeTvec(image.camera_id);
      double nq[4], inv[4];
      internal::NormalizeQuat(rq, nq);  // InvertQuaternion
      inv[0] = nq[0]; inv[1] = -nq[1]; inv[2] = -nq[2]; inv[3] = -nq[3];
      std::array<double, 4> q;
      internal::ConcatenateQuats(image.qvec, inv, q.data());
      const double d[3] = {image.tvec[0] - rt[0], image.tvec[1] - rt[1], image.tvec[2] - rt[2]};
      double t[3];
      internal::RotatePoint(inv, d, t);
      qs.push_back(q);
      for (int k = 0; k < 3; ++k) tsum[k] += t[k];
    }
    internal::AverageQuats(qs, std::vector<double>(qs.size(), 1.0), abs_qvec);
    for (int k = 0; k < 3; ++k) abs_tvec[k] = tsum[k] / (double)snapshot.size();
  }

 private:
  struct RigCamera {
    double rel_qvec[4] = {1, 0, 0, 0};
    double rel_tvec[3] = {0, 0, 0};
  };
  camera_t ref_camera_id_ = kInvalidCameraId;
  std::map<camera_t, RigCamera> rig_cameras_;
  std::vector<std::vector<image_t>> snapshots_;
};

// ---------------------------------------------------------------------------
// RigBundleAdjuster (bundle_adjustment.h:270-327)
// ---------------------------------------------------------------------------
class RigBundleAdjuster {
 public:
  struct Options {
    bool refine_relative_poses = true;  // whether to optimize the relative poses of the camera rigs
    double max_reproj_error = 1000.0;   // observations beyond it at the rig's pose are not added
  };

  RigBundleAdjuster(const BundleAdjustmentOptions& options, const Options& rig_options,
                    const BundleAdjustmentConfig& config)
      : options_(options), rig_options_(rig_options), config_(config) {
    options_.Check();
  }

  bool Solve(Reconstruction* reconstruction, std::vector<CameraRig>* camera_rigs) {
    if (!reconstruction || !camera_rigs) throw std::invalid_argument("RigBundleAdjuster::Solve: null argument");
    if (used_) throw std::logic_error("Cannot use the same BundleAdjuster multiple times");
    used_ = true;
    for (const CameraRig& rig : *camera_rigs) rig.Check(*reconstruction);
    internal::Flat flat;
    flat.Build(*reconstruction, config_);
    RigArrays a;
    a.Build(*reconstruction, *camera_rigs, flat, rig_options_);
    mi_ba_options o = internal::ToOptions(options_);
    internal::CallbackBridge bridge;
    internal::InstallCallbacks(options_, &bridge, [&] { flat.WriteBack(reconstruction); }, &o);
    mi_ba_summary s;
    const mi_ba_status st = mi_ba_rig_solve(&o, &flat.problem, &a.rig, &s);
    bridge.Rethrow();
    if (st == MI_BA_ERR_NO_RESIDUALS) return false;
    internal::ThrowStatus(st, "RigBundleAdjuster::Solve");
    summary_ = internal::ToSummary(s);
    flat.WriteBack(reconstruction);
    a.WriteBack(camera_rigs);
    return true;
  }

  // Problem-assembly counts without solving (host only).
  mi_ba_setup_info SetUpInfo(const Reconstruction& reconstruction, const std::vector<CameraRig>& camera_rigs) const {
    for (const CameraRig& rig : camera_rigs) rig.Check(reconstruction);
    internal::Flat flat;
    flat.Build(reconstruction, config_);
    RigArrays a;
    a.Build(reconstruction, camera_rigs, flat, rig_options_);
    const mi_ba_options o = internal::ToOptions(options_);
    mi_ba_setup_info info;
    internal::ThrowStatus(mi_ba_rig_setup_stats(&o, &flat.problem, &a.rig, &info), "RigBundleAdjuster::SetUpInfo");
    return info;
  }

  const SolverSummary& Summary() const { return summary_; }

 private:
  // mi_ba_rig over the rigs; the snapshots' poses by ComputeCameraRigPoses
  // (bundle_adjustment.cc:1111-1134).
  struct RigArrays {
    std::vector<int32_t> cam_off{0}, cams, ref, rig_snap_off{0}, snap_off{0}, snap_img;
    std::vector<camera_t> cam_ids;
    std::vector<double> rel_q, rel_t, snap_q, snap_t;
    mi_ba_rig rig{};
    void Build(const Reconstruction& rec, const std::vector<CameraRig>& rigs, const internal::Flat& flat,
               const Options& options) {
      std::unordered_map<camera_t, int32_t> cidx;
      std::unordered_map<image_t, int32_t> iidx;
      for (size_t c = 0; c < flat.cam_ids.size(); ++c) cidx[flat.cam_ids[c]] = (int32_t)c;
      for (size_t i = 0; i < flat.img_ids.size(); ++i) iidx[flat.img_ids[i]] = (int32_t)i;
      for (const CameraRig& r : rigs) {
        for (camera_t id : r.GetCameraIds()) {
          cams.push_back(cidx.at(id));
          cam_ids.push_back(id);
          rel_q.insert(rel_q.end(), r.RelativeQvec(id), r.RelativeQvec(id) + 4);
          rel_t.insert(rel_t.end(), r.RelativeTvec(id), r.RelativeTvec(id) + 3);
        }
        cam_off.push_back((int32_t)cams.size());
        ref.push_back(cidx.at(r.RefCameraId()));
        for (size_t sn = 0; sn < r.NumSnapshots(); ++sn) {
          double q[4], t[3];
          r.ComputeAbsolutePose(sn, rec, q, t);
          snap_q.insert(snap_q.end(), q, q + 4);
          snap_t.insert(snap_t.end(), t, t + 3);
          for (image_t id : r.Snapshots()[sn]) snap_img.push_back(iidx.at(id));
          snap_off.push_back((int32_t)snap_img.size());
        }
        rig_snap_off.push_back((int32_t)snap_off.size() - 1);
      }
      mi_ba_default_rig(&rig);
      rig.num_rigs = (int32_t)rigs.size();
      rig.rig_camera_off = cam_off.data();
      rig.rig_camera = cams.data();
      rig.rig_ref_camera = ref.data();
      rig.rel_qvec = rel_q.data();
      rig.rel_tvec = rel_t.data();
      rig.rig_snapshot_off = rig_snap_off.data();
      rig.num_snapshots = (int32_t)snap_off.size() - 1;
      rig.snapshot_off = snap_off.data();
      rig.snapshot_image = snap_img.data();
      rig.snapshot_qvec = snap_q.data();
      rig.snapshot_tvec = snap_t.data();
      rig.refine_relative_poses = options.refine_relative_poses ? 1 : 0;
      rig.max_reproj_error = options.max_reproj_error;
    }
    void WriteBack(std::vector<CameraRig>* rigs) const {
      size_t k = 0;
      for (CameraRig& r : *rigs)
        for (camera_t id : r.GetCameraIds()) {
          std::copy(rel_q.begin() + 4 * k, rel_q.begin() + 4 * k + 4, r.RelativeQvec(id));
          std::copy(rel_t.begin() + 3 * k, rel_t.begin() + 3 * k + 3, r.RelativeTvec(id));
          ++k;
        }
    }
  };

  BundleAdjustmentOptions options_;
  Options rig_options_;
  BundleAdjustmentConfig config_;
  SolverSummary summary_;
  bool used_ = false;
};

}  // namespace colmap_amd
