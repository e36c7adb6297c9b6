"""numpy restatement of the reference's robust triangulation, independent of
csrc/triangulation_block.h (numpy.linalg.svd and eigh, not Jacobi sweeps):

    TriangulatePoint, TriangulateMultiViewPoint, CalculateTriangulationAngle
                                      src/base/triangulation.cc:39-53, 72-89, 122-145
    HasPointPositiveDepth, CalculateNormalizedAngularError and
    CalculateSquaredReprojectionError (projection-matrix overloads)
                                      src/base/projection.cc:130-149, 177-195
    TriangulationEstimator::Estimate / Residuals
                                      src/estimators/triangulation.cc:55-130
    RANSAC::ComputeNumTrials and the constructor's cap
                                      src/optim/ransac.h:143-180
    InlierSupportMeasurer             src/optim/support_measurement.cc:36-60
    LORANSAC::Estimate                src/optim/loransac.h:88-249, statement by
                                      statement, its two residual buffers and
                                      their swaps included
    CombinationSampler                src/optim/combination_sampler.cc: the pairs
                                      in lexicographic order

Eigen is not available here, so the reference's own sources cannot be compiled;
this file is the semantic oracle of the triangulation tests.  size_t's maximum
is MAX_TRIALS = 2**63 - 1, as in the C interface."""
import itertools
import math
from dataclasses import dataclass, field

import numpy as np

import camera_model_ref as cref

EPS = float(np.finfo(np.float64).eps)
DBL_MAX = float(np.finfo(np.float64).max)
MAX_TRIALS = 2 ** 63 - 1
ANGULAR, REPROJECTION = 0, 1


@dataclass
class Track:
    """PointData and PoseData of one track."""
    proj: np.ndarray                 # [n][3][4]
    centers: np.ndarray              # [n][3]
    normalized: np.ndarray           # [n][2] point_normalized
    points: np.ndarray               # [n][2] pixels
    camera: np.ndarray               # [n] index into cameras
    cameras: list = field(default_factory=list)  # (model id, parameters)

    def __len__(self):
        return len(self.proj)


@dataclass
class Options:
    max_error: float
    min_tri_angle: float = 0.0
    residual_type: int = ANGULAR
    min_inlier_ratio: float = 0.1
    confidence: float = 0.99
    dyn_num_trials_multiplier: float = 3.0
    min_num_trials: int = 0
    max_num_trials: int = MAX_TRIALS


def _acos(x):
    return math.acos(x) if -1.0 <= x <= 1.0 else float("nan")


def hnormalized(v):
    return v[:3] / v[3]


def triangulate_point(P1, P2, x1, x2):
    A = np.stack([x1[0] * P1[2] - P1[0], x1[1] * P1[2] - P1[1], x2[0] * P2[2] - P2[0], x2[1] * P2[2] - P2[1]])
    return hnormalized(np.linalg.svd(A)[2][3])


def triangulate_multi_view_point(Ps, xs):
    A = np.zeros((4, 4))
    for P, x in zip(Ps, xs):
        p = np.array([x[0], x[1], 1.0])
        p = p / np.linalg.norm(p)
        term = P - np.outer(p, p) @ P
        A += term.T @ term
    return hnormalized(np.linalg.eigh(A)[1][:, 0])


def triangulation_angle(c1, c2, X):
    b2 = float((c1 - c2) @ (c1 - c2))
    r1 = float((X - c1) @ (X - c1))
    r2 = float((X - c2) @ (X - c2))
    den = 2.0 * math.sqrt(r1 * r2)
    if den == 0.0:
        return 0.0
    angle = abs(_acos((r1 + r2 - b2) / den))
    other = math.pi - angle
    return other if other < angle else angle


def has_positive_depth(P, X):
    return float(P[2] @ np.append(X, 1.0)) >= EPS


def normalized_angular_error(x, X, P):
    ray1 = np.array([x[0], x[1], 1.0])
    ray2 = P @ np.append(X, 1.0)
    n2 = np.linalg.norm(ray2)
    if n2 > 0:
        ray2 = ray2 / n2
    return _acos(float((ray1 / np.linalg.norm(ray1)) @ ray2))


def squared_reprojection_error(point, X, P, camera):
    Xh = np.append(X, 1.0)
    z = float(P[2] @ Xh)
    if z < EPS:
        return DBL_MAX
    inv = 1.0 / z
    u, v = cref.world_to_image(camera[0], camera[1], inv * float(P[0] @ Xh), inv * float(P[1] @ Xh))
    return (float(u[0]) - point[0]) ** 2 + (float(v[0]) - point[1]) ** 2


def estimate(track, idx, min_tri_angle):
    """TriangulationEstimator::Estimate on the observations idx: [] or [xyz]."""
    if len(idx) == 2:
        i, j = idx
        X = triangulate_point(track.proj[i], track.proj[j], track.normalized[i], track.normalized[j])
        if (has_positive_depth(track.proj[i], X) and has_positive_depth(track.proj[j], X)
                and triangulation_angle(track.centers[i], track.centers[j], X) >= min_tri_angle):
            return [X]
        return []
    X = triangulate_multi_view_point(track.proj[idx], track.normalized[idx])
    for i in idx:
        if not has_positive_depth(track.proj[i], X):
            return []
    for a in range(len(idx)):
        for b in range(a):
            if triangulation_angle(track.centers[idx[a]], track.centers[idx[b]], X) >= min_tri_angle:
                return [X]
    return []


def residuals(track, X, residual_type):
    out = np.empty(len(track))
    for i in range(len(track)):
        if residual_type == REPROJECTION:
            out[i] = squared_reprojection_error(track.points[i], X, track.proj[i], track.cameras[track.camera[i]])
        else:
            e = normalized_angular_error(track.normalized[i], X, track.proj[i])
            out[i] = e * e
    return out


def compute_num_trials(num_inliers, num_samples, confidence, multiplier):
    inlier_ratio = num_inliers / float(num_samples)
    nom = 1 - confidence
    if nom <= 0:
        return MAX_TRIALS
    denom = 1 - inlier_ratio ** 2
    if denom <= 0:
        return 1
    if denom == 1.0:
        return MAX_TRIALS
    x = math.ceil(math.log(nom) / math.log(denom) * multiplier)
    return MAX_TRIALS if not 0 <= x < 9.2e18 else int(x)


def evaluate_support(res, max_residual):
    n, s = 0, 0.0
    for r in res:
        if r <= max_residual:
            n += 1
            s += r
    return n, s


def better(a, b):
    return a[0] > b[0] or (a[0] == b[0] and a[1] < b[1])


def estimate_triangulation(o: Options, track: Track):
    """EstimateTriangulation: dict(success, xyz, mask, num_trials, num_inliers,
    best_is_local, local_recursions)."""
    # RANSAC's constructor
    max_num_trials = min(o.max_num_trials, compute_num_trials(int(o.min_inlier_ratio * 100000), 100000, o.confidence,
                                                              o.dyn_num_trials_multiplier))
    n = len(track)
    best_support, best_model, best_is_local = (0, DBL_MAX), None, False
    abort = False
    max_residual = o.max_error * o.max_error
    res, best_local_res = None, None
    pairs = itertools.combinations(range(n), 2)  # lexicographic, as NextCombination
    max_num_trials = min(max_num_trials, n * (n - 1) // 2)
    dyn = max_num_trials
    num_trials, recursions = 0, 0
    while num_trials < max_num_trials:
        if abort:
            num_trials += 1
            break
        sample = list(next(pairs))
        for model in estimate(track, sample, o.min_tri_angle):
            res = residuals(track, model, o.residual_type)
            support = evaluate_support(res, max_residual)
            if better(support, best_support):
                best_support, best_model, best_is_local = support, model, False
                if support[0] > 2:
                    for _ in range(10):
                        inl = [i for i in range(n) if res[i] <= max_residual]
                        local_models = estimate(track, inl, o.min_tri_angle)
                        prev = best_support[0]
                        for local in local_models:
                            recursions += 1
                            res = residuals(track, local, o.residual_type)
                            local_support = evaluate_support(res, max_residual)
                            if better(local_support, best_support):
                                best_support, best_model, best_is_local = local_support, local, True
                                res, best_local_res = best_local_res, res
                        if best_support[0] <= prev:
                            break
                        res, best_local_res = best_local_res, res
                dyn = compute_num_trials(best_support[0], n, o.confidence, o.dyn_num_trials_multiplier)
            if num_trials >= dyn and num_trials >= o.min_num_trials:
                abort = True
                break
        num_trials += 1
    out = dict(success=best_support[0] >= 2, xyz=None, mask=None, num_trials=num_trials, num_inliers=best_support[0],
               best_is_local=best_is_local, local_recursions=recursions)
    if out["success"]:
        out["xyz"] = np.array(best_model)
        out["mask"] = residuals(track, best_model, o.residual_type) <= max_residual
    return out


def discrete(out):
    """The outputs that must agree exactly."""
    return (bool(out["success"]), int(out["num_trials"]), bool(out["best_is_local"]), int(out["num_inliers"]),
            None if out["mask"] is None else tuple(bool(m) for m in out["mask"]))
