"""numpy restatement of EstimateAbsolutePose (src/estimators/pose.cc:50-158):
P3PEstimator and EPNPEstimator (src/estimators/absolute_pose.cc), the LO-RANSAC
of src/optim/loransac.h:88-249 and RANSAC::ComputeNumTrials line by line, with
numpy.roots for the quartic and numpy.linalg.svd / lstsq where the reference
uses Eigen's decompositions.  It shares no code with
csrc/absolute_pose_block.h.

Two build decisions are restated as the library documents them (mi_ba.h): the
counter-based sampler (there is no reference stream to equal) and the order of
a trial's models, ascending in the root x; so is the orientation of EPnP's
principal axes (the component of the largest magnitude positive), on which the
returned pose depends at the level of the noise.  Camera::ImageToWorld is the
library's host function (mi_ba.image_to_world), which has its own tests."""
import math
from dataclasses import dataclass

import numpy as np

import mi_ba

DBL_MAX = float(np.finfo(np.float64).max)
EPS = float(np.finfo(np.float64).eps)
MAX_TRIALS = 2 ** 63 - 1
MASK64 = (1 << 64) - 1
TWO_FOCALS = (1, 4, 5, 7)  # PINHOLE, OPENCV, OPENCV_FISHEYE, FOV (Camera::FocalLengthIdxs)


@dataclass
class Options:
    """RANSACOptions and the sampler's seed."""
    max_error: float
    min_inlier_ratio: float = 0.1
    confidence: float = 0.99
    dyn_num_trials_multiplier: float = 3.0
    min_num_trials: int = 0
    max_num_trials: int = MAX_TRIALS
    seed: int = 0


# ---------------------------------------------------------------- the sampler
def mix64(z):
    z = (z + 0x9E3779B97F4A7C15) & MASK64
    z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & MASK64
    z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & MASK64
    return z ^ (z >> 31)


def sample(seed, t, n):
    """Trial t: the first three steps of a Fisher-Yates shuffle of range(n)."""
    h = mix64(mix64(seed & MASK64) ^ t)
    perm = {}
    out = []
    for i in range(3):
        j = i + ((mix64(h ^ i) * (n - i)) >> 64)
        pi, pj = perm.get(i, i), perm.get(j, j)
        perm[i], perm[j] = pj, pi
        out.append(pj)
    return out


# ---------------------------------------------------------------- residuals, support
def squared_errors(x2, X3, P):
    """ComputeSquaredReprojectionError (estimators/utils.cc:133-185)."""
    out = np.full(len(x2), DBL_MAX)
    for i in range(len(x2)):
        X = X3[i]
        pz = P[2, 0] * X[0] + P[2, 1] * X[1] + P[2, 2] * X[2] + P[2, 3]
        if pz > EPS:
            px = P[0, 0] * X[0] + P[0, 1] * X[1] + P[0, 2] * X[2] + P[0, 3]
            py = P[1, 0] * X[0] + P[1, 1] * X[1] + P[1, 2] * X[2] + P[1, 3]
            inv = 1.0 / pz
            dx, dy = x2[i, 0] - px * inv, x2[i, 1] - py * inv
            out[i] = dx * dx + dy * dy
    return out


def evaluate_support(res, max_residual):
    n, s = 0, 0.0
    for r in res:
        if r <= max_residual:
            n += 1
            s += r
    return n, s


def better(a, b):
    return a[0] > b[0] or (a[0] == b[0] and a[1] < b[1])


def compute_num_trials(num_inliers, num_samples, confidence, multiplier):
    """kMinNumSamples = 3; the cube is written r * r * r as in the library."""
    r = num_inliers / float(num_samples)
    nom = 1 - confidence
    if nom <= 0:
        return MAX_TRIALS
    denom = 1 - r * r * r
    if denom <= 0:
        return 1
    if denom == 1.0:
        return MAX_TRIALS
    x = math.ceil(math.log(nom) / math.log(denom) * multiplier)
    return MAX_TRIALS if not 0 <= x < 9.2e18 else int(x)


# ---------------------------------------------------------------- P3P
def lift(p):
    return np.array([p[0], p[1], 1.0]) / math.sqrt(p[0] * p[0] + p[1] * p[1] + 1)


def umeyama(src, dst):
    """Eigen::umeyama(src, dst, false) for points in columns: the 3 x 4 [R | t]."""
    sm, dm = src.mean(axis=1), dst.mean(axis=1)
    sigma = (dst - dm[:, None]) @ (src - sm[:, None]).T / src.shape[1]
    U, _, Vt = np.linalg.svd(sigma)
    S = np.ones(3)
    if np.linalg.det(U) * np.linalg.det(Vt) < 0:
        S[2] = -1
    R = U @ np.diag(S) @ Vt
    return np.concatenate([R, (dm - R @ sm)[:, None]], axis=1)


def p3p(x2, X3):
    """P3PEstimator::Estimate (absolute_pose.cc:47-174); models ascending in x."""
    u, v, w = lift(x2[0]), lift(x2[1]), lift(x2[2])
    cos_uv, cos_uw, cos_vw = u @ v, u @ w, v @ w
    dAB2 = ((X3[0] - X3[1]) ** 2).sum()
    dAC2 = ((X3[0] - X3[2]) ** 2).sum()
    dBC2 = ((X3[1] - X3[2]) ** 2).sum()
    dAB = math.sqrt(dAB2)
    with np.errstate(all="ignore"):
        a, b = np.float64(dBC2) / np.float64(dAB2), np.float64(dAC2) / np.float64(dAB2)
        a2, b2 = a * a, b * b
        p, q, r = 2 * cos_vw, 2 * cos_uw, 2 * cos_uv
        p2, q2, r2 = p * p, q * q, r * r
        p3, r3 = p2 * p, r2 * r
        r4 = r3 * r
        r5 = r4 * r
        c = [-2 * b + b2 + a2 + 1 + a * b * (2 - r2) - 2 * a,
             -2 * q * a2 - r * p * b2 + 4 * q * a + (2 * q + p * r) * b + (r2 * q - 2 * q + r * p) * a * b - 2 * q,
             (2 + q2) * a2 + (p2 + r2 - 2) * b2 - (4 + 2 * q2) * a - (p * q * r + p2) * b - (p * q * r + r2) * a * b
             + q2 + 2,
             -2 * q * a2 - r * p * b2 + 4 * q * a + (p * r + q * p2 - 2 * q) * b + (r * p + 2 * q) * a * b - 2 * q,
             a2 + b2 - 2 * a + (2 - p2) * b - 2 * a * b + 1]
        if not np.all(np.isfinite(c)) or c[0] == 0:
            return []
        roots = np.roots(c)
        xs = sorted(float(z.real) for z in roots if abs(z.imag) <= 1e-10 and z.real >= 0)
        models = []
        for x in xs:
            x2_, x3 = x * x, x * x * x
            bb1 = (p2 - p * q * r + r2) * a + (p2 - r2) * b - p2 + p * q * r - r2
            b1 = b * bb1 * bb1
            b0 = ((1 - a - b) * x2_ + (a - 1) * q * x - a + b + 1) * (
                r3 * (a2 + b2 - 2 * a - 2 * b + (2 - r2) * a * b + 1) * x3 +
                r2 * (p + p * a2 - 2 * r * q * a * b + 2 * r * q * b - 2 * r * q - 2 * p * a - 2 * p * b + p * r2 * b +
                      4 * r * q * a + q * r3 * a * b - 2 * r * q * a2 + 2 * p * a * b + p * b2 - r2 * p * b2) * x2_ +
                (r5 * (b2 - a * b) - r4 * p * q * b +
                 r3 * (q2 - 4 * a - 2 * q2 * a + q2 * a2 + 2 * a2 - 2 * b2 + 2) +
                 r2 * (4 * p * q * a - 2 * p * q * a * b + 2 * p * q * b - 2 * p * q - 2 * p * q * a2) +
                 r * (p2 * b2 - 2 * p2 * b + 2 * p2 * a * b - 2 * p2 * a + p2 + p2 * a2)) * x +
                (2 * p * r2 - 2 * r3 * q + p3 - 2 * p2 * q * r + p * q2 * r2) * a2 + (p3 - 2 * p * r2) * b2 +
                (4 * q * r3 - 4 * p * r2 - 2 * p3 + 4 * p2 * q * r - 2 * p * q2 * r2) * a +
                (-2 * q * r3 + p * r4 + 2 * p2 * q * r - 2 * p3) * b + (2 * p3 + 2 * q * r3 - 2 * p2 * q * r) * a * b +
                p * q2 * r2 - 2 * p2 * q * r + 2 * p * r2 + p3 - 2 * r3 * q)
            y = np.float64(b0) / np.float64(b1)
            nu = x2_ + y * y - 2 * x * y * cos_uv
            dPC = dAB / np.sqrt(np.float64(nu))
            cam = np.stack([u * (x * dPC), v * (y * dPC), w * dPC], axis=1)
            if not np.all(np.isfinite(cam)):
                models.append(np.full((3, 4), np.nan))
                continue
            models.append(umeyama(np.asarray(X3, np.float64).T, cam))
    return models


# ---------------------------------------------------------------- EPnP
def epnp(x2, X3):
    """EPNPEstimator::Estimate (absolute_pose.cc:183-609): [] or [P]."""
    x2, X3 = np.asarray(x2, np.float64), np.asarray(X3, np.float64)
    n = len(X3)
    with np.errstate(all="ignore"):
        # ChooseControlPoints
        cws = np.zeros((4, 3))
        cws[0] = X3.sum(axis=0) / n
        PW0 = X3 - cws[0]
        U, D, _ = np.linalg.svd(PW0.T @ PW0)
        for i in range(1, 4):
            axis = U[:, i - 1]
            if axis[np.argmax(np.abs(axis))] < 0:  # the library's documented orientation of an axis
                axis = -axis
            cws[i] = cws[0] + math.sqrt(D[i - 1] / n) * axis
        # ComputeBarycentricCoordinates
        CC = (cws[1:] - cws[0]).T
        if np.linalg.matrix_rank(CC) < 3:
            return []
        CCi = np.linalg.inv(CC)
        al = np.zeros((n, 4))
        al[:, 1:] = (X3 - cws[0]) @ CCi.T
        al[:, 0] = 1.0 - al[:, 1] - al[:, 2] - al[:, 3]
        # ComputeM
        Mm = np.zeros((2 * n, 12))
        for j in range(4):
            Mm[0::2, 3 * j] = al[:, j]
            Mm[0::2, 3 * j + 2] = -al[:, j] * x2[:, 0]
            Mm[1::2, 3 * j + 1] = al[:, j]
            Mm[1::2, 3 * j + 2] = -al[:, j] * x2[:, 1]
        Uu, _, _ = np.linalg.svd(Mm.T @ Mm)
        Ut = Uu.T
        # ComputeL6x10, ComputeRho
        pairs = [(0, 1), (0, 2), (0, 3), (1, 2), (1, 3), (2, 3)]
        dv = np.array([[Ut[11 - i, 3 * a:3 * a + 3] - Ut[11 - i, 3 * b:3 * b + 3] for a, b in pairs] for i in range(4)])
        L = np.zeros((6, 10))
        for i in range(6):
            d = dv[:, i]
            L[i] = [d[0] @ d[0], 2 * d[0] @ d[1], d[1] @ d[1], 2 * d[0] @ d[2], 2 * d[1] @ d[2], d[2] @ d[2],
                    2 * d[0] @ d[3], 2 * d[1] @ d[3], 2 * d[2] @ d[3], d[3] @ d[3]]
        rho = np.array([((cws[a] - cws[b]) ** 2).sum() for a, b in pairs])
        if not (np.all(np.isfinite(L)) and np.all(np.isfinite(rho))):
            return [np.full((3, 4), np.nan)]

        def solve(A, b):
            return np.linalg.lstsq(A, b, rcond=None)[0]

        def approx1():
            b4 = solve(L[:, [0, 1, 3, 6]], rho)
            b0 = math.sqrt(-b4[0]) if b4[0] < 0 else math.sqrt(b4[0])
            s = -1.0 if b4[0] < 0 else 1.0
            return np.array([b0, s * b4[1] / b0, s * b4[2] / b0, s * b4[3] / b0])

        def approx23(cols):
            b = solve(L[:, :cols], rho)
            if b[0] < 0:
                b0, b1 = math.sqrt(-b[0]), (math.sqrt(-b[2]) if b[2] < 0 else 0.0)
            else:
                b0, b1 = math.sqrt(b[0]), (math.sqrt(b[2]) if b[2] > 0 else 0.0)
            if b[1] < 0:
                b0 = -b0
            return np.array([b0, b1, b[3] / b0 if cols == 5 else 0.0, 0.0])

        def gauss_newton(be):
            be = be.copy()
            for _ in range(5):
                if not np.all(np.isfinite(be)):
                    return be
                A = np.stack([2 * L[:, 0] * be[0] + L[:, 1] * be[1] + L[:, 3] * be[2] + L[:, 6] * be[3],
                              L[:, 1] * be[0] + 2 * L[:, 2] * be[1] + L[:, 4] * be[2] + L[:, 7] * be[3],
                              L[:, 3] * be[0] + L[:, 4] * be[1] + 2 * L[:, 5] * be[2] + L[:, 8] * be[3],
                              L[:, 6] * be[0] + L[:, 7] * be[1] + L[:, 8] * be[2] + 2 * L[:, 9] * be[3]], axis=1)
                bb = rho - (L[:, 0] * be[0] * be[0] + L[:, 1] * be[0] * be[1] + L[:, 2] * be[1] * be[1] +
                            L[:, 3] * be[0] * be[2] + L[:, 4] * be[1] * be[2] + L[:, 5] * be[2] * be[2] +
                            L[:, 6] * be[0] * be[3] + L[:, 7] * be[1] * be[3] + L[:, 8] * be[2] * be[3] +
                            L[:, 9] * be[3] * be[3])
                be = be + solve(A, bb)
            return be

        def compute_rt(be):
            if not np.all(np.isfinite(be)):
                return np.full((3, 4), np.nan), math.inf
            ccs = sum(be[i] * Ut[11 - i].reshape(4, 3) for i in range(4))
            pcs = al @ ccs
            if pcs[0, 2] < 0.0:  # SolveForSign
                ccs, pcs = -ccs, -pcs
            pc0, pw0 = pcs.sum(axis=0) / n, X3.sum(axis=0) / n
            abt = (pcs - pc0).T @ (X3 - pw0)
            if not np.all(np.isfinite(abt)):
                return np.full((3, 4), np.nan), math.inf
            aU, _, aVt = np.linalg.svd(abt)
            R = aU @ aVt
            if np.linalg.det(R) < 0:
                aVt[2] = -aVt[2]
                R = aU @ aVt
            P = np.concatenate([R, (pc0 - R @ pw0)[:, None]], axis=1)
            return P, float(np.sqrt(squared_errors(x2, X3, P)).sum())

        best, best_err = None, None
        for be in (approx1(), approx23(3), approx23(5)):
            P, err = compute_rt(gauss_newton(be))
            if best is None or err < best_err:
                best, best_err = P, err
        return [best]


# ---------------------------------------------------------------- LO-RANSAC
def loransac(o: Options, x2, X3):
    """LORANSAC<P3PEstimator, EPNPEstimator>::Estimate on normalised points:
    dict(success, P, mask, num_trials, num_inliers, best_is_local)."""
    x2, X3 = np.asarray(x2, np.float64).reshape(-1, 2), np.asarray(X3, np.float64).reshape(-1, 3)
    n = len(x2)
    out = dict(success=False, P=None, mask=None, num_trials=0, num_inliers=0, best_is_local=False)
    if n < 3:
        return out
    max_num_trials = min(o.max_num_trials, compute_num_trials(int(o.min_inlier_ratio * 100000), 100000, o.confidence,
                                                              o.dyn_num_trials_multiplier))
    best_support, best_model, best_is_local = (0, DBL_MAX), None, False
    abort = False
    max_residual = o.max_error * o.max_error
    res, best_local_res = None, None
    dyn = max_num_trials
    num_trials = 0
    while num_trials < max_num_trials:
        if abort:
            num_trials += 1
            break
        idx = sample(o.seed, num_trials, n)
        for model in p3p(x2[idx], X3[idx]):
            res = squared_errors(x2, X3, model)
            support = evaluate_support(res, max_residual)
            if better(support, best_support):
                best_support, best_model, best_is_local = support, model, False
                if support[0] > 3 and support[0] >= 4:
                    for _ in range(10):
                        inl = [i for i in range(n) if res[i] <= max_residual]
                        local_models = epnp(x2[inl], X3[inl])
                        prev = best_support[0]
                        for local in local_models:
                            res = squared_errors(x2, X3, local)
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
    out.update(num_trials=num_trials, num_inliers=best_support[0], best_is_local=best_is_local)
    if best_support[0] < 3:
        return out
    out.update(success=True, P=np.array(best_model), mask=squared_errors(x2, X3, best_model) <= max_residual)
    return out


# ---------------------------------------------------------------- EstimateAbsolutePose
def scaled_params(model, params, factor):
    prm = np.array(params, np.float64)
    prm[0] *= factor
    if model in TWO_FOCALS:
        prm[1] *= factor
    return prm


def estimate_kernel(o: Options, model, params, factor, points2D, points3D):
    """EstimateAbsolutePoseKernel (pose.cc:50-75)."""
    prm = scaled_params(model, params, factor)
    mean_focal = (prm[0] + prm[1]) / 2.0 if model in TWO_FOCALS else prm[0]
    x2 = np.array([mi_ba.image_to_world(model, prm, x, y) for x, y in np.asarray(points2D, np.float64).reshape(-1, 2)])
    oo = Options(**{**o.__dict__, "max_error": o.max_error / mean_focal})
    out = loransac(oo, x2.reshape(-1, 2), points3D)
    # pose.cc:150-155
    if out["success"]:
        out["qvec"] = rotation_to_quaternion(out["P"][:, :3])
        out["tvec"] = out["P"][:, 3].copy()
        if np.isnan(out["qvec"]).any() or np.isnan(out["tvec"]).any():
            out["success"] = False
    return out


def rotation_to_quaternion(R):
    """Eigen::Quaterniond(R) as (w, x, y, z)."""
    t = R[0, 0] + R[1, 1] + R[2, 2]
    q = np.zeros(4)
    if t > 0:
        t = math.sqrt(t + 1.0)
        q[0] = 0.5 * t
        t = 0.5 / t
        q[1:] = [(R[2, 1] - R[1, 2]) * t, (R[0, 2] - R[2, 0]) * t, (R[1, 0] - R[0, 1]) * t]
    else:
        i = 0
        if R[1, 1] > R[0, 0]:
            i = 1
        if R[2, 2] > R[i, i]:
            i = 2
        j, k = (i + 1) % 3, (i + 2) % 3
        t = math.sqrt(R[i, i] - R[j, j] - R[k, k] + 1.0)
        q[1 + i] = 0.5 * t
        t = 0.5 / t
        q[0] = (R[k, j] - R[j, k]) * t
        q[1 + j] = (R[j, i] + R[i, j]) * t
        q[1 + k] = (R[k, i] + R[i, k]) * t
    return q


def focal_length_factors(num_samples, min_ratio, max_ratio):
    """The sweep's loop (pose.cc:91-98) verbatim: its trip count is decided by rounding."""
    out = []
    fstep = 1.0 / num_samples
    fscale = max_ratio - min_ratio
    f = 0.0
    while f <= 1.0:
        out.append(min_ratio + fscale * f * f)
        f += fstep
    return out


def estimate_absolute_pose(o: Options, model, params, points2D, points3D, estimate_focal_length=False,
                           num_focal_length_samples=30, min_focal_length_ratio=0.2, max_focal_length_ratio=5.0):
    """EstimateAbsolutePose (pose.cc:79-158): dict(success, factor, num_inliers, mask, P, params)."""
    factors = (focal_length_factors(num_focal_length_samples, min_focal_length_ratio, max_focal_length_ratio)
               if estimate_focal_length else [1.0])
    best = dict(success=False, factor=0.0, num_inliers=0, mask=None, P=None, params=np.array(params, np.float64))
    for f in factors:
        r = estimate_kernel(o, model, params, f, points2D, points3D)
        if r["success"] and r["num_inliers"] > best["num_inliers"]:
            best.update(num_inliers=r["num_inliers"], P=r["P"], mask=r["mask"], factor=f)
    if best["num_inliers"] == 0:
        return best
    if estimate_focal_length:
        best["params"] = scaled_params(model, params, best["factor"])
    q = rotation_to_quaternion(best["P"][:, :3])
    best["success"] = not (np.isnan(q).any() or np.isnan(best["P"][:, 3]).any())
    return best


def discrete(out):
    """The outputs that must agree exactly."""
    return (bool(out["success"]), int(out["num_trials"]), bool(out["best_is_local"]), int(out["num_inliers"]),
            None if not out["success"] else tuple(bool(b) for b in out["mask"]))
