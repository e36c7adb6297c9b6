"""Batched robust absolute pose: mi_ba_estimate_absolute_pose_batch
(EstimateAbsolutePose, src/estimators/pose.cc:50-158).

The oracle is tests/absolute_pose_reference.py, a numpy restatement of P3P,
EPnP and the LO-RANSAC (numpy.roots, numpy.linalg.svd / lstsq; it shares no
code with csrc/absolute_pose_block.h).  The sampler is the library's
counter-based one and the models of a trial come in ascending order of the
root x (both documented in mi_ba.h), so the comparison is decision for
decision: success, the inlier mask, num_trials, num_inliers and best_is_local
must be equal.  A problem is excused only if the reference itself changes a
discrete output under inputs moved by one ulp (estimator_testing.ulp_solves),
at most 1 problem in 20 of a test; test_reference_decisions_are_stable checks
on the CPU that the committed seeds stay within that cap.

proj_matrix is compared with the reference's within PROJ_TOL (below).

CPU tests run the host build of the block header (tests/cpp/
absolute_pose_block_test.cc), the numpy reference and the argument checks; GPU
tests the device."""
import ctypes as C
import functools
import json
import os
import subprocess

import numpy as np
import pytest

import absolute_pose_cases as ac
import absolute_pose_reference as aref
import mi_ba
from estimator_testing import CPP

M = mi_ba
INT64_MAX = 2 ** 63 - 1
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "absolute_pose_known_answers.json")

# Largest |proj_matrix (host build) - proj_matrix (numpy reference)| over the
# case list, measured on the CPU by test_host_build_matches_reference (it
# prints the value): 1.4207e-11, on max_trials1, a P3P model that rests on its
# three sample points.  The device may differ from the reference by ten times
# that (FMA-free too, but its local optimisation sums in another order and its
# libm differs).  Not derived from any device output.  The CPU test itself
# allows the host build five times the recorded value: the difference is that
# of numpy.roots and LAPACK's svd against the block header's root finder and
# Jacobi, and another numpy or LAPACK build may order its operations otherwise.
HOST_VS_NUMPY = 1.4207e-11
HOST_TOL = 5 * HOST_VS_NUMPY
PROJ_TOL = 10 * HOST_VS_NUMPY


def pose_waves():
    """kPoseWaves, the problems of one workgroup, read from csrc/pose_common.h."""
    import re
    text = open(os.path.join(M._HERE, "csrc", "pose_common.h")).read()
    tb = int(re.search(r"constexpr int kPoseTB = (\d+);", text).group(1))
    assert "constexpr int kPoseWaves = kPoseTB / 64;" in text
    return tb // 64


def make(target):
    """Builds one target of tests/cpp/absolute_pose.mk; returns its path."""
    subprocess.run(["make", "-C", CPP, "-f", "absolute_pose.mk", target], check=True, capture_output=True)
    return os.path.join(CPP, target)


def run_program(target, *args, timeout=600):
    out = subprocess.run([make(target), *args], capture_output=True, text=True, timeout=timeout)
    print(out.stdout)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "0 failure(s)" in out.stdout
    return out.stdout


def pack(cases):
    """(sets, cameras, problems) of [(Problem, Options)]: one set and one camera per problem."""
    sets = [(p.points2D, p.points3D) for p, _ in cases]
    cameras = [(p.model, p.params) for p, _ in cases]
    problems = [M.AbsolutePoseEstimationProblem(k, k, p.factor, o.seed) for k, (p, o) in enumerate(cases)]
    return sets, cameras, problems


def write_batch(path, sets, cameras, problems, o):
    """The binary form tests/cpp/absolute_pose_block_test.cc reads."""
    a = M._AbsolutePoseEstimationArrays(sets, cameras, problems, ac.device_options(o))
    prm8 = np.zeros((len(a.models), 8))
    for c in range(len(a.models)):
        prm8[c, :a.prm_off[c + 1] - a.prm_off[c]] = a.prm[a.prm_off[c]:a.prm_off[c + 1]]
    with open(path, "wb") as f:
        np.array([a.n, len(sets), int(a.set_off[-1]), len(a.models)], np.int64).tofile(f)
        np.array([o.max_error, o.min_inlier_ratio, o.confidence, o.dyn_num_trials_multiplier], np.float64).tofile(f)
        np.array([o.min_num_trials, o.max_num_trials], np.int64).tofile(f)
        for arr in (a.set_off, a.points2D, a.points3D, a.models, prm8, a.set_index, a.camera_index, a.factor, a.seed):
            np.ascontiguousarray(arr).tofile(f)


def fromhex(ws):
    return np.array([float.fromhex(w) for w in ws])


def host_estimate(cases, tmp_path, target="absolute_pose_block_test"):
    """The host build of the block header on cases of one option_key: result dicts."""
    src, dst = str(tmp_path / "batch.bin"), str(tmp_path / "batch.out")
    write_batch(src, *pack(cases), cases[0][1])
    run_program(target, "estimate", src, dst)
    out = []
    for line in open(dst):
        w = line.split()
        ok = w[0] == "1"
        out.append(dict(success=ok, num_trials=int(w[1]), num_inliers=int(w[2]), best_is_local=w[3] == "1",
                        P=fromhex(w[4:16]).reshape(3, 4) if ok else None,
                        qvec=fromhex(w[16:20]) if ok else None, tvec=fromhex(w[20:23]) if ok else None,
                        mask=np.array([c == "1" for c in (w[23] if len(w) > 23 else "")]) if ok else None))
    return out


def device_estimate(cases):
    """The device on cases of one option_key: result dicts."""
    r = M.estimate_absolute_pose_batch(ac.device_options(cases[0][1]), *pack(cases))
    return [dict(success=bool(r.success[k]), num_trials=int(r.num_trials[k]), num_inliers=int(r.num_inliers[k]),
                 best_is_local=bool(r.best_is_local[k]), P=r.proj_matrix[k], qvec=r.qvec[k], tvec=r.tvec[k],
                 mask=r.inlier_mask[k]) for k in range(len(cases))]


def grouped(names):
    """{option_key: [case name]} in a fixed order."""
    groups = {}
    for k in names:
        groups.setdefault(ac.option_key(ac.built(k)[1]), []).append(k)
    return groups


def estimate_named(names, estimate):
    """{case name: result} with one call of `estimate` per option_key."""
    out = {}
    for ks in grouped(names).values():
        for k, r in zip(ks, estimate([ac.built(k) for k in ks])):
            out[k] = r
    return out


def check_against_reference(name, got, tol):
    """True when compared; False when the case was excused as rounding-decided."""
    p, o, ref = ac.solved(name)
    want, have = aref.discrete(ref), aref.discrete(got)
    dP = None if not (ref["success"] and got["success"]) else float(np.abs(got["P"] - ref["P"]).max())
    print(f"{name}: n {len(p.points2D)} trials {ref['num_trials']} inliers {ref['num_inliers']} "
          f"local {ref['best_is_local']} | got trials {got['num_trials']} inliers {got['num_inliers']} "
          f"local {got['best_is_local']} | dP {dP}")
    if have != want:
        if ac.rounding_decided(name):
            print(f"{name}: excused, the reference's decisions change under one ulp")
            return False
        assert have == want, name
    # a degenerate scene fixes no pose (a line of points leaves the rotation about it free): decisions only
    if ref["success"] and name not in ac.DEGENERATE_CASES:
        assert dP <= tol, (name, dP, tol)
    return True


def assert_excused_cap(compared):
    excused = [k for k, ok in compared.items() if not ok]
    print(f"excused as rounding-decided: {len(excused)} of {len(compared)} {excused}")
    assert len(excused) * 20 <= len(compared)


def all_case_names():
    return ac.LENGTH_CASES + ac.MODEL_CASES + [k for k in ac.CASES if k.startswith(("max_trials", "min_trials"))] + \
        ac.DEGENERATE_CASES + ["mapper_outliers", "mapper_pinhole"] + ac.capacity_cases(M.absolute_pose_lds_capacity())


# --------------------------------------------------------------------------- CPU: ABI, defaults, refusals
def test_defaults_are_the_reference_options():
    """RANSACOptions (optim/ransac.h:47-66)."""
    o = M.default_absolute_pose_estimation_options()
    assert (o.max_error, o.min_inlier_ratio, o.confidence, o.dyn_num_trials_multiplier) == (0.0, 0.1, 0.99, 3.0)
    assert (o.min_num_trials, o.max_num_trials, o.seed, o.device) == (0, INT64_MAX, 0, 0)


def test_new_symbols_are_declared():
    text = open(os.path.join(M._HERE, "..", "include", "mi_ba.h")).read()
    for name in ("mi_ba_absolute_pose_estimation_options", "mi_ba_absolute_pose_estimation_batch"):
        assert name in text
    for name in ("mi_ba_default_absolute_pose_estimation_options", "mi_ba_estimate_absolute_pose_batch",
                 "mi_ba_absolute_pose_lds_capacity"):
        assert name in text and hasattr(M.load(), name)
    assert "#define MI_BA_ABI_VERSION 4" in text
    assert M.load().mi_ba_abi_version() == 4


def test_lds_capacity():
    """Reported without a device; four waves of records fit the 160 KiB."""
    cap = M.absolute_pose_lds_capacity()
    assert 64 <= cap and 4 * cap * 5 * 8 <= 160 * 1024


def estimate_status(cases, o, mutate=None):
    a = M._AbsolutePoseEstimationArrays(*pack(cases), o)
    if mutate:
        mutate(a)
    n = max(a.n, 1)
    succ = np.zeros(n, np.int32)
    return M.load().mi_ba_estimate_absolute_pose_batch(C.byref(o), C.byref(a.batch), None, None, None, None,
                                                       M._ptr(succ, M._i32p), None, None, None)


def test_invalid_arguments_are_refused_without_a_device():
    """Every check returns MI_BA_ERR_INVALID_ARGUMENT (1) before a device is
    touched (without a device a valid call returns MI_BA_ERR_NO_DEVICE, 2)."""
    cases = [ac.built("n5"), ac.built("model_pinhole")]
    good = lambda **kw: M.default_absolute_pose_estimation_options(**{**dict(max_error=12.0), **kw})
    assert estimate_status(cases, good()) in (0, 2)
    # RANSACOptions::Check
    for kw in (dict(max_error=0.0), dict(max_error=-1.0), dict(max_error=float("nan")), dict(max_error=float("inf")),
               dict(min_inlier_ratio=-0.1), dict(min_inlier_ratio=1.1), dict(confidence=-0.1), dict(confidence=1.1),
               dict(min_num_trials=11, max_num_trials=10), dict(min_num_trials=-1)):
        assert estimate_status(cases, good(**kw)) == 1, kw
    # the unbounded-trials case
    assert estimate_status(cases, good(confidence=1.0)) == 1
    assert estimate_status(cases, good(min_inlier_ratio=0.0)) == 1
    assert estimate_status(cases, good(confidence=1.0, max_num_trials=1000)) in (0, 2)
    # focal factors
    for bad in (0.0, -1.0, float("nan"), float("inf")):
        def mutate(a, bad=bad):
            a.factor[1] = bad
        assert estimate_status(cases, good(), mutate) == 1, bad

    def decreasing(a):
        a.set_off[1] = a.set_off[2] + 1
    assert estimate_status(cases, good(), decreasing) == 1
    for index, value in (("set_index", 2), ("set_index", -1), ("camera_index", 2), ("camera_index", -1)):
        def mutate(a, index=index, value=value):
            getattr(a, index)[0] = value
        assert estimate_status(cases, good(), mutate) == 1, (index, value)

    def unknown_model(a):
        a.models[0] = 6  # FULL_OPENCV
    assert estimate_status(cases, good(), unknown_model) == 1

    def wrong_count(a):
        a.models[0] = M.RADIAL  # five parameters, three given
    assert estimate_status(cases, good(), wrong_count) == 1

    def negative(a):
        a.batch.num_problems = -1
    assert estimate_status(cases, good(), negative) == 1

    def too_long(a):  # 5 doubles per record are indexed with int (refused before any array is read)
        a.set_off[2] = a.set_off[1] + (2 ** 31 - 1) // 5 + 1
    assert estimate_status(cases, good(), too_long) == 1

    def nullable(a):  # focal_length_factor = NULL means 1, seed = NULL the option's
        a.batch.focal_length_factor = None
        a.batch.seed = None
    assert estimate_status(cases, good(), nullable) in (0, 2)
    assert M.load().mi_ba_estimate_absolute_pose_batch(None, None, None, None, None, None, None, None, None, None) == 1


# --------------------------------------------------------------------------- CPU: the sampler
def c_samples(seed, n, count, tmp_path):
    dst = str(tmp_path / f"samples_{seed}_{n}.txt")
    run_program("absolute_pose_block_test", "sample", str(seed), str(n), str(count), dst)
    return np.loadtxt(dst, dtype=np.int64).reshape(-1, 3)


def test_sampler_is_the_same_in_c_and_numpy(tmp_path):
    """Distinct, in range, identical in both restatements, for n at its minimum and across a lane edge."""
    for seed, n in ((0, 3), (1, 4), (2 ** 64 - 1, 5), (12345678901234567, 65), (7, 1000)):
        got = c_samples(seed, n, 500, tmp_path)
        want = np.array([aref.sample(seed, t, n) for t in range(500)])
        assert np.array_equal(got, want), (seed, n)
        assert got.min() >= 0 and got.max() < n
        assert all(len(set(row)) == 3 for row in got.tolist())


def test_sampler_is_uniform_on_five():
    """Chi-square sanity check: the 60 ordered triples of five elements over
    60 000 trials; 59 degrees of freedom, the 99.99 % quantile is 109."""
    counts = {}
    for t in range(60000):
        k = tuple(aref.sample(3, t, 5))
        counts[k] = counts.get(k, 0) + 1
    assert len(counts) == 60
    chi2 = sum((c - 1000.0) ** 2 / 1000.0 for c in counts.values())
    print("chi-square", chi2)
    assert chi2 < 109.0


# --------------------------------------------------------------------------- CPU: the reference's own unit tests
@functools.lru_cache(maxsize=None)
def golden():
    return json.load(open(GOLDEN))


def ransac_p3p_only(x2, X3, max_error, models_of):
    """RANSAC<P3PEstimator> made deterministic: every triple of the scene in
    lexicographic order, the best support wins."""
    best, best_model = (0, aref.DBL_MAX), None
    n = len(x2)
    for i in range(n):
        for j in range(i + 1, n):
            for k in range(j + 1, n):
                for P in models_of((i, j, k)):
                    if not np.all(np.isfinite(P)):
                        continue
                    s = aref.evaluate_support(aref.squared_errors(x2, X3, P), max_error * max_error)
                    if aref.better(s, best):
                        best, best_model = s, P
    return best, best_model


def check_scene8(pose, X3, P, matrix_bound):
    g = golden()
    b = g["bounds"]
    x2 = np.array(pose["points2D"])
    faulty = X3.copy()
    faulty[:, 0] = g["scene8"]["faulty_x"]
    assert np.linalg.norm(np.array(pose["matrix"]) - P) < matrix_bound
    assert (aref.squared_errors(x2, X3, P) < b["residual_exact_below"]).all()
    assert (aref.squared_errors(x2, faulty, P) > b["residual_faulty_above"]).all()


def model_sets_file(tmp_path, sets, name):
    src, dst = str(tmp_path / f"{name}.bin"), str(tmp_path / f"{name}.out")
    cams = [(M.SIMPLE_PINHOLE, [1.0, 0.0, 0.0])]
    write_batch(src, sets, cams, [], ac.options(max_error=1.0))
    run_program("absolute_pose_block_test", name, src, dst)
    out = []
    for line in open(dst):
        w = line.split()
        out.append([fromhex(w[1 + 12 * k:13 + 12 * k]).reshape(3, 4) for k in range(int(w[0]))])
    return out


TRIPLES = [(i, j, k) for i in range(8) for j in range(i + 1, 8) for k in range(j + 1, 8)]


@pytest.mark.parametrize("build", ["numpy", "host"])
def test_p3p_known_answers(build, tmp_path):
    """TestP3P (absolute_pose_test.cc:46-104) on every pose of the fixture."""
    g = golden()
    X3 = np.array(g["scene8"]["points3D"])
    poses = g["scene8"]["poses"]
    if build == "host":
        sets = [(np.array(p["points2D"])[list(t)], X3[list(t)]) for p in poses for t in TRIPLES]
        models = model_sets_file(tmp_path, sets, "p3p")
    for n, pose in enumerate(poses):
        x2 = np.array(pose["points2D"])
        if build == "host":
            of = {t: models[n * len(TRIPLES) + m] for m, t in enumerate(TRIPLES)}
            models_of = lambda t: of[t]
        else:
            models_of = lambda t: aref.p3p(x2[list(t)], X3[list(t)])
        support, P = ransac_p3p_only(x2, X3, g["scene8"]["max_error"], models_of)
        assert support[0] >= 3
        check_scene8(pose, X3, P, g["bounds"]["p3p_matrix_diff"])


@pytest.mark.parametrize("build", ["numpy", "host"])
def test_epnp_known_answers(build, tmp_path):
    """TestEPNP and TestEPNP_BrokenSolveSignCase (absolute_pose_test.cc:106-220)."""
    g = golden()
    X3 = np.array(g["scene8"]["points3D"])
    poses = g["scene8"]["poses"]
    bx2, bX3 = np.array(g["broken_sign"]["points2D"]), np.array(g["broken_sign"]["points3D"])
    if build == "host":
        models = model_sets_file(tmp_path, [(np.array(p["points2D"]), X3) for p in poses] + [(bx2, bX3)], "epnp")
    else:
        models = [aref.epnp(np.array(p["points2D"]), X3) for p in poses] + [aref.epnp(bx2, bX3)]
    for pose, ms in zip(poses, models):
        assert len(ms) == 1
        # RANSAC<EPNPEstimator> at max_error 1e-5 succeeds: at least four inliers
        res = aref.squared_errors(np.array(pose["points2D"]), X3, ms[0])
        assert (res <= g["scene8"]["max_error"] ** 2).sum() >= 4
        check_scene8(pose, X3, ms[0], g["bounds"]["epnp_matrix_diff"])
    assert len(models[-1]) == g["bounds"]["broken_sign_num_models"]
    P = models[-1][0]
    pc = bX3 @ P[:, :3].T + P[:, 3]
    reproj = np.linalg.norm(pc[:, :2] / pc[:, 2:] - bx2, axis=1).sum()
    print("reprojection", reproj)
    assert reproj < g["bounds"]["broken_sign_reprojection_below"]


def test_block_header_on_the_host():
    run_program("absolute_pose_block_test")


def test_block_header_under_sanitizers(tmp_path):
    """The stand-alone program under AddressSanitizer + UBSan: its built-in
    checks and a batch with outliers, degenerate and short problems."""
    run_program("absolute_pose_block_test_san")
    names = ["n2", "n3", "n5", "n65", "coincident", "collinear", "behind"]
    got = host_estimate([ac.built(k) for k in names], tmp_path, target="absolute_pose_block_test_san")
    assert len(got) == len(names)


# --------------------------------------------------------------------------- CPU: host build against numpy
def test_host_build_matches_reference(tmp_path):
    """Decision for decision on the case list; prints the largest proj_matrix
    difference, which HOST_VS_NUMPY records."""
    names = all_case_names()
    got = estimate_named(names, lambda cases: host_estimate(cases, tmp_path))
    compared = {k: check_against_reference(k, got[k], HOST_TOL) for k in names}
    assert_excused_cap(compared)
    worst = max(float(np.abs(got[k]["P"] - ac.solved(k)[2]["P"]).max()) for k in names
                if compared[k] and ac.solved(k)[2]["success"] and k not in ac.DEGENERATE_CASES)
    print(f"largest |P host - P numpy| over the case list: {worst:.4e} (recorded {HOST_VS_NUMPY:.4e})")
    assert worst <= HOST_TOL


def test_reference_decisions_are_stable():
    """With the numpy reference alone: at most 1 case in 20 changes a discrete
    output under inputs moved by one ulp, so the excuse of the comparisons
    cannot hide a category."""
    names = all_case_names()
    unstable = [k for k in names if ac.rounding_decided(k)]
    print("rounding-decided cases:", unstable)
    assert len(unstable) * 20 <= len(names)


def test_short_and_failing_cases_are_what_they_claim():
    """n = 2 fails with 0 trials; n = 3 cannot run the local optimisation."""
    assert aref.discrete(ac.solved("n2")[2]) == (False, 0, False, 0, None)
    r3 = ac.solved("n3")[2]
    assert r3["success"] and r3["num_inliers"] == 3 and not r3["best_is_local"]
    assert ac.solved("n4")[2]["num_inliers"] == 4  # the local optimisation ran on four
    for k in ("n5", "n64", "mapper_outliers"):
        assert ac.solved(k)[2]["best_is_local"], k
    for t in (1, 64, 65):
        assert ac.solved(f"max_trials{t}")[2]["num_trials"] == t
    # the abort lands at trial min_num_trials and one more trial is counted
    for t in (63, 64, 65):
        assert ac.solved(f"min_trials{t}")[2]["num_trials"] == t + 2


# --------------------------------------------------------------------------- CPU: the facade
def facade_lines(*args):
    return run_program("absolute_pose_test", *args)


def test_facade_sweep_factors():
    """The focal-length factors of the facade equal the reference loop's, whose trip count rounding decides."""
    for samples in (1, 3, 30):
        out = facade_lines("factors", str(samples), "0.2", "5.0")
        got = [float.fromhex(w) for line in out.splitlines() if line.startswith("FACTORS") for w in line.split()[1:]]
        want = aref.focal_length_factors(samples, 0.2, 5.0)
        assert got == want, samples
    assert len(aref.focal_length_factors(30, 0.2, 5.0)) == 31


def test_facade_options_check():
    facade_lines("check")


# --------------------------------------------------------------------------- GPU
@pytest.fixture(scope="module")
def device_results():
    """Every named case on the device, one launch per option_key."""
    return estimate_named(all_case_names(), device_estimate)


def compare_on_device(names, device_results):
    compared = {k: check_against_reference(k, device_results[k], PROJ_TOL) for k in names}
    assert_excused_cap(compared)


@pytest.mark.gpu
def test_gpu_lengths(device_results):
    """2: failure with 0 trials; 3: no local optimisation; 4, 5: EPnP at its minimum; 63, 64, 65: lane edges."""
    got = device_results["n2"]
    assert aref.discrete(got) == (False, 0, False, 0, None)
    assert np.isnan(got["P"]).all()  # a failed problem's outputs are untouched
    compare_on_device(ac.LENGTH_CASES + ac.DEGENERATE_CASES + ["mapper_outliers", "mapper_pinhole"], device_results)


@pytest.mark.gpu
def test_gpu_resident_against_streamed(device_results):
    """One below, at and one above the LDS capacity."""
    compare_on_device(ac.capacity_cases(M.absolute_pose_lds_capacity()), device_results)


@pytest.mark.gpu
def test_gpu_trial_edges(device_results):
    """max_num_trials 1, 64, 65 and an abort inside, at the end of and just past a round."""
    names = [f"max_trials{t}" for t in (1, 64, 65)] + [f"min_trials{t}" for t in (63, 64, 65)]
    compare_on_device(names, device_results)
    for t in (63, 64, 65):
        assert device_results[f"min_trials{t}"]["num_trials"] == t + 2  # the extra counted trial


@pytest.mark.gpu
def test_gpu_all_camera_models_in_one_batch(device_results):
    """Nine models, one problem each, one launch (they share an option_key)."""
    assert len(grouped(ac.MODEL_CASES)) == 1
    compare_on_device(ac.MODEL_CASES, device_results)
    for k in ac.MODEL_CASES:
        p, _, _ = ac.solved(k)
        got = device_results[k]
        assert got["success"] and np.array_equal(got["mask"], p.inlier), k
        assert np.abs(got["P"][:, :3] - p.R).max() < 5e-3 and np.abs(got["P"][:, 3] - p.t).max() < 5e-2


@pytest.mark.gpu
def test_gpu_batch_positions_and_runs_give_the_same_bits():
    """1, kPoseWaves and kPoseWaves + 1 problems; the same problem first, in
    the middle, last and alone; two runs."""
    waves = pose_waves()
    probe = ac.built("mapper_outliers")
    others = [ac.make_problem(50 + i, 700 + i) for i in range(waves)]
    o = probe[1]
    fill = [(q, o) for q in others]
    alone = device_estimate([probe])[0]
    again = device_estimate([probe])[0]

    def same(a, b):
        return (aref.discrete(a) == aref.discrete(b) and a["P"].tobytes() == b["P"].tobytes()
                and a["qvec"].tobytes() == b["qvec"].tobytes() and a["tvec"].tobytes() == b["tvec"].tobytes())
    assert alone["success"] and same(alone, again)
    for size in (waves, waves + 1):
        for pos in (0, size // 2, size - 1):
            batch = fill[:size - 1]
            batch.insert(pos, probe)
            got = device_estimate(batch)
            assert same(got[pos], alone), (size, pos)
    # the fillers have their own seeds in their own batch: compare two runs of a full batch
    full = [(q, ac.options(seed=40 + i)) for i, q in enumerate(others)] + [(probe[0], ac.options(seed=o.seed))]
    a, b = device_estimate(full), device_estimate(full)
    assert all(same(x, y) for x, y in zip(a, b))


@pytest.mark.gpu
def test_gpu_null_factor_and_seed_arrays():
    """focal_length_factor = NULL is a factor of 1 for every problem and
    seed = NULL the option's seed: the same bits as the arrays that say so."""
    cases = [ac.built("n65"), ac.built("model_pinhole")]
    o = ac.device_options(ac.options(seed=77))

    def call(null):
        a = M._AbsolutePoseEstimationArrays(*pack(cases), o)
        a.factor[:] = 1.0
        a.seed[:] = 77
        if null:
            a.batch.focal_length_factor = None
            a.batch.seed = None
        n, total = a.n, int(a.mask_off[-1])
        P, mask = np.zeros((n, 12)), np.zeros(total, np.uint8)
        succ, inl, loc, trials = np.zeros(n, np.int32), np.zeros(n, np.int32), np.zeros(n, np.int32), np.zeros(n, np.int64)
        M.check(M.load().mi_ba_estimate_absolute_pose_batch(
            C.byref(o), C.byref(a.batch), M._ptr(P, M._dp), None, None, M._ptr(mask, M._u8p), M._ptr(succ, M._i32p),
            M._ptr(trials, M._i64p), M._ptr(inl, M._i32p), M._ptr(loc, M._i32p)), "mi_ba_estimate_absolute_pose_batch")
        return P.tobytes(), mask.tobytes(), succ.tolist(), trials.tolist(), inl.tolist(), loc.tolist()
    given, null = call(False), call(True)
    assert given[2] == [1, 1] and given == null


@pytest.mark.gpu
def test_gpu_known_answers():
    """The reference's own unit-test scenes through the batch entry point (a
    unit camera: pixels are normalised coordinates)."""
    g = golden()
    X3 = np.array(g["scene8"]["points3D"])
    poses = g["scene8"]["poses"]
    cam = (M.SIMPLE_PINHOLE, [1.0, 0.0, 0.0])
    bx2, bX3 = np.array(g["broken_sign"]["points2D"]), np.array(g["broken_sign"]["points3D"])
    o = M.default_absolute_pose_estimation_options(max_error=g["scene8"]["max_error"], max_num_trials=200)
    sets = [(np.array(p["points2D"]), X3) for p in poses]
    problems = [M.AbsolutePoseEstimationProblem(k, 0, 1.0, k) for k in range(len(poses))]
    r = M.estimate_absolute_pose_batch(o, sets, [cam], problems)
    for k, pose in enumerate(poses):
        assert r.success[k] and r.num_inliers[k] >= 3
        check_scene8(pose, X3, r.proj_matrix[k], g["bounds"]["epnp_matrix_diff" if r.best_is_local[k] else "p3p_matrix_diff"])
    # the broken-sign scene is noisy: every point within 0.1 makes EPnP on all twelve the local model
    ob = ac.options(max_error=0.1, seed=5)
    pb = ac.Problem(bx2, bX3, cam[0], np.array(cam[1]))
    got = device_estimate([(pb, ob)])[0]
    ref = ac.reference(pb, ob)
    assert aref.discrete(got) == aref.discrete(ref)
    assert got["best_is_local"] and got["num_inliers"] == 12
    pc = bX3 @ got["P"][:, :3].T + got["P"][:, 3]
    assert np.linalg.norm(pc[:, :2] / pc[:, 2:] - bx2, axis=1).sum() < g["bounds"]["broken_sign_reprojection_below"]


@pytest.mark.gpu
def test_gpu_focal_sweep_through_the_facade(tmp_path):
    """A camera whose focal length is off by 1.4: the facade's sweep picks the
    reference's factor, mask and inlier count."""
    p = ac.make_problem(60, 801, camera="simple_radial", true_factor=1.4)
    o = ac.options(seed=0)
    ref = aref.estimate_absolute_pose(o, p.model, p.params, p.points2D, p.points3D, estimate_focal_length=True)
    src = str(tmp_path / "sweep.bin")
    write_batch(src, *pack([(p, o)]), o)
    out = facade_lines("sweep", src)
    w = [line for line in out.splitlines() if line.startswith("SWEEP")][0].split()
    ok, inliers, f0, mask = w[1] == "1", int(w[2]), float.fromhex(w[3]), np.array([c == "1" for c in w[4]])
    print("factor", ref["factor"], "inliers", ref["num_inliers"], "| facade focal", f0, "inliers", inliers)
    assert ref["success"] and 1.2 < ref["factor"] < 1.6
    assert ok and inliers == ref["num_inliers"] and np.array_equal(mask, ref["mask"])
    assert f0 == ref["params"][0]


@pytest.mark.gpu
def test_gpu_estimate_then_refine_reaches_the_ground_truth():
    """The estimate's mask and pose into the existing refine_absolute_pose_batch
    on a noisy scene with 30 % outliers.

    The bound test_pose_refine.py uses for such scenes is 1e-5 on qvec and tvec
    against its reference solution, the unchanged CPU oracle on the same
    problem (pose_cases.oracle_solve); the chain is held to exactly that.  The
    true pose itself cannot be met to 1e-5 by any estimator: with uniform noise
    of 0.5 px (sigma 0.29 px) on 140 inliers at focal 1000 and depths of 4 to
    10, the least-squares optimum scatters about the truth by some
    7 x 2.9e-4 / (0.4 x sqrt 140) = 4e-4 in the depth of tvec and a tenth of
    that in qvec.  So the distance to the truth is bounded by ten such sigmas,
    4e-3 and 4e-4.  Measured on the device: 1.4e-3 and 8.4e-5; the same
    refinement started at the true pose ends 1.4e-5 (tvec) and 1.1e-7 (qvec)
    away, which is Ceres' function tolerance, not the estimate."""
    import pose_cases as pc
    p, o = ac.make_problem(200, 901, camera="simple_radial"), ac.mapper_options(seed=9)
    got = device_estimate([(p, o)])[0]
    assert got["success"] and np.array_equal(got["mask"], p.inlier)
    chain = M.PoseProblem(p.model, p.params.copy(), got["qvec"].copy(), got["tvec"].copy(), p.points2D, p.points3D,
                          inlier_mask=got["mask"].astype(np.uint8))
    r = M.refine_absolute_pose_batch(M.default_pose_refine_options(), [chain])
    assert np.all(r.statuses == M.OK) and np.all(r.usable == 1)
    _, _, sc = pc.oracle_solve(chain)
    q_true = aref.rotation_to_quaternion(p.R)
    q = r.qvec[0] * np.sign(r.qvec[0][0])
    dq, dt = np.abs(r.qvec[0] - sc.qvec[0]).max(), np.abs(r.tvec[0] - sc.tvec[0]).max()
    tq, tt = np.abs(q - q_true * np.sign(q_true[0])).max(), np.abs(r.tvec[0] - p.t).max()
    print("refined against the oracle: dq", dq, "dt", dt, "| against the true pose: dq", tq, "dt", tt)
    assert dq <= 1e-5 and dt <= 1e-5
    assert tq <= 4e-4 and tt <= 4e-3
