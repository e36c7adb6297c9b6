"""Batched robust triangulation: mi_ba_estimate_triangulation_batch
(EstimateTriangulation, src/estimators/triangulation.cc:132-160) and
mi_ba_triangulate_points.

The oracle is tests/triangulation_reference.py, a numpy restatement of the
reference's LO-RANSAC and of the functions under it (numpy.linalg.svd / eigh;
it shares no code with csrc/triangulation_block.h).  Eigen is not available,
so the reference's own sources cannot be compiled.  The estimator is
deterministic (CombinationSampler draws no random number), so the comparison
is decision for decision: success, the inlier mask, num_trials, num_inliers
and best_is_local must be equal, and xyz must agree within the larger of
1e-9 max(1, |xyz|) and ten times the restatement's own spread under inputs
perturbed by one ulp (triangulation_cases.solved).

Decision stability is a condition, not a tolerance: a case is compared only if
the restatement's discrete outputs are unchanged under four runs with every
projection-matrix entry and image coordinate perturbed by a relative 1e-9 (the
arithmetic differences between SVD implementations are some three orders below
that).  At most 5 % of the cases and no whole category may be dropped; on the
committed seeds none is.

CPU tests run the host build of the block header (tests/cpp/
triangulation_block_test.cc) and the facade's host mode; GPU tests the device."""
import ctypes as C
import functools
import os

import numpy as np
import pytest

import mi_ba
import triangulation_cases as tc
import triangulation_reference as tref
from estimator_testing import hexes, make, run_program

M = mi_ba
run_program = functools.partial(run_program, timeout=600)
INT64_MAX = 2 ** 63 - 1

# the categories of the parity comparison: every one must keep a stable case
CATEGORIES = {
    "lengths": ["len2", "len3", "len4", "len15", "len16", "len64", "len65"],
    "lengths_reprojection_mixed_cameras": ["len2_reproj", "len3_reproj", "len4_reproj", "len15_reproj", "len16_reproj",
                                           "len64_reproj", "len65_reproj"],
    "derived_normalized": ["len9_derived", "len9_derived_reproj"],
    "outliers": ["len30_outliers", "len40_outliers_reproj"],
    "trial_cap": ["len12_cap40", "len12_trials64", "len12_trials65"],
    "min_num_trials": ["len20_min150"],
    "failing": list(tc.FAILING),
}


def option_key(o):
    """What a batch shares; min_num_trials goes per track."""
    return (o.min_tri_angle, o.residual_type, o.max_error, o.min_inlier_ratio, o.confidence,
            o.dyn_num_trials_multiplier, o.max_num_trials)


def write_batch(path, tracks, with_normalized=True):
    """The binary form tests/cpp/triangulation_block_test.cc reads; tracks: [(Track, Options)] of one option_key."""
    a = M._TriangulationArrays(*tc.pack(tracks))
    o = tracks[0][1]
    n, N = a.n, int(a.obs_off[-1])
    prm8 = np.zeros((len(a.models), 8))
    for c in range(len(a.models)):
        prm8[c, :a.prm_off[c + 1] - a.prm_off[c]] = a.prm[a.prm_off[c]:a.prm_off[c + 1]]
    with open(path, "wb") as f:
        np.array([n, N, len(a.proj), len(a.models), 1 if with_normalized else 0, 1], np.int64).tofile(f)
        np.array([o.min_tri_angle, o.residual_type, o.max_error, o.min_inlier_ratio, o.confidence,
                  o.dyn_num_trials_multiplier, 0, min(o.max_num_trials, 1e19)], np.float64).tofile(f)
        a.obs_off.tofile(f)
        np.array([t[1].min_num_trials for t in tracks], np.int64).tofile(f)
        a.view.tofile(f)
        a.points.tofile(f)
        if with_normalized:
            a.normalized.tofile(f)
        a.proj.tofile(f)
        a.centers.tofile(f)
        a.view_cam.tofile(f)
        a.models.tofile(f)
        prm8.tofile(f)


def host_estimate(tracks, tmp_path, with_normalized=True, target="triangulation_block_test"):
    """The host build of the block header on tracks of one option_key: a list of result dicts."""
    src, dst = str(tmp_path / "batch.bin"), str(tmp_path / "batch.out")
    write_batch(src, tracks, with_normalized)
    run_program(target, "estimate", src, dst)
    out = []
    for line in open(dst):
        w = line.split()
        ok = w[0] == "1"
        out.append(dict(success=ok, num_trials=int(w[1]), num_inliers=int(w[2]), best_is_local=w[3] == "1",
                        xyz=np.array([float.fromhex(v) for v in w[4:7]]) if ok else None,
                        mask=np.array([c == "1" for c in w[7]]) if ok else None))
    return out


def grouped(names):
    """{option_key: [case name]} in a fixed order."""
    groups = {}
    for k in names:
        groups.setdefault(option_key(tc.solved(k)[1]), []).append(k)
    return groups


def check_against_reference(name, got):
    track, o, ref, stable, bound = tc.solved(name)
    want = tref.discrete(ref)
    have = tref.discrete(got)
    dx = None if not ref["success"] or got["xyz"] is None else float(np.abs(got["xyz"] - ref["xyz"]).max())
    print(f"{name}: n {len(track)} stable {stable} trials {ref['num_trials']} inliers {ref['num_inliers']} "
          f"local {ref['best_is_local']} recursions {ref['local_recursions']} | got trials {got['num_trials']} "
          f"inliers {got['num_inliers']} local {got['best_is_local']} | dxyz {dx} bound {bound}")
    if not stable:
        return False
    assert have == want, name
    if ref["success"]:
        assert dx <= bound, (name, dx, bound)
    return True


def all_case_names():
    return [k for ks in CATEGORIES.values() for k in ks] + list(tc.capacity_cases(M.triangulation_lds_capacity()))


def assert_stability_cap(compared):
    """compared: {case name: bool}.  At most 5 % dropped, no whole category."""
    dropped = [k for k, ok in compared.items() if not ok]
    print("dropped as unstable:", dropped)
    assert len(dropped) * 20 <= len(compared)
    cats = dict(CATEGORIES, capacity=list(tc.capacity_cases(M.triangulation_lds_capacity())))
    for cat, ks in cats.items():
        assert any(compared[k] for k in ks), cat


def grid_pairs():
    """The scene of the reference's TestTriangulatePoint (triangulation_test.cc:42-78): 6 points x 5 qz x 5 tx."""
    pts = np.array([[0, 0.1, 0.1], [0, 1, 3], [0, 1, 2], [0.01, 0.2, 3], [-1, 0.1, 1], [0.1, 0.1, 0.2]])
    P1 = np.eye(3, 4)
    out = []
    qz = 0.0
    while qz < 1:
        tx = 0.0
        while tx < 10:
            q = np.array([0.2, 0.3, 0.4, qz])
            P2 = np.concatenate([M.quat_to_rot(q / np.linalg.norm(q)), [[tx], [2.0], [3.0]]], axis=1)
            x1 = pts[:, :2] / pts[:, 2:]
            pc = pts @ P2[:, :3].T + P2[:, 3]
            out.append((P1, P2, x1, pc[:, :2] / pc[:, 2:], pts))
            tx += 2
        qz += 0.2
    assert len(out) == 25
    return out


# --------------------------------------------------------------------------- CPU: ABI, defaults, refusals
def test_defaults_are_the_reference_options():
    """RANSACOptions (optim/ransac.h:47-66) and EstimateTriangulationOptions (estimators/triangulation.h:123-138)."""
    o = M.default_triangulation_options()
    assert (o.min_tri_angle, o.residual_type, o.max_error) == (0.0, M.TRIANGULATION_ANGULAR_ERROR, 0.0)
    assert (o.min_inlier_ratio, o.confidence, o.dyn_num_trials_multiplier) == (0.1, 0.99, 3.0)
    assert (o.min_num_trials, o.max_num_trials, o.device) == (0, INT64_MAX, 0)


def test_new_symbols_are_declared():
    text = open(os.path.join(M._HERE, "..", "include", "mi_ba.h")).read()
    for name in ("mi_ba_triangulation_options", "mi_ba_triangulation_batch"):
        assert name in text
    for name in ("mi_ba_default_triangulation_options", "mi_ba_estimate_triangulation_batch",
                 "mi_ba_triangulate_points", "mi_ba_triangulation_lds_capacity"):
        assert name in text and hasattr(M.load(), name)
    assert "#define MI_BA_ABI_VERSION 4" in text
    assert M.load().mi_ba_abi_version() == 4


def test_lds_capacity():
    """Reported without a device; four waves of padded records fit the 160 KiB."""
    cap = M.triangulation_lds_capacity()
    assert 64 <= cap and 4 * cap * 25 * 8 <= 160 * 1024


def estimate_status(tracks, o, mutate=None, sentinel=None):
    a = M._TriangulationArrays(*tc.pack(tracks))
    a.resolve_min_trials(o)
    if mutate:
        mutate(a)
    n, total = a.n, max(int(a.obs_off.max()), 1)
    xyz = np.full((max(n, 1), 3), 7.0)
    mask = np.full(total, 9, np.uint8)
    succ, inl, loc = np.zeros(max(n, 1), np.int32), np.zeros(max(n, 1), np.int32), np.zeros(max(n, 1), np.int32)
    trials = np.zeros(max(n, 1), np.int64)
    st = M.load().mi_ba_estimate_triangulation_batch(C.byref(o), C.byref(a.batch), M._ptr(xyz, M._dp),
                                                     M._ptr(mask, M._u8p), M._ptr(succ, M._i32p),
                                                     M._ptr(trials, M._i64p), M._ptr(inl, M._i32p),
                                                     M._ptr(loc, M._i32p))
    if sentinel is not None:
        sentinel.update(xyz=xyz, mask=mask, success=succ, offsets=a.obs_off)
    return st


def two_tracks():
    return [(tc.make_track(5, 1), tc.create_options(5)), (tc.make_track(3, 2, cameras=tc.MIXED), tc.create_options(3))]


@pytest.mark.parametrize("kw", [dict(max_error=0.0), dict(max_error=-1.0), dict(max_error=float("nan")),
                                dict(min_inlier_ratio=-0.1), dict(min_inlier_ratio=1.5), dict(confidence=-0.1),
                                dict(confidence=1.1), dict(min_num_trials=11, max_num_trials=10),
                                dict(min_num_trials=-1), dict(min_tri_angle=-1e-300), dict(residual_type=2)])
def test_options_are_refused(kw):
    """RANSACOptions::Check and EstimateTriangulationOptions::Check; refused before any device is touched."""
    tracks = two_tracks()
    o = tc.device_options(tracks[0][1])
    o.min_num_trials = 0
    for k, v in kw.items():
        setattr(o, k, v)
    for t in tracks:
        t[1].min_num_trials = None  # the option's value goes for every track
    assert estimate_status(tracks, o) == M.ERR_INVALID_ARGUMENT
    with pytest.raises(M.MiBaError) as e:
        M.estimate_triangulation_batch(o, *tc.pack(tracks))
    assert e.value.status == M.ERR_INVALID_ARGUMENT


def test_arguments_are_refused():
    tracks = two_tracks()
    o = tc.device_options(tracks[0][1])
    bad = M.ERR_INVALID_ARGUMENT

    def setter(name, value):
        return lambda a: setattr(a.batch, name, value)

    def poke(array, index, value):
        def f(a):
            getattr(a, array)[index] = value
        return f
    assert estimate_status(tracks, o, setter("num_problems", -1)) == bad
    assert estimate_status(tracks, o, poke("obs_off", 1, 9)) == bad          # offsets that decrease
    assert estimate_status(tracks, o, poke("obs_off", 1, 7)) == bad          # a track of one observation
    assert estimate_status(tracks, o, poke("view", 2, 8)) == bad             # view index out of range
    assert estimate_status(tracks, o, poke("view", 2, -1)) == bad
    assert estimate_status(tracks, o, poke("view_cam", 0, 3)) == bad         # camera index out of range
    assert estimate_status(tracks, o, poke("models", 1, 6)) == bad           # FULL_OPENCV: refused
    assert estimate_status(tracks, o, poke("models", 0, 0)) == bad           # parameter count does not fit
    assert estimate_status(tracks, o, poke("min_trials", 0, 20000)) == bad   # above max_num_trials
    # the angular residual needs no pixels when point_normalized is given: not refused
    assert estimate_status(tracks, o, setter("points", None)) in (M.OK, M.ERR_NO_DEVICE)
    ro = tc.device_options(tc.complete_options())
    assert estimate_status(tracks, ro, setter("points", None)) == bad        # reprojection residuals without points

    def neither(a):
        a.batch.points = None
        a.batch.points_normalized = None
    assert estimate_status(tracks, o, neither) == bad
    assert estimate_status(tracks, o, setter("proj_matrices", None)) == bad
    # an empty batch is no error and needs no device
    assert estimate_status([], o) == M.OK
    # the two-view entry
    lib, z = M.load(), np.zeros(12)
    assert lib.mi_ba_triangulate_points(None, None, 1, None, None, None, None, 0, M._ptr(z, M._dp), None) == bad
    assert lib.mi_ba_triangulate_points(M._ptr(z, M._dp), None, 1, M._ptr(z, M._dp), M._ptr(z, M._dp), None, None, 0,
                                        M._ptr(z, M._dp), None) == bad
    assert lib.mi_ba_triangulate_points(M._ptr(z, M._dp), M._ptr(z, M._dp), -1, M._ptr(z, M._dp), M._ptr(z, M._dp),
                                        None, None, 0, M._ptr(z, M._dp), None) == bad
    with pytest.raises(ValueError):
        M.triangulate_points(np.eye(3, 4), np.eye(3, 4), np.zeros((2, 2)), np.zeros((3, 2)))


# --------------------------------------------------------------------------- CPU: the restatement against itself
def test_reference_num_trials():
    """ComputeNumTrials' three early returns and the constructor's cap (ransac.h:146-180)."""
    assert tref.compute_num_trials(5, 10, 1.0, 3.0) == tref.MAX_TRIALS
    assert tref.compute_num_trials(10, 10, 0.99, 3.0) == 1
    assert tref.compute_num_trials(0, 10, 0.99, 3.0) == tref.MAX_TRIALS
    assert tref.compute_num_trials(10000, 100000, 0.99, 3.0) == 1375   # min_inlier_ratio 0.1
    assert tref.compute_num_trials(5, 10, 0.99, 3.0) == 49


def test_reference_known_answers():
    for P1, P2, x1, x2, pts in grid_pairs():
        for a, b, X in zip(x1, x2, pts):
            assert np.linalg.norm(tref.triangulate_point(P1, P2, a, b) - X) < 1e-10
    c1, c2 = np.zeros(3), np.array([0.0, 1, 0])
    assert abs(tref.triangulation_angle(c1, c2, np.array([0.0, 0, 100])) / 0.009999666687 - 1) <= 1e-10
    assert abs(tref.triangulation_angle(c1, c2, np.array([0.0, 0, 50])) / 0.019997333973 - 1) <= 1e-10


# --------------------------------------------------------------------------- CPU: the kernel's arithmetic on the host
def test_host_known_answers(tmp_path):
    """The known answers of src/base/triangulation_test.cc on the host build
    of the block header: the TestTriangulatePoint grid below the reference's
    own 1e-10, the two angles within its relative 1e-8 percent."""
    worst = 0.0
    for k, (P1, P2, x1, x2, pts) in enumerate(grid_pairs()):
        path = str(tmp_path / f"grid{k}.txt")
        with open(path, "w") as f:
            f.write(f"{hexes(P1)} {hexes(P2)} {hexes(np.zeros(3))} {hexes([0, 1, 0])} {float(len(pts)).hex()}\n")
            for a, b in zip(x1, x2):
                f.write(f"{hexes(a)} {hexes(b)}\n")
        rows = np.array([[float.fromhex(v) for v in l.split()[1:]]
                         for l in run_program("triangulation_block_test", "points", path).splitlines()
                         if l.startswith("ROW")])
        worst = max(worst, float(np.linalg.norm(rows[:, :3] - pts, axis=1).max()))
    print("grid: worst error norm", worst)
    assert worst < 1e-10
    path = str(tmp_path / "angles.txt")
    with open(path, "w") as f:
        # the points (0, 0, 100) and (0, 0, 50) seen from (0, 0, 0) and (0, 1, 0)
        P2 = np.concatenate([np.eye(3), [[0.0], [-1.0], [0.0]]], axis=1)
        f.write(f"{hexes(np.eye(3, 4))} {hexes(P2)} {hexes(np.zeros(3))} {hexes([0, 1, 0])} {2.0.hex()}\n")
        f.write(f"{hexes([0, 0])} {hexes([0, -0.01])}\n{hexes([0, 0])} {hexes([0, -0.02])}\n")
    rows = np.array([[float.fromhex(v) for v in l.split()[1:]]
                     for l in run_program("triangulation_block_test", "points", path).splitlines()
                     if l.startswith("ROW")])
    assert np.abs(rows[:, :3] - [[0, 0, 100], [0, 0, 50]]).max() < 1e-9
    assert abs(rows[0, 3] / 0.009999666687 - 1) <= 1e-10 and abs(rows[1, 3] / 0.019997333973 - 1) <= 1e-10


def host_results(names, tmp_path, target="triangulation_block_test"):
    got = {}
    for g, (key, ks) in enumerate(grouped(names).items()):
        d = tmp_path / f"g{g}"
        d.mkdir(exist_ok=True)
        derived = [k for k in ks if "derived" in k]
        plain = [k for k in ks if "derived" not in k]
        for part, with_normalized in ((plain, True), (derived, False)):
            if not part:
                continue
            sub = d / ("n" if with_normalized else "d")
            sub.mkdir(exist_ok=True)
            res = host_estimate([tc.solved(k)[:2] for k in part], sub, with_normalized, target)
            got.update(zip(part, res))
    return got


def test_host_block_matches_reference(tmp_path):
    """tri_loransac of the block header, compiled for the host, against the
    restatement on every case: the discrete outputs equal, xyz within the
    bound; point_normalized given and derived from the pixels."""
    names = all_case_names()
    got = host_results(names, tmp_path)
    compared = {k: check_against_reference(k, got[k]) for k in names}
    assert_stability_cap(compared)
    # the cases do what their names say
    ref = {k: tc.solved(k)[2] for k in names}
    assert ref["len12_cap40"]["num_trials"] == 40 and ref["len12_trials64"]["num_trials"] == 64
    assert ref["len12_trials65"]["num_trials"] == 65 and ref["len20_min150"]["num_trials"] >= 150
    assert ref["len15"]["num_trials"] == 105 and ref["len16"]["num_trials"] < 120
    for k in ("len30_outliers", "len40_outliers_reproj"):
        n = len(tc.solved(k)[0])
        assert ref[k]["local_recursions"] >= 2 and ref[k]["num_trials"] < n * (n - 1) // 2
        assert ref[k]["num_inliers"] < n
    assert not any(ref[k]["success"] for k in tc.FAILING)
    assert any(ref[k]["best_is_local"] for k in names) and any(not ref[k]["best_is_local"] for k in names
                                                               if ref[k]["success"])


def test_general_scenes_are_stable_and_match(tmp_path):
    """The 120 general scenes (lengths 2 to 65, 20 % outliers, Create's
    options): the stability cap holds, all succeed, and the host block agrees
    with the restatement on every stable one."""
    scenes = tc.general_scenes()
    tracks = [(tc.make_track(n, seed), tc.create_options(n)) for n, seed in scenes]
    refs = [tref.estimate_triangulation(o, t) for t, o in tracks]
    stable = [all(tref.discrete(tref.estimate_triangulation(o, tc.perturbed(t, 1e-9, 100 + s))) == tref.discrete(r)
                  for s in range(4)) for (t, o), r in zip(tracks, refs)]
    early = sum(r["num_trials"] < len(t) * (len(t) - 1) // 2 for (t, o), r in zip(tracks, refs))
    print("general scenes: unstable", stable.count(False), "succeeded", sum(r["success"] for r in refs), "ended early",
          early)
    assert stable.count(False) * 20 <= len(scenes)
    assert all(r["success"] for r in refs) and early >= 40
    got = host_estimate(tracks, tmp_path)
    for (t, o), r, g, ok in zip(tracks, refs, got, stable):
        if ok:
            assert tref.discrete(g) == tref.discrete(r)
            assert np.abs(g["xyz"] - r["xyz"]).max() <= 1e-9 * max(1.0, np.linalg.norm(r["xyz"]))


def test_host_block_under_sanitizers(tmp_path):
    """The same stand-alone program built with AddressSanitizer and UBSan, run
    as a child process of its own (nothing is preloaded, nothing is loaded
    into Python).  A machine with a visible GPU builds it but does not run it."""
    binary = make("triangulation_block_test_san")
    try:
        if M.device_count() > 0:
            return
    except Exception:
        pass
    names = ["len3", "len16", "len30_outliers", "len40_outliers_reproj", "len9_derived_reproj", "parallel", "behind"]
    san = host_results(names, tmp_path, "triangulation_block_test_san")
    plain = host_results(names, tmp_path)
    for k in names:
        assert tref.discrete(san[k]) == tref.discrete(plain[k]), k
    assert os.path.exists(binary)


def test_triangulation_facade_host():
    """Defaults, Check(), the size checks and the reference's known answers on the single-item functions."""
    assert run_program("triangulation_test", "host").count("PASS") == 3


# --------------------------------------------------------------------------- GPU
def device_run(tracks, **kw):
    o = tc.device_options(tracks[0][1], **kw)
    r = M.estimate_triangulation_batch(o, *tc.pack(tracks))
    return [dict(success=bool(r.success[k]), num_trials=int(r.num_trials[k]), num_inliers=int(r.num_inliers[k]),
                 best_is_local=bool(r.best_is_local[k]), xyz=r.xyz[k] if r.success[k] else None,
                 mask=r.inlier_mask[k] if r.success[k] else None) for k in range(len(tracks))], r


@pytest.fixture(scope="module")
def device_results(gpu):
    """Every case through the device, one launch per option set; computed once."""
    got = {}
    for key, ks in grouped(all_case_names()).items():
        derived = [k for k in ks if "derived" in k]
        plain = [k for k in ks if "derived" not in k]
        if plain:
            got.update(zip(plain, device_run([tc.solved(k)[:2] for k in plain])[0]))
        if derived:  # point_normalized left out: derived on the device from the pixels
            tracks = []
            for k in derived:
                t, o = tc.solved(k)[:2]
                tracks.append((tref.Track(t.proj, t.centers, None, t.points, t.camera, t.cameras), o))
            got.update(zip(derived, device_run(tracks)[0]))
    return got


@pytest.mark.gpu
@pytest.mark.parametrize("category", list(CATEGORIES) + ["capacity"])
def test_device_matches_reference(device_results, category):
    """The device against the restatement, decision for decision: track
    lengths 2, 3, 4, 15, 16, 64, 65, the LDS capacity and one more, both
    residual types, mixed cameras, point_normalized given and derived, 20 %
    outliers, a binding trial cap, 64 and 65 trials (one speculation round and
    one trial more), min_num_trials per track, and the failing tracks."""
    names = (CATEGORIES[category] if category != "capacity"
             else list(tc.capacity_cases(M.triangulation_lds_capacity())))
    compared = {k: check_against_reference(k, device_results[k]) for k in names}
    assert any(compared.values()), "no stable case left in " + category


@pytest.mark.gpu
def test_device_stability_cap(device_results):
    names = all_case_names()
    assert_stability_cap({k: tc.solved(k)[3] for k in names})
    # the masked num_inliers equals the mask's popcount
    for k in names:
        g = device_results[k]
        if g["success"]:
            assert int(g["mask"].sum()) == g["num_inliers"], k


@pytest.mark.gpu
def test_failing_tracks_leave_outputs_untouched(gpu):
    """All rays nearly parallel under min_tri_angle 1.5 degrees, a point behind
    one camera, two views that disagree beyond max_error: success 0, xyz and
    the mask as the caller left them; a good track between them is written."""
    tracks = [tc.solved(k)[:2] for k in ("parallel", "len4", "behind", "disagree")]
    s = {}
    assert estimate_status(tracks, tc.device_options(tracks[0][1]), sentinel=s) == M.OK
    assert list(s["success"]) == [0, 1, 0, 0]
    off = s["offsets"]
    for k in (0, 2, 3):
        assert np.all(s["xyz"][k] == 7.0) and np.all(s["mask"][off[k]:off[k + 1]] == 9)
    assert np.all(s["mask"][off[1]:off[2]] <= 1) and not np.any(s["xyz"][1] == 7.0)


@pytest.fixture(scope="module")
def batch257():
    rng = np.random.default_rng(11)
    lengths = rng.integers(2, 66, size=257)
    lengths[0] = lengths[256] = 23
    lengths[100] = M.triangulation_lds_capacity() + 3   # one streamed track inside
    tracks = [(tc.make_track(int(n), 9000 + k), tc.create_options(int(n))) for k, n in enumerate(lengths)]
    tracks[256] = tracks[0]
    return tracks


def same_bits(a, b):
    return (tref.discrete(a) == tref.discrete(b)
            and (a["xyz"] is None or np.array_equal(a["xyz"].view(np.uint64), b["xyz"].view(np.uint64))))


@pytest.mark.gpu
def test_batch_position_run_to_run_and_permutation(gpu, batch257):
    """A track gives identical bits alone, at both ends of a 257-track batch
    and on a second run; permuting the problems permutes the outputs; the
    inlier count is the mask's popcount."""
    first, raw = device_run(batch257)
    second, _ = device_run(batch257)
    alone, _ = device_run([batch257[0]])
    assert same_bits(alone[0], first[0]) and same_bits(alone[0], first[256])
    assert all(same_bits(a, b) for a, b in zip(first, second))
    perm = np.random.default_rng(5).permutation(len(batch257))
    shuffled, _ = device_run([batch257[i] for i in perm])
    assert all(same_bits(shuffled[j], first[i]) for j, i in enumerate(perm))
    assert sum(r["success"] for r in first) >= 250
    for r in first:
        if r["success"]:
            assert int(r["mask"].sum()) == r["num_inliers"]
    # the streamed track alone gives the bits it gives inside the batch
    assert same_bits(device_run([batch257[100]])[0][0], first[100])


@pytest.mark.gpu
def test_triangulate_points(gpu):
    """mi_ba_triangulate_points on the known-answer grid (below the
    reference's 1e-10) and on 1 000 random pairs against the restatement,
    with the xyz bound of the estimator; the angles within 1e-12."""
    worst = 0.0
    for P1, P2, x1, x2, pts in grid_pairs():
        xyz, ang = M.triangulate_points(P1, P2, x1, x2)
        assert ang is None
        worst = max(worst, float(np.linalg.norm(xyz - pts, axis=1).max()))
    print("grid on the device: worst error norm", worst)
    assert worst < 1e-10
    c1, c2 = np.zeros(3), np.array([0.0, 1, 0])
    _, ang = M.triangulate_points(proj_center1=c1, proj_center2=c2, xyz=[[0, 0, 100], [0, 0, 50], [0, 0, 0]])
    assert abs(ang[0] / 0.009999666687 - 1) <= 1e-10 and abs(ang[1] / 0.019997333973 - 1) <= 1e-10
    assert ang[2] >= 0.0
    # 1 000 random pairs: two cameras of a track, noisy projections of points 3 to 7 units away
    rng = np.random.default_rng(3)
    t = tc.make_track(2, 77, outliers=0.0)
    X = rng.uniform(-1, 1, size=(1000, 3))
    pn = []
    for P in t.proj:
        pc = X @ P[:, :3].T + P[:, 3]
        pn.append(pc[:, :2] / pc[:, 2:] + rng.normal(size=(1000, 2)) * tc.NOISE)
    xyz, ang = M.triangulate_points(t.proj[0], t.proj[1], pn[0], pn[1], t.centers[0], t.centers[1])
    want = np.array([tref.triangulate_point(t.proj[0], t.proj[1], a, b) for a, b in zip(*pn)])
    want_ang = np.array([tref.triangulation_angle(t.centers[0], t.centers[1], x) for x in want])
    # the restatement's own spread under one-ulp inputs, as for the estimator
    spread = 0.0
    for s in range(3):
        p = tc.perturbed(tref.Track(t.proj, t.centers, pn[0], pn[1], t.camera, t.cameras), None, 300 + s)
        moved = np.array([tref.triangulate_point(p.proj[0], p.proj[1], a, b) for a, b in zip(p.normalized, p.points)])
        spread = max(spread, float(np.abs(moved - want).max()))
    dx = np.abs(xyz - want).max(axis=1)
    bound = np.maximum(1e-9 * np.maximum(1.0, np.linalg.norm(want, axis=1)), 10 * spread)
    print("random pairs: max dxyz", dx.max(), "spread", spread, "max dangle", np.abs(ang - want_ang).max())
    assert np.all(dx <= bound) and np.abs(ang - want_ang).max() <= 1e-12


def write_track(track, o, path):
    """The text form tests/cpp/triangulation_test.cc reads."""
    with open(path, "w") as f:
        f.write(hexes([o.residual_type, o.min_tri_angle, o.max_error, o.confidence, o.min_inlier_ratio,
                       min(o.max_num_trials, 2 ** 53), o.min_num_trials, len(track.cameras)]) + "\n")
        for model, prm in track.cameras:
            f.write(hexes([model, len(prm), *prm]) + "\n")
        f.write(hexes([len(track)]) + "\n")
        for i in range(len(track)):
            f.write(hexes([track.camera[i], *track.points[i], *track.normalized[i], *track.proj[i].reshape(-1),
                           *track.centers[i]]) + "\n")


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["len16_reproj", "len30_outliers", "parallel"])
def test_triangulation_facade_gpu(gpu, tmp_path, name):
    """EstimateTriangulation with the reference's signature through the C++
    facade, alone and inside a batch, against the restatement."""
    track, o, ref, stable, bound = tc.solved(name)
    assert stable
    path = str(tmp_path / "track.txt")
    write_track(track, o, path)
    out = run_program("triangulation_test", "gpu", path)
    w = [l for l in out.splitlines() if l.startswith("RESULT")][0].split()
    assert (w[1] == "1") == ref["success"] and int(w[2]) == ref["num_trials"]
    if ref["success"]:
        xyz = np.array([float.fromhex(v) for v in w[3:6]])
        assert np.abs(xyz - ref["xyz"]).max() <= bound
        assert [c == "1" for c in w[6]] == list(ref["mask"])
