"""The semantic pass with one workgroup per image pair ("semantic_pair_fused"
1: semantic_pair_kernel runs the pair's flat test tile by tile, keeps the
pair's deferred list to itself, runs the stencil chunks on it and sums the
pair block) against the five-kernel route (key 0: flat pass, ordering,
compaction, four-wave deferred pass, pair sums).

The fused kernel calls the same device bodies on the same inputs, appends the
deferred samples in the ordering kernel's order and sums the chunk rows in
chunk order, so every output must be equal bit for bit: no tolerance anywhere
in this file.  The fused route runs only where the step writes no samples, so
its pair blocks, tile partials and semantic cost have no download of their
own (as in test_linearize_fusion.py); they are pinned through what they
drive: linearize() and then solve() with two LM iterations (initial cost,
every accept / reject decision, final cost, final parameters).  That the
fused kernel really ran is read from the launch count the context keeps under
"semantic_pair_fused" while timing is on.  Against the oracle the standard is
the existing semantic tests' (bitwise samples): evaluate_semantic writes
samples, so under key 1 it takes the five-kernel route, and that fallback is
what the oracle comparison and test_evaluate_semantic_falls_back pin.

Scenes: 8 images of 64 x 64 (cropped from a 72 x 72 render), every pixel's
label drawn from two values, so a sample is deferred whenever its stencil's
pixel box spans both; the numeric step 1e-2 makes that box wider than one
pixel for most samples (a hundred or more deferred samples in most pairs).
Pixel step 3 gives 484 samples per pair (one full tile and a ragged one), step
4 exactly 256 (one tile); the
mixed-size scene (48 x 72 against 66 x 54) gives 216 / 238 (a partial tile)
and 384 / 396.  Images 4 and 5 carry one label and image 5 a far depth: pair
(4, 5) has no deferred sample.  The gauge fixes image 0's pose (a pair with a
constant pose on its first side, one on its second) and one coordinate of
image 1's tvec; "pose" / "tvec" add more of both.  "semantic_pair_min_pairs" 0
lets these few pairs take the fused route (the default asks for a resident
grid's worth), "semantic_pair_list_cap" shortens the list's LDS part so that
the pair's dlist region carries the rest."""
import functools

import numpy as np
import pytest

import mi_ba

pytestmark = pytest.mark.gpu

I = 8
FULL = 72
MODELS = [mi_ba.SIMPLE_PINHOLE, mi_ba.PINHOLE, mi_ba.SIMPLE_RADIAL, mi_ba.RADIAL, mi_ba.OPENCV]
PAIRS = np.array([(0, 1), (2, 3), (4, 5), (6, 7), (1, 2), (3, 0), (5, 6), (7, 4)], np.int32)
PAIR_NONE = 2                 # (4, 5): one label, far depth in the second image
PAIR64, PAIR65 = 1, 3         # (2, 3) and (6, 7): no image in common
SQUARE = [(64, 64)] * I
MIXED = [(48, 72), (66, 54)] + [(64, 64)] * (I - 2)
REL = 1e-2
FAR = 100.0
LM = dict(max_num_iterations=2, semantic_weight=0.1)
FORMS = {"lp": (), "ws": (("semantic_label_planes", 0),),
         "plain": (("semantic_label_planes", 0), ("semantic_window_summary", 0))}


def bits(x):
    return np.ascontiguousarray(np.asarray(x, np.float64)).view(np.uint64)


def frozen(out):
    for x in out:
        x.setflags(write=False)
    return out


def build(models, step, flags="gauge", sizes=SQUARE, rel=REL, lm=False):
    sc = mi_ba.generate_scene(mi_ba.synth_config(mi_ba.SIMPLE_RADIAL, I, 150, track_length=4, image_size=FULL,
                                                 rotation_range=0.05, extra=(0.05, 0, 0, 0), seed=7))
    sc = mi_ba.convert_cameras(sc, list(models)).gauge()
    if flags != "gauge":
        sc.image_constant_pose = np.zeros(I, np.uint8)
        sc.image_constant_tvec = np.zeros(I, np.uint8)
    if flags == "pose":
        sc.image_constant_pose[2] = 1
        sc.image_constant_pose[7] = 1
    if flags == "tvec":
        for i, m in {1: 0b101, 3: 0b010, 6: 0b111}.items():
            sc.image_constant_tvec[i] = m
    if not lm:
        sc.camera_constant = np.ones(sc.num_cameras, np.uint8)
    depth, _ = mi_ba.render_semantic(sc, FULL, FULL, cell=0.05)
    depth = depth.copy()
    label = np.random.default_rng(11).integers(3, 5, size=depth.shape).astype(np.float32)
    label[4:6] = 3.0
    depth[5] = FAR
    sc.tvec[3:] += 0.003
    if sizes is SQUARE:
        depth, label = np.ascontiguousarray(depth[:, :64, :64]), np.ascontiguousarray(label[:, :64, :64])
    else:
        depth = [np.ascontiguousarray(d[:h, :w]) for d, (h, w) in zip(depth, sizes)]
        label = [np.ascontiguousarray(m[:h, :w]) for m, (h, w) in zip(label, sizes)]
    return sc, mi_ba.SemanticInput(depth, label, PAIRS, pixel_step=step, numeric_relative_step_size=rel)


def decode(st):
    """status -> (plain status, deferred +0x1000)"""
    t = st.astype(np.int64) + 2   # the plain statuses are -2, -1, 10
    return ((t & 0xFFF) - 2).astype(np.int32), ((t >> 12) & 1).astype(bool)


def marks(sc, sem, keys=()):
    """Samples and deferred samples per pair, from the five-kernel route's marks."""
    with mi_ba.Context(mi_ba.default_options(), sc.copy(), sem) as ctx:
        for k, v in keys:
            ctx.set_tuning(k, v)
        ctx.set_tuning("semantic_diag", 2)
        ctx.evaluate_semantic()
        px, st, _, _ = ctx.download_semantic()
    _, deferred = decode(st)
    return (np.bincount(px[:, 0], minlength=len(PAIRS)), np.bincount(px[:, 0][deferred], minlength=len(PAIRS)),
            px, deferred)


def run(sc, sem, fused, keys=(), cap=None):
    """linearize() and its Jacobian, then two LM iterations, on one context."""
    b = sc.copy()
    with mi_ba.Context(mi_ba.default_options(**LM), b, sem) as ctx:
        for k, v in keys:
            ctx.set_tuning(k, v)
        ctx.set_tuning("semantic_pair_fused", fused)
        ctx.set_tuning("semantic_pair_min_pairs", 0)
        if cap is not None:
            ctx.set_tuning("semantic_pair_list_cap", cap)
        ctx.set_timing(True)
        ctx.linearize()
        jac = frozen(ctx.download_jacobian())
        launches = ctx.kernel_time("semantic_pair_fused")[1]
        ctx.set_timing(False)
        s = ctx.solve()
        ctx.writeback()
    return jac, s, b, launches


def assert_runs_equal(ref, got):
    (j0, s0, a, n0), (j, s, x, n) = ref, got
    assert n0 == 0 and n > 0                      # the five-kernel route / the fused kernel ran
    assert np.array_equal(j0[0], j[0])
    assert np.array_equal(bits(j0[1]), bits(j[1])) and np.array_equal(bits(j0[2]), bits(j[2]))
    assert s0.num_semantic_residuals > 0 and s0.initial_cost > 0
    assert (s.num_successful_steps, s.num_unsuccessful_steps) == (s0.num_successful_steps, s0.num_unsuccessful_steps)
    assert np.array_equal(bits([s.initial_cost, s.final_cost]), bits([s0.initial_cost, s0.final_cost]))
    for key in ("qvec", "tvec", "xyz", "camera_params"):
        assert np.array_equal(bits(getattr(a, key)), bits(getattr(x, key))), key


def check(sc, sem, keys=(), caps=(None,)):
    ref = run(sc, sem, 0, keys)
    print("LM", ref[1].num_successful_steps, ref[1].num_unsuccessful_steps, ref[1].initial_cost, ref[1].final_cost)
    for cap in caps:
        assert_runs_equal(ref, run(sc, sem, 1, keys, cap))


@pytest.mark.parametrize("model", MODELS)
def test_each_model(gpu, model):
    """484 samples per pair: a full tile and a ragged one; pairs with none,
    one partial and several chunks; constant poses and a tvec mask (gauge)."""
    sc, sem = build([model], 3, lm=True)
    samples, counts, _, _ = marks(sc, sem)
    print("samples per pair", samples.tolist(), "deferred per pair", counts.tolist())
    assert (samples == 484).all()
    assert counts[PAIR_NONE] == 0
    assert (counts > 64).any() and ((counts > 64) & (counts % 64 != 0)).any()
    check(sc, sem, caps=(None, 16))


@pytest.mark.parametrize("flags", ["pose", "tvec"])
def test_constant_pose_and_tvec(gpu, flags):
    sc, sem = build([mi_ba.OPENCV], 3, flags, lm=True)
    check(sc, sem)


@pytest.mark.parametrize("form", ["ws", "plain"])
def test_flat_forms(gpu, form):
    """The window-summary and the plain form of the flat body."""
    sc, sem = build([mi_ba.OPENCV], 3, lm=True)
    check(sc, sem, FORMS[form])


@pytest.mark.parametrize("step,sizes", [(4, "square"), (4, "mixed"), (3, "mixed")])
def test_tile_shapes(gpu, step, sizes):
    """Exactly one tile (256 samples); a partial tile (216 / 238); 384 / 396."""
    sc, sem = build([mi_ba.OPENCV], step, sizes=SQUARE if sizes == "square" else MIXED, lm=True)
    samples, counts, _, _ = marks(sc, sem)
    print("samples per pair", samples.tolist(), "deferred per pair", counts.tolist())
    if sizes == "square":
        assert (samples == 256).all()
    elif step == 4:
        assert samples[0] == 216 and samples[4] == 238
    else:
        assert samples[0] == 384 and samples[4] == 396
    assert counts.sum() > 0
    check(sc, sem)


def test_two_models(gpu):
    """Two models alternate over the cameras: each model's pairs are a
    scattered subset of the pair list, one launch per model."""
    sc, sem = build([mi_ba.SIMPLE_RADIAL, mi_ba.OPENCV], 3, lm=True)
    second = sc.camera_models[sc.image_camera[PAIRS[:, 1]]]
    assert set(second.tolist()) == {mi_ba.SIMPLE_RADIAL, mi_ba.OPENCV}
    check(sc, sem, caps=(None, 16))


@functools.lru_cache(maxsize=None)
def edge_scene():
    """All but the first 64 deferred samples of pair PAIR64, and all but the
    first 65 of pair PAIR65, moved far away in their first image's depth map:
    the flat test then settles them."""
    sc, sem = build([mi_ba.OPENCV], 3, lm=True)
    _, counts, px, deferred = marks(sc, sem)
    depth = np.array(sem.depth, np.float32, copy=True)
    for pair, keep in ((PAIR64, 64), (PAIR65, 65)):
        rows = np.flatnonzero(deferred & (px[:, 0] == pair))
        assert len(rows) > keep, counts.tolist()
        drop = rows[keep:]
        depth[PAIRS[pair, 0], px[drop, 2], px[drop, 1]] = FAR
    return sc, mi_ba.SemanticInput(depth, sem.label, PAIRS, pixel_step=3, numeric_relative_step_size=REL)


def test_chunk_edge(gpu):
    """A pair with exactly 64 deferred samples (one full chunk) and one with
    exactly 65 (a one-row second chunk); the list's LDS part ends at 64."""
    sc, sem = edge_scene()
    _, counts, _, _ = marks(sc, sem)
    print("deferred per pair", counts.tolist())
    assert counts[PAIR64] == 64 and counts[PAIR65] == 65 and counts[PAIR_NONE] == 0
    check(sc, sem, caps=(None, 64, 0))


def test_every_sample_deferred(gpu):
    """A numeric step of 0.5 puts every stencil outside the flat test's reach:
    all 484 samples of a pair are deferred, and with 16 list entries in LDS
    the other 468 go through the pair's dlist region."""
    sc, sem = build([mi_ba.OPENCV], 3, rel=0.5, lm=True)
    samples, counts, _, _ = marks(sc, sem)
    print("samples per pair", samples.tolist(), "deferred per pair", counts.tolist())
    assert (samples == 484).all() and (counts == samples).all()
    check(sc, sem, caps=(None, 16))


def test_state_reuse(gpu):
    """One context through both routes in turn."""
    sc, sem = build([mi_ba.OPENCV], 3, lm=True)
    with mi_ba.Context(mi_ba.default_options(**LM), sc.copy(), sem) as ctx:
        ctx.set_tuning("semantic_pair_min_pairs", 0)
        out = []
        for fused in (0, 1, 1, 0, 1):
            ctx.set_tuning("semantic_pair_fused", fused)
            ctx.linearize()
            out.append(frozen(ctx.download_jacobian()))
        for j in out[1:]:
            assert np.array_equal(bits(out[0][1]), bits(j[1])) and np.array_equal(bits(out[0][2]), bits(j[2]))


def test_few_pairs_fall_back(gpu):
    """Without "semantic_pair_min_pairs" eight pairs are fewer than a resident
    grid: key 1 takes the five-kernel route."""
    sc, sem = build([mi_ba.OPENCV], 3, lm=True)
    with mi_ba.Context(mi_ba.default_options(**LM), sc.copy(), sem) as ctx:
        ctx.set_tuning("semantic_pair_fused", 1)
        ctx.set_timing(True)
        ctx.linearize()
        assert ctx.kernel_time("semantic_pair_fused")[1] == 0
        assert ctx.kernel_time("semantic_jacobian")[1] == 1


@functools.lru_cache(maxsize=None)
def evaluated(model, fused):
    sc, sem = build([model], 3)
    with mi_ba.Context(mi_ba.default_options(), sc.copy(), sem) as ctx:
        ctx.set_tuning("semantic_pair_fused", fused)
        ctx.set_tuning("semantic_pair_min_pairs", 0)
        ctx.set_timing(True)
        ctx.evaluate_semantic()
        assert ctx.kernel_time("semantic_pair_fused")[1] == 0    # samples to write: the five-kernel route
        return frozen(ctx.download_semantic())


def test_evaluate_semantic_falls_back(gpu):
    a, b = evaluated(mi_ba.OPENCV, 0), evaluated(mi_ba.OPENCV, 1)
    for x, y in zip(a[:2], b[:2]):
        assert np.array_equal(x, y)
    for x, y in zip(a[2:], b[2:]):
        assert np.array_equal(bits(x), bits(y))


@pytest.mark.parametrize("model", MODELS)
def test_oracle(gpu, model):
    import oracle
    sc, sem = build([model], 3)
    px_o, st_o, r_o, J_o = oracle.semantic_eval(mi_ba.default_options(), sc, sem)
    px, st, r, J = evaluated(model, 1)
    bad = (st != st_o) | (bits(r) != bits(r_o)) | np.any(bits(J) != bits(J_o), axis=1)
    print(f"{int(bad.sum())} of {len(bad)} samples differ from the oracle")
    assert np.array_equal(px, px_o)
    assert not bad.any()
