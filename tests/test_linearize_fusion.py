"""The linearization step with its bookkeeping kernels carried by their
neighbours' launches ("linearize_fusion", a bit mask: 1 the step prologue —
pair tables, image records, scalar zero fill and input warm-up in one launch;
2 the flat pass counts each pair's deferred samples and the ordering kernel
lays out the chunk list; 4 the pair blocks in the cost sums' launch) against
the ten separate launches (mask 0) and the oracle.

The fused launches call the same device bodies on the same inputs, integer
counts are summed behind a kernel boundary, and every floating-point sum keeps
its order, so status, residuals, Jacobians, pair blocks and a whole LM solve
must be equal bit for bit: no tolerance anywhere in this file.  Reference
values come from mask 0 and from oracle.semantic_eval.

The scene: 10 images with their own raster sizes (ABI 4), chosen so that the
pairs' sample counts (the first image's grid at pixel step 2) are 49, 64, 150,
256, 400, several thousand, and 17424 (more than 256 mask words: the ordering
kernel's loop runs twice).  Two camera models alternate over the images, so
the second images' models are interleaved in pair order and a model's pairs
are not contiguous.  Images 5-7 carry a fine label grid and depth steps (many
deferred samples), image 8 one label but for a small patch (a few), image 9 a
far depth (none).  test_coverage asserts these cases from the marks."""
import functools

import numpy as np
import pytest

import mi_ba

pytestmark = pytest.mark.gpu

I = 10
STEP = 2
FULL = 264
# (H, W) of images 0..9; samples per pair with this first image: ceil(H / 2) * ceil(W / 2)
SIZES = [(14, 14), (16, 16), (20, 30), (32, 32), (40, 40), (264, 264), (160, 160), (120, 160), (160, 100), (90, 130)]
MODELS = [mi_ba.SIMPLE_RADIAL, mi_ba.OPENCV]
PAIRS = np.array([(i, (i + 1) % I) for i in range(I)] + [(i, (i + 3) % I) for i in range(I)] +
                 [(5, 7), (7, 5), (6, 5), (8, 5)], np.int32)
MASKS = (0, 1, 2, 4, 7)


def crop(maps):
    return [np.ascontiguousarray(m[:h, :w]) for m, (h, w) in zip(maps, SIZES)]


def build():
    sc = mi_ba.generate_scene(mi_ba.synth_config(mi_ba.SIMPLE_RADIAL, I, 300, track_length=4, image_size=FULL,
                                                 rotation_range=0.05, extra=(0.05, 0, 0, 0), seed=3))
    sc = mi_ba.convert_cameras(sc, MODELS).gauge()
    sc.camera_constant = np.ones(sc.num_cameras, np.uint8)
    depth, label = mi_ba.render_semantic(sc, FULL, FULL, cell=0.05)
    depth, label = depth.copy(), label.copy()
    depth[5:8, 40:44, :] *= 1.5      # depth steps
    depth[5:8, :, 100:103] *= 0.6
    label[:5] = 3.0
    label[8] = 3.0
    label[8, 70:80, 70:80] = 4.0     # a few deferred samples around the patch
    label[9] = 3.0
    depth[9] = 100.0                 # never within the threshold: every outcome 0
    sc.tvec[3:] += 0.003
    return sc, mi_ba.SemanticInput(crop(depth), crop(label), PAIRS, pixel_step=STEP)


def frozen(out):
    for x in out:
        x.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def evaluate(mask):
    sc, sem = build()
    with mi_ba.Context(mi_ba.default_options(), sc.copy(), sem) as ctx:
        ctx.set_tuning("linearize_fusion", mask)
        ctx.set_tuning("semantic_diag", 2)
        ctx.evaluate_semantic()
        return frozen(ctx.download_semantic())


def decode(st):
    """status -> (plain status, deferred +0x1000, redone per point +0x10000)"""
    t = st.astype(np.int64) + 2   # the plain statuses are -2, -1, 10
    return ((t & 0xFFF) - 2).astype(np.int32), ((t >> 12) & 1).astype(bool), (t >> 16).astype(bool)


def bits(x):
    return np.ascontiguousarray(x).view(np.uint64)


def assert_samples_equal(a, b):
    for x, y in zip(a[:2], b[:2]):     # pixels, status with its marks
        assert np.array_equal(x, y)
    for x, y in zip(a[2:], b[2:]):     # r, J
        assert np.array_equal(bits(x), bits(y))


def test_coverage(gpu):
    """The cases the tests below are meant to run through, from mask 0's marks."""
    px, st, r, J = evaluate(0)
    _, deferred, _ = decode(st)
    samples = np.bincount(px[:, 0], minlength=len(PAIRS))
    per_pair = np.bincount(px[:, 0][deferred], minlength=len(PAIRS))
    print("samples per pair", samples.tolist())
    print("deferred per pair", per_pair.tolist())
    assert ((samples > 0) & (samples < 64)).any()
    assert (samples == 64).any()
    assert ((samples >= 65) & (samples <= 255)).any()
    assert (samples == 256).any()
    assert ((samples >= 257) & (samples < 4096)).any()
    assert (samples > 256 * 64).any()                        # the ordering kernel's loop runs twice
    assert (per_pair == 0).any()                             # a pair with no chunk
    assert ((per_pair >= 1) & (per_pair <= 63)).any()        # one partial chunk
    assert ((per_pair > 64) & (per_pair % 64 != 0)).any()    # several chunks, the last one partial
    # both models among the second images, interleaved in pair order
    sc, _ = build()
    second = sc.camera_models[sc.image_camera[PAIRS[:, 1]]]
    assert set(second.tolist()) == set(MODELS)
    for m in MODELS:
        idx = np.flatnonzero(second == m)
        assert np.any(np.diff(idx) > 1)                      # the model's pairs are not contiguous
        assert per_pair[idx].sum() > 64                      # and it has deferred chunks to list


@pytest.mark.parametrize("mask", [2, 7])
def test_evaluate_semantic_equals_separate_launches(gpu, mask):
    assert_samples_equal(evaluate(0), evaluate(mask))


def test_evaluate_semantic_equals_oracle(gpu):
    import oracle
    sc, sem = build()
    px_o, st_o, r_o, J_o = oracle.semantic_eval(mi_ba.default_options(), sc, sem)
    px, st, r, J = evaluate(7)
    plain, _, _ = decode(st)
    bad = (plain != st_o) | (bits(r) != bits(r_o)) | np.any(bits(J) != bits(J_o), axis=1)
    print(f"{int(bad.sum())} of {len(bad)} samples differ from the oracle")
    assert np.array_equal(px, px_o)
    assert not bad.any()


def lm_scene():
    sc, sem = build()
    sc.camera_constant = None        # intrinsics variable
    return sc, sem


LM = dict(max_num_iterations=3, semantic_weight=0.1)


def solve(mask, keys=(), scene=None):
    sc, sem = scene if scene is not None else lm_scene()
    b = sc.copy()
    with mi_ba.Context(mi_ba.default_options(**LM), b, sem) as ctx:
        ctx.set_tuning("linearize_fusion", mask)
        for k, v in keys:
            ctx.set_tuning(k, v)
        s = ctx.solve()
        ctx.writeback()
    return s, b


@functools.lru_cache(maxsize=None)
def solve_separate():
    return solve(0)


def assert_solves_equal(ref, got):
    (s0, a), (s, x) = ref, got
    assert (s.num_successful_steps, s.num_unsuccessful_steps) == (s0.num_successful_steps, s0.num_unsuccessful_steps)
    assert s.initial_cost == s0.initial_cost and s.final_cost == s0.final_cost
    for key in ("qvec", "tvec", "xyz", "camera_params"):
        assert np.array_equal(bits(getattr(a, key)), bits(getattr(x, key))), key


@pytest.mark.parametrize("mask", [1, 2, 4, 7, 7])
def test_lm_bitwise(gpu, mask):
    """Three LM iterations: the prologue's image records and scalar zero fill,
    the pair blocks and the epilogue's sums drive every accept / reject
    decision and the final parameters (mask 7 twice: the same run to run)."""
    s0, _ = solve_separate()
    print("LM", s0.num_successful_steps, s0.num_unsuccessful_steps, s0.initial_cost, s0.final_cost)
    assert s0.num_semantic_residuals > 0 and s0.num_residuals_reduced > 0
    assert s0.num_successful_steps + s0.num_unsuccessful_steps >= 3
    assert_solves_equal(solve_separate(), solve(mask))


def linearized(ctx):
    ctx.linearize()
    return frozen(ctx.download_jacobian())


def assert_jacobians_equal(a, b):
    assert np.array_equal(a[0], b[0])
    assert np.array_equal(bits(a[1]), bits(b[1])) and np.array_equal(bits(a[2]), bits(b[2]))


@functools.lru_cache(maxsize=None)
def jacobian_separate():
    sc, sem = lm_scene()
    with mi_ba.Context(mi_ba.default_options(**LM), sc.copy(), sem) as ctx:
        ctx.set_tuning("linearize_fusion", 0)
        return linearized(ctx)


def test_linearize_jacobian_bitwise(gpu):
    sc, sem = lm_scene()
    with mi_ba.Context(mi_ba.default_options(**LM), sc.copy(), sem) as ctx:
        ctx.set_tuning("linearize_fusion", 7)
        got = linearized(ctx)
    assert len(got[0]) > 0
    assert_jacobians_equal(jacobian_separate(), got)


def test_state_reuse(gpu):
    """One context through both routes in turn: the counters and lists are
    re-zeroed by whichever route runs."""
    sc, sem = lm_scene()
    b = sc.copy()
    with mi_ba.Context(mi_ba.default_options(**LM), b, sem) as ctx:
        ctx.set_tuning("semantic_diag", 2)
        ctx.set_tuning("linearize_fusion", 7)
        ctx.evaluate_semantic()
        first = frozen(ctx.download_semantic())
        for _ in range(3):
            assert_jacobians_equal(jacobian_separate(), linearized(ctx))
        ctx.set_tuning("linearize_fusion", 0)
        assert_jacobians_equal(jacobian_separate(), linearized(ctx))
        ctx.set_tuning("linearize_fusion", 7)
        assert_jacobians_equal(jacobian_separate(), linearized(ctx))
        ctx.evaluate_semantic()
        assert_samples_equal(first, ctx.download_semantic())
        s = ctx.solve()
        ctx.writeback()
    assert_samples_equal(evaluate(0), first)         # camera_constant does not enter the samples
    assert_solves_equal(solve_separate(), (s, b))


def geometric_only():
    sc, _ = lm_scene()
    return sc, None


def semantic_only():
    sc, sem = build()                                 # intrinsics constant
    sc.obs_xy, sc.obs_image, sc.obs_point = sc.obs_xy[:0], sc.obs_image[:0], sc.obs_point[:0]
    return sc, sem


@pytest.mark.parametrize("case", ["warm_off", "geometric_only", "semantic_only", "compact_off", "one_wave"])
def test_fallbacks(gpu, case):
    """Where the fused forms do not apply the separate launches run under
    mask 7 too."""
    keys = {"warm_off": (("linearize_warm_inputs", 0),), "compact_off": (("semantic_deferred_compact", 0),),
            "one_wave": (("semantic_deferred_waves", 1),)}.get(case, ())
    scene = {"geometric_only": geometric_only, "semantic_only": semantic_only}.get(case, lm_scene)()
    ref = solve(0, keys, scene)
    got = solve(7, keys, scene)
    print(case, ref[0].num_successful_steps, ref[0].num_unsuccessful_steps, ref[0].initial_cost, ref[0].final_cost)
    assert ref[0].initial_cost > 0
    assert_solves_equal(ref, got)
    if case in ("warm_off", "compact_off", "one_wave"):
        assert_solves_equal(solve_separate(), got)   # these keys do not change a bit either


def test_more_pairs_than_the_order_kernel_takes(gpu):
    """70 images of 8 x 8 rasters with every ordered pair: 4830 pairs of one
    model, above the ordering kernel's cap of 4096, so the separate ordering
    and compaction kernels run under mask 7."""
    n = 70
    sc = mi_ba.generate_scene(mi_ba.synth_config(mi_ba.OPENCV, n, 400, track_length=4, image_size=8, noise=0.05,
                                                 rotation_range=0.02, extra=(-0.1, 0.01, 1e-4, -1e-4), seed=5)).gauge()
    depth, label = mi_ba.render_semantic(sc, 8, 8, cell=0.05)
    pairs = np.array([(i, j) for i in range(n) for j in range(n) if i != j], np.int32)
    assert len(pairs) > 4096
    sem = mi_ba.SemanticInput(depth, label, pairs, pixel_step=4)
    sc.tvec[3:] += 0.003
    out = []
    for mask in (0, 7):
        b = sc.copy()
        with mi_ba.Context(mi_ba.default_options(**LM), b, sem) as ctx:
            ctx.set_tuning("linearize_fusion", mask)
            jac = linearized(ctx)
            s = ctx.solve()
            ctx.writeback()
        assert s.num_semantic_residuals >= 4 * len(pairs) // 2
        out.append((jac, (s, b)))
    assert_jacobians_equal(out[0][0], out[1][0])
    assert_solves_equal(out[0][1], out[1][1])
