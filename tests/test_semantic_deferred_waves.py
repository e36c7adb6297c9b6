"""The deferred semantic pass with one wave per stencil parameter group
("semantic_deferred_waves" 4: semantic_deferred_waves_kernel) against the
one-wave kernel (1) and the oracle.

Every stencil point is evaluated by the same device functions with the same
inputs, each tangent column is accumulated inside one wave in the one-wave
kernel's order, and the chunk sums are formed over the same rows in the same
order, so status, residual, Jacobian, pair blocks and with them a whole LM
solve must be equal bit for bit: no tolerance anywhere in this file.

The scene: 8 images of 160 x 160, a fine label grid and depth steps in images
0-3 (many deferred samples), images 4 and 5 with one label but for a small
patch in image 5 (a pair with a few deferred samples), images 6 and 7 with one
label and one far depth (pairs with no deferred sample).  test_coverage
asserts from the diagnostic marks that these cases are really present."""
import functools

import numpy as np
import pytest

import mi_ba

pytestmark = pytest.mark.gpu

EXTRA = {mi_ba.SIMPLE_PINHOLE: (), mi_ba.SIMPLE_RADIAL: (0.05,), mi_ba.OPENCV: (-0.1, 0.01, 1e-4, -1e-4)}
MODELS = [mi_ba.SIMPLE_PINHOLE, mi_ba.SIMPLE_RADIAL, mi_ba.OPENCV]
I = 8
PAIRS = np.array([(i, (i + 1) % I) for i in range(I)] + [(i, (i + 3) % I) for i in range(I)], np.int32)
# Chosen on the GPU with the one-wave kernel so that it redoes samples per
# point (+0x10000: a stencil point inside a margin).  With the gauge flags it
# deferred 2700 / 2696 / 2640 of the 102400 samples and redid 3 / 1 / 4 of
# them for SIMPLE_PINHOLE / SIMPLE_RADIAL / OPENCV; OPENCV's deferred samples
# per pair: 569 571 626 11 0 0 21 0 565 12 12 0 0 253 0 0.
SEED, STEP, CELL = 1, 2, 0.05
CONST_POSE = 2               # flags "pose": this image's pose is constant
CONST_TVEC = {1: 0b101, 3: 0b010, 6: 0b111}  # flags "tvec": image -> constant tvec coordinates


def build(model, flags="gauge", seed=None, step=None, cell=None):
    seed = SEED if seed is None else seed
    step = STEP if step is None else step
    cell = CELL if cell is None else cell
    sc = mi_ba.generate_scene(mi_ba.synth_config(model, I, 200, track_length=3, image_size=160, rotation_range=0.05,
                                                 extra=EXTRA[model], seed=seed)).gauge()
    if flags != "gauge":
        sc.image_constant_pose = np.zeros(I, np.uint8)
        sc.image_constant_tvec = np.zeros(I, np.uint8)
    if flags == "pose":
        sc.image_constant_pose[CONST_POSE] = 1
    if flags == "tvec":
        for i, m in CONST_TVEC.items():
            sc.image_constant_tvec[i] = m
    sc.camera_constant = np.ones(I, np.uint8)
    depth, label = mi_ba.render_semantic(sc, 160, 160, cell=cell)
    depth, label = depth.copy(), label.copy()
    depth[:4, 40:44, :] *= 1.5      # depth steps
    depth[:4, :, 100:103] *= 0.6
    label[4:] = 3.0
    label[5, 70:80, 70:80] = 4.0    # a few deferred samples around the patch
    depth[6:] = 100.0               # never within the threshold: every outcome 0
    sc.tvec[3:] += 0.003
    return sc, mi_ba.SemanticInput(depth, label, PAIRS, pixel_step=step)


@functools.lru_cache(maxsize=None)
def evaluate(model, flags, waves):
    sc, sem = build(model, flags)
    with mi_ba.Context(mi_ba.default_options(), sc.copy(), sem) as ctx:
        ctx.set_tuning("semantic_deferred_waves", waves)
        ctx.set_tuning("semantic_diag", 2)
        ctx.evaluate_semantic()
        out = ctx.download_semantic()
    for x in out:
        x.setflags(write=False)
    return out


def decode(st):
    """status -> (plain status, deferred +0x1000, redone per point +0x10000)"""
    t = st.astype(np.int64) + 2   # the plain statuses are -2, -1, 10
    return ((t & 0xFFF) - 2).astype(np.int32), ((t >> 12) & 1).astype(bool), (t >> 16).astype(bool)


def assert_routes_equal(model, flags):
    a, b = evaluate(model, flags, 1), evaluate(model, flags, 4)
    px_a, st_a, r_a, J_a = a
    px_b, st_b, r_b, J_b = b
    assert np.array_equal(px_a, px_b)
    pa, da, ra = decode(st_a)
    pb, db, rb = decode(st_b)
    print(f"model {model} flags {flags}: samples {len(st_a)} deferred {int(da.sum())} redone {int(ra.sum())} / "
          f"{int(rb.sum())} nonzero J rows {int((np.abs(J_a).sum(axis=1) > 0).sum())}")
    assert np.array_equal(pa, pb)
    assert np.array_equal(da, db)
    # a sample redone by the one-wave kernel had some group inside a margin:
    # that group is redone here too (and no group of any other sample)
    assert np.array_equal(ra, rb)
    assert np.array_equal(r_a.view(np.uint64), r_b.view(np.uint64))
    assert J_a.shape[1] == 12
    assert np.array_equal(J_a.view(np.uint64), J_b.view(np.uint64))
    assert da.sum() > 1000 and (np.abs(J_b).sum(axis=1) > 0).sum() > 100
    return b


@pytest.mark.parametrize("model", MODELS)
def test_old_route_against_new(gpu, model):
    assert_routes_equal(model, "gauge")


def plus_zero(x):
    return np.all(x.view(np.uint64) == 0)


@pytest.mark.parametrize("flags", ["all", "pose", "tvec"])
def test_pose_flags(gpu, flags):
    """Every pose variable; one image's pose constant; constant tvec
    coordinates: a constant pose's columns are +0.0 exactly (sign bit clear)."""
    px, st, r, J = assert_routes_equal(mi_ba.OPENCV, flags)
    i1, i2 = PAIRS[px[:, 0], 0], PAIRS[px[:, 0], 1]
    moving = np.abs(J).sum(axis=0) > 0
    if flags == "all":
        assert moving.all()   # every one of the 12 columns is in use
    if flags == "pose":
        assert (i1 == CONST_POSE).any() and (i2 == CONST_POSE).any()
        assert plus_zero(J[i1 == CONST_POSE, 0:6])
        assert plus_zero(J[i2 == CONST_POSE, 6:12])
        assert np.abs(J[i1 != CONST_POSE, 0:6]).sum() > 0 and np.abs(J[i2 != CONST_POSE, 6:12]).sum() > 0
    if flags == "tvec":
        for img, mask in CONST_TVEC.items():
            for k in range(3):
                if (mask >> k) & 1:
                    assert plus_zero(J[i1 == img, 3 + k])
                    assert plus_zero(J[i2 == img, 9 + k])
        assert moving[0:3].all() and moving[6:9].all()   # the rotations stay variable
    # the gauge flags (test_old_route_against_new): image 0's pose, image 1's first tvec coordinate
    px, st, r, J = evaluate(mi_ba.OPENCV, "gauge", 4)
    i1, i2 = PAIRS[px[:, 0], 0], PAIRS[px[:, 0], 1]
    assert plus_zero(J[i1 == 0, 0:6]) and plus_zero(J[i2 == 0, 6:12])
    assert plus_zero(J[i1 == 1, 3]) and plus_zero(J[i2 == 1, 9])


@pytest.mark.parametrize("model", MODELS)
def test_oracle_bitwise(gpu, model):
    import oracle
    sc, sem = build(model, "gauge")
    px_o, st_o, r_o, J_o = oracle.semantic_eval(mi_ba.default_options(), sc, sem)
    px, st, r, J = evaluate(model, "gauge", 4)
    plain, _, _ = decode(st)
    bad = (plain != st_o) | (r.view(np.uint64) != r_o.view(np.uint64)) | \
        np.any(J.view(np.uint64) != J_o.view(np.uint64), axis=1)
    print(f"model {model}: {int(bad.sum())} of {len(bad)} samples differ from the oracle")
    assert np.array_equal(px, px_o)
    assert not bad.any()


def test_coverage(gpu):
    """The cases the tests above are meant to run through, from the marks."""
    px, st, r, J = evaluate(mi_ba.OPENCV, "gauge", 4)
    _, deferred, redone = decode(st)
    per_pair = np.bincount(px[:, 0][deferred], minlength=len(PAIRS))
    print("deferred per pair", per_pair.tolist(), "redone", int(redone.sum()))
    assert (per_pair == 0).any()                             # a pair with no chunk
    assert ((per_pair >= 1) & (per_pair <= 63)).any()        # one partial chunk
    assert ((per_pair > 64) & (per_pair % 64 != 0)).any()    # several chunks, the last one partial
    assert redone.sum() >= 1                                 # the per-point route of a group
    assert np.all(deferred[redone])


def solve(waves):
    sc, sem = build(mi_ba.OPENCV, "gauge")
    sc.camera_constant = None
    opts = mi_ba.default_options(max_num_iterations=3, semantic_weight=0.1)
    b = sc.copy()
    with mi_ba.Context(opts, b, sem) as ctx:
        ctx.set_tuning("semantic_deferred_waves", waves)
        s = ctx.solve()
        ctx.writeback()
    return s, b


def test_pair_blocks_lm_bitwise(gpu):
    """The pair blocks drive the LM: three iterations under both keys, and
    twice under key 4, end with the same bits."""
    s1, a = solve(1)
    s4, b = solve(4)
    s4b, c = solve(4)
    print("LM", s1.num_successful_steps, s1.num_unsuccessful_steps, s1.initial_cost, s1.final_cost, s4.final_cost)
    assert s1.num_semantic_residuals > 0
    assert s1.num_successful_steps + s1.num_unsuccessful_steps >= 3
    for s, x in ((s4, b), (s4b, c)):
        assert (s.num_successful_steps, s.num_unsuccessful_steps) == (s1.num_successful_steps, s1.num_unsuccessful_steps)
        assert s.initial_cost == s1.initial_cost and s.final_cost == s1.final_cost
        for key in ("qvec", "tvec", "xyz"):
            assert np.array_equal(getattr(a, key).view(np.uint64), getattr(x, key).view(np.uint64)), key
