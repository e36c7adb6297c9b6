"""The four-wave deferred pass with its chunk loop reading ahead
("semantic_deferred_pipeline" 1: the chunk records carry the pair's count and
start, and a workgroup loads the record, the dlist entries and the samples of
the chunks to come while it computes the current one) against today's loop
(key 0), which loads each chunk's inputs before it computes.

The pipelined loop hands the same record, entry and sample values to the same
chunk body, and the chunk sums go to slots addressed by (pair, chunk), so
status, residual, Jacobian, and with the costs and pair blocks a whole LM solve
must be equal bit for bit whichever workgroup takes which chunk: no tolerance
anywhere in this file.  The step's costs and pair blocks have no download of
their own; they are pinned through the LM solves they drive (test_lm_bitwise), as in
test_linearize_fusion.py.

The scene is the one of test_semantic_deferred_waves.py (8 images of
160 x 160, 16 pairs, about 46 live chunks for OPENCV: full chunks, partial
last chunks, pairs of one short chunk, pairs with none), and an edit of it
that leaves one pair with exactly 64 deferred samples (a full last chunk) and
one with exactly 65 (a one-row chunk).  "semantic_deferred_groups" sets the
resident grid in workgroups: with 1, 2 and 3 a workgroup walks many chunks
across every pair change and off the end of the list (the loop carry runs);
chunk count - 1, the chunk count and four times the chunk count cover a grid
one short of, equal to and larger than the list.  Both list writers are run:
deferred_compact_kernel ("linearize_fusion" without bit 2) and
deferred_order_kernel<true> (with it)."""
import functools

import numpy as np
import pytest

import mi_ba
from test_semantic_deferred_waves import MODELS, PAIRS, build, decode

pytestmark = pytest.mark.gpu

FLAGS = ["gauge", "pose", "tvec"]
FUSIONS = (1, 7)     # the chunk list by deferred_compact_kernel / by deferred_order_kernel<true>
PAIR64, PAIR65 = 13, 2   # (5, 0): 253 deferred samples for OPENCV; (2, 3): 626.  No image in common.
FAR = 100.0          # a first-image depth never within the threshold: the sample is settled by the flat pass


def bits(x):
    return np.ascontiguousarray(x).view(np.uint64)


def frozen(out):
    for x in out:
        x.setflags(write=False)
    return out


def assert_samples_equal(a, b, what):
    for x, y in zip(a[:2], b[:2]):     # pixels, status with its marks
        assert np.array_equal(x, y), what
    for x, y in zip(a[2:], b[2:]):     # r, J
        assert np.array_equal(bits(x), bits(y)), what


def evaluated(ctx, **keys):
    for k, v in keys.items():
        ctx.set_tuning("semantic_deferred_" + k if k != "fusion" else "linearize_fusion", v)
    ctx.evaluate_semantic()
    return frozen(ctx.download_semantic())


def per_pair_deferred(out):
    px, st = out[0], out[1]
    _, deferred, _ = decode(st)
    return np.bincount(px[:, 0][deferred], minlength=len(PAIRS))


def live_chunks(out):
    return int(((per_pair_deferred(out) + 63) // 64).sum())


def grids(nch):
    return (1, 2, 3, nch - 1, nch, 4 * nch)


def check_scene(sc, sem, expect=None):
    """Key 0 at the default grid is the reference; every grid, both list
    writers and both settings of the compaction under key 1 (and key 0 at the
    small grids: the groups key alone) must reproduce its bytes."""
    with mi_ba.Context(mi_ba.default_options(), sc.copy(), sem) as ctx:
        ctx.set_tuning("semantic_diag", 2)
        ref = evaluated(ctx, pipeline=0, groups=0, compact=1, fusion=1)
        counts = per_pair_deferred(ref)
        nch = live_chunks(ref)
        print("deferred per pair", counts.tolist(), "live chunks", nch)
        assert nch >= 8
        if expect is not None:
            expect(counts)
        for fusion in FUSIONS:
            for compact in (1, 0):
                for g in grids(nch):
                    for pipe in ((1, 0) if g <= 3 else (1,)):
                        got = evaluated(ctx, pipeline=pipe, groups=g, compact=compact, fusion=fusion)
                        assert_samples_equal(ref, got, f"fusion {fusion} compact {compact} groups {g} pipeline {pipe}")
        # back to key 0 on the same context: nothing of the pipelined layout lingers
        assert_samples_equal(ref, evaluated(ctx, pipeline=0, groups=0, compact=1, fusion=1), "key 0 again")
    return ref


@pytest.mark.parametrize("flags", FLAGS)
@pytest.mark.parametrize("model", MODELS)
def test_every_grid_against_key_0(gpu, model, flags):
    def expect(counts):
        assert (counts == 0).any()                             # a pair with no chunk
        assert ((counts >= 1) & (counts <= 63)).any()          # a pair of one short chunk
        assert ((counts > 64) & (counts % 64 != 0)).any()      # several chunks, the last one partial
        assert (counts >= 128).any()                           # full chunks
    sc, sem = build(model, flags)
    check_scene(sc, sem, expect)


@functools.lru_cache(maxsize=None)
def edge_scene():
    """The OPENCV scene with all but the first 64 deferred samples of pair
    PAIR64, and all but the first 65 of pair PAIR65, moved far away in their
    first image's depth map: the flat pass then settles them."""
    sc, sem = build(mi_ba.OPENCV, "gauge")
    with mi_ba.Context(mi_ba.default_options(), sc.copy(), sem) as ctx:
        ctx.set_tuning("semantic_diag", 2)
        px, st, _, _ = evaluated(ctx, pipeline=0)
    _, deferred, _ = decode(st)
    depth = np.array(sem.depth, np.float32, copy=True)
    for pair, keep in ((PAIR64, 64), (PAIR65, 65)):
        rows = np.flatnonzero(deferred & (px[:, 0] == pair))
        assert len(rows) > keep
        drop = rows[keep:]
        depth[PAIRS[pair, 0], px[drop, 2], px[drop, 1]] = FAR
    return sc, mi_ba.SemanticInput(depth, sem.label, PAIRS, pixel_step=sem.pixel_step)


def test_full_last_chunk_and_one_row_chunk(gpu):
    def expect(counts):
        assert counts[PAIR64] == 64 and counts[PAIR65] == 65
    sc, sem = edge_scene()
    check_scene(sc, sem, expect)


def test_one_wave_kernel_on_the_new_layout(gpu):
    """The one-wave kernel (the bitwise reference of the four-wave one) reads
    the chunk list the pipelined layout's writers leave."""
    sc, sem = edge_scene()
    with mi_ba.Context(mi_ba.default_options(), sc.copy(), sem) as ctx:
        ctx.set_tuning("semantic_diag", 2)
        four = evaluated(ctx)                                  # the default build
        for fusion in FUSIONS:
            one = evaluated(ctx, waves=1, pipeline=1, fusion=fusion)
            pa, da, _ = decode(four[1])
            pb, db, _ = decode(one[1])
            assert np.array_equal(pa, pb) and np.array_equal(da, db)
            assert np.array_equal(bits(four[2]), bits(one[2])) and np.array_equal(bits(four[3]), bits(one[3]))
            ctx.set_tuning("semantic_deferred_waves", 4)
            assert_samples_equal(four, evaluated(ctx, pipeline=1, groups=2, fusion=fusion), f"four waves, fusion {fusion}")
            ctx.set_tuning("semantic_deferred_groups", 0)


LM = dict(max_num_iterations=3, semantic_weight=0.1)


def lm_scene():
    sc, sem = edge_scene()
    sc = sc.copy()
    sc.camera_constant = None        # intrinsics variable
    return sc, sem


def test_linearize_jacobian_bitwise(gpu):
    """linearize() under every list writer and a few grids, then the step's
    Jacobian as test_linearize_fusion.py downloads it (the step's costs and
    pair blocks show in test_lm_bitwise: initial cost, every accept / reject
    decision, the final parameters)."""
    sc, sem = lm_scene()
    with mi_ba.Context(mi_ba.default_options(**LM), sc.copy(), sem) as ctx:
        def step(**keys):
            for k, v in keys.items():
                ctx.set_tuning("semantic_deferred_" + k if k != "fusion" else "linearize_fusion", v)
            ctx.linearize()
            return frozen(ctx.download_jacobian())
        jac0 = step(pipeline=0, groups=0, fusion=0)
        assert len(jac0[0]) > 0
        for fusion in (1, 7):
            for g in (1, 3, 0):
                jac = step(pipeline=1, groups=g, fusion=fusion)
                assert np.array_equal(jac0[0], jac[0])
                assert np.array_equal(bits(jac0[1]), bits(jac[1])) and np.array_equal(bits(jac0[2]), bits(jac[2]))


def solve(pipeline, groups, fusion):
    sc, sem = lm_scene()
    b = sc.copy()
    with mi_ba.Context(mi_ba.default_options(**LM), b, sem) as ctx:
        ctx.set_tuning("semantic_deferred_pipeline", pipeline)
        ctx.set_tuning("semantic_deferred_groups", groups)
        ctx.set_tuning("linearize_fusion", fusion)
        s = ctx.solve()
        ctx.writeback()
    return s, b


@functools.lru_cache(maxsize=None)
def solve_key_0():
    return solve(0, 0, 1)


@pytest.mark.parametrize("groups,fusion", [(1, 1), (2, 7), (0, 1), (0, 7)])
def test_lm_bitwise(gpu, groups, fusion):
    """Three LM iterations: the pair blocks drive every accept / reject
    decision and the final parameters."""
    s0, a = solve_key_0()
    s, x = solve(1, groups, fusion)
    print("LM", s0.num_successful_steps, s0.num_unsuccessful_steps, s0.initial_cost, s0.final_cost, s.final_cost)
    assert s0.num_semantic_residuals > 0
    assert s0.num_successful_steps + s0.num_unsuccessful_steps >= 3
    assert (s.num_successful_steps, s.num_unsuccessful_steps) == (s0.num_successful_steps, s0.num_unsuccessful_steps)
    assert s.initial_cost == s0.initial_cost and s.final_cost == s0.final_cost
    for key in ("qvec", "tvec", "xyz", "camera_params"):
        assert np.array_equal(bits(getattr(a, key)), bits(getattr(x, key))), key
