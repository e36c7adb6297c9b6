"""The semantic term of the LM step on irregular image-pair lists.

The semantic term reaches the step through the tables semantic_create builds
from the pair list (the compacted pair list, img_pairs, sblk / sblk_ent, the
poses only it makes variable) and through semantic_fblock / gradient /
product / dense / model_kernel and pair_reduce_kernel.  Every other semantic
LM test uses a regular list (a ring, all ordered pairs, disjoint pairs) and
asserts final costs or the equality of two GPU routes that share the tables:
a wrong side flag on a descending pair, a lost second copy of a duplicate, a
hub's list cut short, an off-by-one behind a skipped pair or a pair beyond
lane 63 missing from the model cost would pass them (the LM still converges).
tests/semantic_pair_scenes.py builds a list that holds all of those, and
restates the tables' rules in Python.

CPU (oracle only):
  * structure: the restated rules show every edge in its scene;
  * the reference is stable: the oracle's steps on a list and on a random
    permutation of it agree within 1e-9 of each block type's largest change
    (measured <= 4.8e-12 over all variants at weights 0.1 and 1.0; the base
    list 3.6e-15 at 0.1 and 8.6e-15 at 1.0);
  * the criterion sees one pair: dropping any kept pair of the base list
    moves the oracle's first step by >= 1e-3 of a block type's largest change
    (measured: minimum 2.2e-3 over the 23 kept pairs, each copy of the
    duplicate (3, 5) 4.6e-3), swapping the sides of any kept pair by >= 1e-3
    (measured 2.5e-3 .. 7.6e-1); dropping a skipped pair moves it by exactly 0;
  * ITERATIVE_SCHUR: the oracle's own PCG at eta 1e-12 lands within 1e-6 of
    its dense step on every variant and with both robust losses (measured
    2.3e-8 .. 4.9e-7), so none is left out of the PCG cases.

GPU: the samples of the full list (skipped and empty pairs included) equal
the oracle's, input pair index and pixel exactly, status / residual /
Jacobian bit for bit; after max_num_iterations 1 and 3, on the list and on
its permuted twin, every parameter's change agrees with the oracle's within
STEP_TOL = 1e-6 of the largest oracle change of its block type, with equal
counts (num_effective_parameters_reduced among them), initial cost (1e-12),
per-iteration flags and final cost (1e-6) — assert_step_parity of
tests/test_ragged_edges.py; constant poses and masked tvec components come
back bit for bit.

Measured GPU-to-oracle step differences (largest ratio per case over both
pair orders and 1 / 3 iterations, MI355X; each case prints its own):
  DENSE_SCHUR full / empty / two_models           1.2e-14 / 5.8e-15 / 2.1e-14
  DENSE_SCHUR ring63 / ring64 / ring65            3.4e-12 / 1.7e-12 / 1.5e-12
  DENSE_SCHUR semantic_only                       6.9e-12
  Cauchy / SoftL1, DENSE_SCHUR                    5.5e-15 / 9.7e-15
  semantic_pair_fused 0 / 1, deterministic_sums 1 / 0: their variant's figure
  ITERATIVE_SCHUR (CG truncation: the oracle's own PCG's distance from its
  exact step, to three digits, stored-J and matrix-free alike):
  full 4.9e-8, empty 2.5e-8, two_models 3.8e-8, ring 4.9e-7 / 4.2e-7 /
  2.8e-7, semantic_only 2.8e-7, Cauchy 3.0e-8, SoftL1 4.9e-8
So the exact path sits six to eight orders of magnitude inside STEP_TOL, at
the oracle's own order-stability figure: it could be held to 1e-9, no tighter.
"""
import functools

import numpy as np
import pytest

import mi_ba
import oracle
import semantic_pair_scenes as ps
from test_ragged_edges import (BLOCK_TYPES, EXACT_PCG, ITERS, STABLE_TOL, STEP_TOL, assert_step_parity, change_ratios,
                               options)

SR, CV = mi_ba.SIMPLE_RADIAL, mi_ba.OPENCV
ONE_PAIR = 1e-3        # what one dropped / swapped pair must move
VARIANTS = ("full", "empty", "ring63", "ring64", "ring65", "two_models", "semantic_only")
LOSSES = {"trivial": {},
          "cauchy": dict(loss_function_type=mi_ba.LOSS_CAUCHY, loss_function_scale=1.0),
          "softl1": dict(loss_function_type=mi_ba.LOSS_SOFT_L1, loss_function_scale=1.0)}
PCG = dict(linear_solver_type=mi_ba.SOLVER_ITERATIVE_SCHUR, **EXACT_PCG)
# ITERATIVE_SCHUR runs every variant, and the base list with both robust
# losses: test_oracle_pcg_reaches_the_exact_step
PCG_VARIANTS = VARIANTS
PCG_CASES = [(v, "trivial") for v in PCG_VARIANTS] + [("full", "cauchy"), ("full", "softl1")]


@functools.lru_cache(maxsize=None)
def scenes(variant):
    """(scene, semantic input, the same with the pair list permuted) —
    shared, never modified: solve on copies."""
    models = (SR, CV) if variant == "two_models" else (SR,)
    sc, depth, label = ps.base_scene(models, observations=variant != "semantic_only")
    step, pairs = 3, ps.PAIRS
    if variant == "empty":
        pairs = np.concatenate([ps.PAIRS, np.array([ps.EMPTY_PAIR], np.int32)])
        depth = ps.empty_rasters(depth)
    elif variant.startswith("ring"):
        step, pairs = 8, ps.ring_variant(sc, int(variant[4:]))
    for a in (depth, label, pairs):
        a.setflags(write=False)
    return sc, ps.semantic(depth, label, pairs, step), ps.semantic(depth, label, ps.twin(pairs)[0], step)


def sem_options(iters, **kw):
    kw.setdefault("semantic_weight", ps.WEIGHT)
    return options(iters, **kw)


def oracle_after(sc, sem, iters=1, **kw):
    a = sc.copy()
    s = oracle.solve(sem_options(iters, **kw), a, sem)
    return a, s


# ---------------------------------------------------------------------------
# CPU: structure, from the restated rules
# ---------------------------------------------------------------------------
def test_base_list_holds_every_edge():
    sc, sem, _ = scenes("full")
    pairs = [tuple(p) for p in sem.pairs.tolist()]
    kept = ps.kept_pairs(sc, pairs)
    assert len(pairs) == 26 and len(kept) == 23
    # skipped pairs in the middle: the internal index falls behind the input index
    skipped = [k for k in range(len(pairs)) if k not in [r[0] for r in kept]]
    assert [pairs[k] for k in skipped] == ps.SKIPPED == [(7, 7), (0, 9), (9, 0)]
    assert 0 < skipped[0] and skipped[-1] < len(pairs) - 1
    assert [r[0] for r in kept[:20]] == list(range(20)) and [r[0] for r in kept[20:]] == [23, 24, 25]
    assert ps.constant_pose(sc, 0) and ps.constant_pose(sc, ps.CONST_POSE)
    assert sum(ps.constant_pose(sc, i) for i in range(sc.num_images)) == 2

    lists = ps.image_pair_lists(sc.num_images, kept)
    hub = lists[ps.HUB]
    # the hub: >= 16 pairs, on both sides, among them a constant second and a constant first pose
    assert len(hub) == 17 and sum(s == 0 for _, s in hub) == 11 and sum(s == 1 for _, s in hub) == 6
    assert any(s == 0 and not kept[k][4] for k, s in hub)      # (1, 0), (1, 9): second pose constant
    assert any(s == 1 and not kept[k][3] for k, s in hub)      # (9, 1): first pose constant
    assert [len(x) for x in lists] == [1, 17, 3, 4, 4, 4, 2, 1, 3, 2, 4, 1, 0]
    assert lists[ps.NO_PAIR] == [] and ps.NO_PAIR in ps.reprojection_variable_images(sc)
    assert all(k0 < k1 for x in lists for (k0, _), (k1, _) in zip(x, x[1:]))   # pair order
    # image 6: no observation, variable through its pairs alone; its mask counts
    assert not np.any(sc.obs_image == ps.SEMANTIC_ONLY) and len(lists[ps.SEMANTIC_ONLY]) == 2
    assert ps.semantic_variable_images(sc, kept) == ([ps.SEMANTIC_ONLY], 5)
    assert {i: int(m) for i, m in enumerate(sc.image_constant_tvec) if m} == ps.TVEC_MASKS

    blocks = ps.s_blocks(kept)
    # descending pairs, both orders of one pair and an exact duplicate
    assert sum(i > j for _, i, j, _, _ in kept) == 10
    assert pairs.count((3, 5)) == 2 and pairs.count((5, 3)) == 1
    k53, k35a, k35b = (pairs.index((5, 3)), pairs.index((3, 5)), pairs.index((3, 5)) + 1)
    assert blocks[(3, 5)] == [(k53, 1), (k35a, 0), (k35b, 0)]   # three entries, both flags (internal = input here)
    both = [b for b, e in blocks.items() if b[0] != b[1] and {f for _, f in e} == {0, 1}]
    assert (3, 5) in both and (1, 2) in both and (4, 10) in both
    # off-diagonal flag 1 exactly on descending pairs; the diagonal flag is the side
    for (a, b), ent in blocks.items():
        for k, f in ent:
            _, i, j, _, _ = kept[k]
            assert f == ((i > j) if a != b else (a == j))
    assert len(blocks[(ps.HUB, ps.HUB)]) == 17
    # behind the skipped pairs the entries carry the internal index, not the input index
    assert blocks[(4, 10)] == [(20, 1), (21, 0)] and blocks[(2, 8)] == [(22, 1)]
    # one full 256-sample tile and a ragged one per pair
    assert set(ps.sample_counts(sem.depth, pairs, 3)) == {484}


def test_empty_pair_is_kept_without_samples():
    sc, sem, twin = scenes("empty")
    pairs = [tuple(p) for p in sem.pairs.tolist()]
    kept = ps.kept_pairs(sc, pairs)
    assert len(kept) == 24 and kept[-1][:3] == (26, ps.EMPTY_IMAGE, 2) and kept[-1][3] and kept[-1][4]
    counts = ps.sample_counts(sem.depth, pairs, 3)
    assert counts[-1] == 0 and all(c == 484 for c in counts[:-1])
    # in the twin the empty pair lies in the middle of the list
    tp = [tuple(p) for p in twin.pairs.tolist()]
    assert sorted(tp) == sorted(pairs) and 0 < tp.index(ps.EMPTY_PAIR) < len(tp) - 1
    assert ps.s_blocks(kept)[(2, ps.EMPTY_IMAGE)] == [(23, 1)]


@pytest.mark.parametrize("n", [63, 64, 65])
def test_ring_variants_sit_on_the_wave_edge(n):
    sc, sem, twin = scenes(f"ring{n}")
    kept = ps.kept_pairs(sc, sem.pairs)
    assert len(kept) == n == len(ps.kept_pairs(sc, twin.pairs))
    assert (n + 63) // 64 == (1 if n <= 64 else 2)          # workgroups of semantic_model_kernel, mpart entries
    assert len(sem.pairs) == n + 3 and sem.pairs[:26].tolist() == ps.PAIRS.tolist()
    assert all(tuple(p) in ps.RING for p in sem.pairs[26:].tolist())
    assert set(ps.sample_counts(sem.depth, sem.pairs, 8)) == {64}
    assert max(len(e) for e in ps.s_blocks(kept).values()) >= 17


def test_two_model_variant_scatters_the_pairs():
    sc, sem, _ = scenes("two_models")
    assert sc.camera_models.tolist() == [SR, CV] * 6 + [SR]
    kept = ps.kept_pairs(sc, sem.pairs)
    second = [int(sc.camera_models[sc.image_camera[j]]) for _, _, j, _, _ in kept]
    # the tiles and chunks are grouped by the second camera's model: that order is not pair order
    assert set(second) == {SR, CV} and second != sorted(second)
    assert sum(a != b for a, b in zip(second, second[1:])) >= 10


def test_semantic_only_variant_has_no_observation():
    sc, sem, _ = scenes("semantic_only")
    assert sc.num_obs == 0 and ps.reprojection_variable_images(sc) == set()
    extra, params = ps.semantic_variable_images(sc, ps.kept_pairs(sc, sem.pairs))
    assert sorted(extra) == [1, 2, 3, 4, 5, 6, 7, 8, 10, 11] and params == 60 - 2 - 1 - 3
    assert oracle_after(sc, sem)[1].num_effective_parameters_reduced == params


def test_oracle_counts_follow_the_restated_rules():
    sc, sem, _ = scenes("full")
    s = oracle_after(sc, sem)[1]
    geo = oracle.solve(options(1), sc.copy())
    kept = ps.kept_pairs(sc, sem.pairs)
    assert s.num_effective_parameters_reduced == geo.num_effective_parameters_reduced + 5
    samples = sum(c for k, c in enumerate(ps.sample_counts(sem.depth, sem.pairs, 3)) if k in [r[0] for r in kept])
    assert s.num_residuals_reduced == geo.num_residuals_reduced + samples == 2 * sc.num_obs + 23 * 484


# ---------------------------------------------------------------------------
# CPU: the reference is stable, sees one pair, and its PCG reaches its exact step
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("weight", [0.1, 1.0])
@pytest.mark.parametrize("variant", VARIANTS)
def test_oracle_step_is_stable_under_pair_order(variant, weight):
    sc, sem, twin = scenes(variant)
    for iters in ITERS:
        (a, s_a), (b, s_b) = (oracle_after(sc, x, iters, semantic_weight=weight) for x in (sem, twin))
        assert (s_a.num_successful_steps, s_a.num_unsuccessful_steps) == \
            (s_b.num_successful_steps, s_b.num_unsuccessful_steps)
        assert s_a.num_successful_steps >= 1
        r = change_ratios(b, a, sc)
        print(f"oracle pair-order stability {variant} weight {weight} iters {iters}: {max(r.values()):.2e}")
        assert max(r.values()) <= STABLE_TOL, (iters, r)


def test_one_dropped_or_swapped_pair_moves_the_oracle_step():
    sc, sem, _ = scenes("full")
    base = oracle_after(sc, sem)[0]
    low_drop = low_swap = np.inf
    for k, i, j, _, _ in ps.kept_pairs(sc, sem.pairs):
        d = oracle_after(sc, ps.semantic(sem.depth, sem.label, ps.drop_pair(sem.pairs, k)))[0]
        w = oracle_after(sc, ps.semantic(sem.depth, sem.label, ps.swap_pair(sem.pairs, k)))[0]
        rd, rw = max(change_ratios(d, base, sc).values()), max(change_ratios(w, base, sc).values())
        print(f"pair {k} ({i}, {j}): dropped {rd:.2e}, sides swapped {rw:.2e}")
        assert rd >= ONE_PAIR and rw >= ONE_PAIR, (k, i, j, rd, rw)
        low_drop, low_swap = min(low_drop, rd), min(low_swap, rw)
    print(f"one pair: smallest step change dropped {low_drop:.2e}, swapped {low_swap:.2e}")


def test_a_skipped_pair_does_not_move_the_oracle_step():
    sc, sem, _ = scenes("full")
    base = oracle_after(sc, sem)[0]
    pairs = [tuple(p) for p in sem.pairs.tolist()]
    for p in ps.SKIPPED:
        d = oracle_after(sc, ps.semantic(sem.depth, sem.label, ps.drop_pair(sem.pairs, pairs.index(p))))[0]
        assert all(np.array_equal(getattr(d, n), getattr(base, n)) for n in BLOCK_TYPES), p


@pytest.mark.parametrize("loss", ["cauchy", "softl1"])
def test_the_loss_moves_the_oracle_step(loss):
    """The corrector path is visible in the step: a robust loss of scale 1
    moves it by far more than STEP_TOL (measured 4.3e-1 / 2.6e-1)."""
    sc, sem, _ = scenes("full")
    r = change_ratios(oracle_after(sc, sem, **LOSSES[loss])[0], oracle_after(sc, sem)[0], sc)
    print(f"{loss} against the trivial loss: {max(r.values()):.2e}")
    assert max(r.values()) >= 1e-2


@pytest.mark.parametrize("variant,loss", PCG_CASES)
def test_oracle_pcg_reaches_the_exact_step(variant, loss):
    """The oracle's own PCG (eta 1e-12, 1000 iterations) lands within
    STEP_TOL of its dense-Schur step on both pair orders, so the exact step is
    a reference a correct PCG can meet."""
    sc, sem, twin = scenes(variant)
    for x in (sem, twin):
        for iters in ITERS:
            (a, s_d), (b, s_p) = (oracle_after(sc, x, iters, **LOSSES[loss]),
                                  oracle_after(sc, x, iters, **LOSSES[loss], **PCG))
            assert (s_p.num_successful_steps, s_p.num_unsuccessful_steps) == \
                (s_d.num_successful_steps, s_d.num_unsuccessful_steps)
            assert s_d.num_successful_steps >= 1
            assert s_p.num_linear_solver_iterations > s_p.num_successful_steps
            r = change_ratios(b, a, sc)
            print(f"oracle pcg against its dense step {variant} {loss} iters {iters}: {max(r.values()):.2e}")
            assert max(r.values()) <= STEP_TOL, (iters, r)


# ---------------------------------------------------------------------------
# GPU
# ---------------------------------------------------------------------------
def bits(x):
    return np.ascontiguousarray(np.asarray(x, np.float64)).view(np.uint64)


@pytest.mark.gpu
@pytest.mark.parametrize("order", ["list", "twin"])
@pytest.mark.parametrize("variant", ["empty", "two_models"])
def test_sample_parity(gpu, variant, order):
    """evaluate_semantic + download_semantic against the oracle's samples:
    the input pair index across skipped and empty pairs and the pixel exactly,
    status, residual and Jacobian bit for bit."""
    sc, sem, twin = scenes(variant)
    sem = sem if order == "list" else twin
    px_o, st_o, r_o, J_o = oracle.semantic_eval(sem_options(1), sc, sem)
    with mi_ba.Context(sem_options(1), sc.copy(), sem) as ctx:
        ctx.evaluate_semantic()
        px, st, r, J = ctx.download_semantic()
    kept = [k for k, _, _, _, _ in ps.kept_pairs(sc, sem.pairs)]
    counts = ps.sample_counts(sem.depth, sem.pairs, sem.pixel_step)
    want = np.repeat(kept, [counts[k] for k in kept])
    assert np.array_equal(px_o[:, 0], want)                    # the oracle's index is the restated one
    assert np.array_equal(px, px_o)
    bad = (st != st_o) | (bits(r) != bits(r_o)) | np.any(bits(J) != bits(J_o), axis=1)
    print(f"sample parity {variant} {order}: {int(bad.sum())} of {len(bad)} samples differ, "
          f"{int(np.any(J_o != 0, axis=1).sum())} with a Jacobian")
    assert np.any(J_o != 0) and not bad.any()


def counted(launches):
    """gpu_traced that also appends semantic_pair_kernel's launch count."""
    def solve(opts, sc, sem=None, tuning=None):
        rec = {}
        opts.set_callback(lambda it: rec.__setitem__(
            it.iteration, (it.step_is_valid, it.step_is_successful, it.linear_solver_iterations)))
        with mi_ba.Context(opts, sc, sem) as ctx:
            for k, v in (tuning or {}).items():
                ctx.set_tuning(k, v)
            ctx.set_timing(True)
            s = ctx.solve()
            launches.append(ctx.kernel_time("semantic_pair_fused")[1])
            ctx.writeback()
        return s, rec
    return solve


def run_case(label, variant, kw=None, tuning=None, fused=None):
    """Step parity on the list and on its permuted twin after 1 and 3
    iterations; fused 0 / 1: also assert which route the semantic pass took."""
    sc, sem, twin = scenes(variant)
    worst = 0.0
    for order, x in (("list", sem), ("permuted", twin)):
        for iters in ITERS:
            launches = []
            ratio, steps = assert_step_parity(sem_options(iters, **(kw or {})), sc, tuning, x, counted(launches))
            if fused is not None:
                assert (launches[0] > 0) == bool(fused), launches
            print(f"step parity {label} {order} iters {iters} steps {steps}: {ratio:.2e}")
            worst = max(worst, ratio)
    print(f"step parity {label}: largest ratio {worst:.2e}")
    return worst


@pytest.mark.gpu
@pytest.mark.parametrize("variant", VARIANTS)
def test_step_dense_schur(gpu, variant):
    """semantic_dense_kernel (sblk / sblk_ent), semantic_fblock_kernel's b
    and semantic_model_kernel (63 / 64 / 65 pairs: one full wave less one, one
    full workgroup, a second workgroup of one lane)."""
    run_case(f"dense {variant}", variant)


@pytest.mark.gpu
@pytest.mark.parametrize("mf", [0, 1])
@pytest.mark.parametrize("variant", PCG_VARIANTS)
def test_step_iterative_schur(gpu, variant, mf):
    """semantic_product_kernel and the semantic_fblock_kernel preconditioner
    (img_pairs) at eta 1e-12 against the oracle's exact LM, with the stored-J
    and the matrix-free Schur product."""
    run_case(f"pcg {variant} mf{mf}", variant, PCG, {"pcg_matrix_free": mf})


@pytest.mark.gpu
@pytest.mark.parametrize("solver", ["dense", "pcg"])
@pytest.mark.parametrize("loss", ["cauchy", "softl1"])
def test_step_robust_loss(gpu, loss, solver):
    """The corrector in the pair blocks (the trivial loss: every other case)."""
    run_case(f"{loss} {solver}", "full", {**LOSSES[loss], **(PCG if solver == "pcg" else {})})


@pytest.mark.gpu
@pytest.mark.parametrize("fused", [0, 1])
@pytest.mark.parametrize("variant", ["full", "empty", "ring65", "two_models"])
def test_step_pair_fused(gpu, variant, fused):
    """One workgroup per pair (semantic_pair_kernel) and the five-kernel
    route (pair_reduce_kernel), each against the oracle, not each other."""
    run_case(f"fused{fused} {variant}", variant, None,
             {"semantic_pair_fused": fused, "semantic_pair_min_pairs": 0}, fused=fused)


@pytest.mark.gpu
@pytest.mark.parametrize("solver", ["dense", "pcg"])
@pytest.mark.parametrize("det", [1, 0])
@pytest.mark.parametrize("variant", ["full", "ring65"])
def test_step_deterministic_sums(gpu, variant, det, solver):
    run_case(f"det{det} {solver} {variant}", variant, PCG if solver == "pcg" else None, {"deterministic_sums": det})


@pytest.mark.gpu
@pytest.mark.parametrize("solver", ["dense", "pcg"])
@pytest.mark.parametrize("variant", ["full", "empty", "semantic_only"])
def test_constant_parameters_stay(gpu, variant, solver):
    """After three iterations the constant poses (0 by the gauge, 9 by its
    flag) and the masked tvec components are the input's bit for bit (a
    quaternion comes back normalised, as everywhere), every other pose in a
    pair moved, image 6 among them."""
    sc, sem, _ = scenes(variant)
    g = sc.copy()
    with mi_ba.Context(sem_options(3, **(PCG if solver == "pcg" else {})), g, sem) as ctx:
        s = ctx.solve()
        ctx.writeback()
    assert s.num_successful_steps >= 1
    q0 = sc.qvec / np.linalg.norm(sc.qvec, axis=1, keepdims=True)
    for i in (0, ps.CONST_POSE):
        assert np.array_equal(bits(g.qvec[i]), bits(q0[i])) and np.array_equal(bits(g.tvec[i]), bits(sc.tvec[i])), i
    for i, mask in ps.TVEC_MASKS.items():
        for b in range(3):
            if (mask >> b) & 1:
                assert bits(g.tvec[i, b]) == bits(sc.tvec[i, b]), (i, b)
            else:
                assert g.tvec[i, b] != sc.tvec[i, b], (i, b)
    moved = [i for i in range(sc.num_images) if not np.array_equal(g.qvec[i], q0[i])]
    in_problem = sorted(set(range(1, 12)) - {ps.CONST_POSE} | ({ps.NO_PAIR} if sc.num_obs else set()))
    assert moved == in_problem and ps.SEMANTIC_ONLY in moved
