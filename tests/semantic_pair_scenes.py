"""Scenes whose image-pair list is irregular, for the semantic part of the LM step.

The semantic term enters the step through tables that semantic_create
(csrc/semantic.hip) builds once from the input pair list: the compacted pair
list (self pairs and pairs of two constant poses are skipped, so the internal
pair index differs from the input index), each image's pairs (img_pairs,
(pair << 1) | side), each touched 6 x 6 block of the reduced camera system
with its contributions (sblk / sblk_ent, (pair << 1) | flag), and the poses
that only the semantic term makes variable.  Every other semantic LM test
uses a ring, all ordered pairs or disjoint pairs, where every image has the
same number of pairs and lies in the reprojection problem.

base_scene: the generator's 12-image scene plus a 13th image with its own
observations (SIMPLE_RADIAL, intrinsics constant), 64 x 64 rasters.
Image 0 is constant by the gauge, image 9 by its flag, image 6 has no
observation (only the semantic term makes its pose variable), image 12 is in
no pair, images 3, 6 and 10 carry tvec masks.  PAIRS, in input order:

  * hub pairs (1, j) for j = 0, 2 .. 11 ((1, 0) and (1, 9): constant second
    pose), then (j, 1) for j = 2, 4 .. 10 and (9, 1) (constant first pose):
    image 1 is in 17 pairs, on both sides;
  * (5, 3), (3, 5), (3, 5): a descending pair, the other order and an exact
    duplicate, so S block (3, 5) holds three entries with both flags;
  * (7, 7), (0, 9), (9, 0): skipped, in the middle of the list;
  * (10, 4), (4, 10), (8, 2): more descending pairs behind the skipped ones.

EMPTY_PAIR (11, 2) is kept but has no sample once image 11's depth raster is
zero (which also silences (1, 11): hence a raster copy of its own, "empty").
ring_variant appends ring pairs until exactly 63 / 64 / 65 pairs are kept
(semantic_model_kernel: one lane per pair, 64 pairs per workgroup).

kept_pairs, image_pair_lists, s_blocks, semantic_variable_images and
sample_counts restate semantic_create's rules in Python;
tests/test_semantic_pair_graph.py uses them to prove that the scenes hold
the edges above.  twin() is the same list in a random order.
"""
import numpy as np

import mi_ba

IMAGES = 13
SIZE = 64
HUB = 1
SEMANTIC_ONLY = 6      # no observation: variable through its pairs alone
NO_PAIR = 12           # observations, no pair
CONST_POSE = 9         # beside image 0 (the gauge)
EMPTY_IMAGE = 11       # zero depth raster in the "empty" variant
TVEC_MASKS = {3: 0b101, 6: 0b010, 10: 0b111}
WEIGHT = 0.1
REL_STEP = 1e-2

HUB_OUT = [(HUB, j) for j in range(12) if j != HUB]
HUB_IN = [(j, HUB) for j in (2, 4, 6, 8, 10)] + [(CONST_POSE, HUB)]
TAIL = [(5, 3), (3, 5), (3, 5), (7, 7), (0, 9), (9, 0), (10, 4), (4, 10), (8, 2)]
PAIRS = np.array(HUB_OUT + HUB_IN + TAIL, np.int32)
EMPTY_PAIR = (EMPTY_IMAGE, 2)
SKIPPED = [(7, 7), (0, 9), (9, 0)]
RING = [(i, (i + 1) % 12) for i in range(12)]


def base_scene(models=(mi_ba.SIMPLE_RADIAL,), observations=True):
    """(scene, depth, label): the scene above; models alternate over the
    cameras; observations False: no reprojection block at all."""
    def generated(images):
        return mi_ba.generate_scene(mi_ba.synth_config(mi_ba.SIMPLE_RADIAL, images, 200, track_length=4,
                                                       image_size=72, rotation_range=0.05, extra=(0.05, 0, 0, 0),
                                                       seed=7))

    # The generator draws cameras, poses and points before the tracks, so the
    # 13-image scene holds the 12-image scene's and one more pose.  The
    # observations are the 12-image scene's, and image 12 adds its own: a
    # fifth observation on 51 of the 200 points.
    small, sc = generated(IMAGES - 1), generated(IMAGES)
    assert np.array_equal(small.xyz, sc.xyz) and np.array_equal(small.tvec, sc.tvec[:IMAGES - 1])
    own = sc.obs_image == NO_PAIR
    sc.obs_xy = np.concatenate([small.obs_xy, sc.obs_xy[own]])
    sc.obs_image = np.concatenate([small.obs_image, sc.obs_image[own]])
    sc.obs_point = np.concatenate([small.obs_point, sc.obs_point[own]])
    if tuple(models) != (mi_ba.SIMPLE_RADIAL,):
        sc = mi_ba.convert_cameras(sc, list(models))
    sc = sc.gauge()
    sc.camera_constant = np.ones(sc.num_cameras, np.uint8)
    sc.image_constant_pose[CONST_POSE] = 1
    sc.image_constant_tvec[:] = 0
    for i, m in TVEC_MASKS.items():
        sc.image_constant_tvec[i] = m
    depth, label = mi_ba.render_semantic(sc, 72, 72, cell=0.1)
    depth = np.ascontiguousarray(depth[:, :SIZE, :SIZE])
    label = np.ascontiguousarray(label[:, :SIZE, :SIZE])
    sc.tvec[2:] += np.random.default_rng(3).uniform(-0.01, 0.01, sc.tvec[2:].shape)
    keep = (sc.obs_image != SEMANTIC_ONLY) if observations else np.zeros(sc.num_obs, bool)
    sc.obs_xy, sc.obs_image, sc.obs_point = sc.obs_xy[keep].copy(), sc.obs_image[keep].copy(), sc.obs_point[keep].copy()
    return sc, depth, label


def semantic(depth, label, pairs, step=3):
    return mi_ba.SemanticInput(depth, label, np.array(pairs, np.int32).reshape(-1, 2), pixel_step=step,
                               numeric_relative_step_size=REL_STEP)


def empty_rasters(depth):
    d = depth.copy()
    d[EMPTY_IMAGE] = 0.0
    return d


def twin(pairs, seed=5):
    """(the list in a random order, the permutation)."""
    pairs = np.asarray(pairs, np.int32).reshape(-1, 2)
    perm = np.random.default_rng(seed).permutation(len(pairs))
    return pairs[perm].copy(), perm


def ring_variant(sc, kept):
    """PAIRS followed by ring pairs (i, i + 1 mod 12), repeated, until
    exactly `kept` pairs are kept."""
    out = [tuple(p) for p in PAIRS.tolist()]
    k = 0
    while len(kept_pairs(sc, out)) < kept:
        out.append(RING[k % len(RING)])
        k += 1
    return np.array(out, np.int32)


def drop_pair(pairs, k):
    pairs = np.asarray(pairs, np.int32).reshape(-1, 2)
    return pairs[np.arange(len(pairs)) != k].copy()


def swap_pair(pairs, k):
    out = np.array(pairs, np.int32).reshape(-1, 2)
    out[k] = out[k][::-1]
    return out


# ---------------------------------------------------------------------------
# semantic_create's rules, restated
# ---------------------------------------------------------------------------
def constant_pose(sc, i, refine_extrinsics=True):
    return (not refine_extrinsics) or (sc.image_constant_pose is not None and bool(sc.image_constant_pose[i]))


def kept_pairs(sc, pairs, refine_extrinsics=True):
    """[(input index, i, j, first pose variable, second pose variable)] of
    the pairs that become residual blocks, in input order: a pair with i == j
    and a pair of two constant poses is skipped.  A row's position is the
    internal pair index."""
    out = []
    for k, (i, j) in enumerate(np.asarray(pairs).reshape(-1, 2).tolist()):
        if i == j:
            continue
        c1, c2 = constant_pose(sc, i, refine_extrinsics), constant_pose(sc, j, refine_extrinsics)
        if c1 and c2:
            continue
        out.append((k, i, j, not c1, not c2))
    return out


def image_pair_lists(num_images, kept):
    """Per image its [(internal pair, side)] in pair order: side 0 where the
    image is the pair's first pose, 1 where it is the second (img_pairs)."""
    lists = [[] for _ in range(num_images)]
    for k, (_, i, j, _, _) in enumerate(kept):
        lists[i].append((k, 0))
        lists[j].append((k, 1))
    return lists


def s_blocks(kept):
    """{(a, b), a <= b: [(internal pair, flag)]} in pair order (sblk /
    sblk_ent).  Diagonal block: flag 0 is the pair's M11, 1 its M22.
    Off-diagonal block: flag 0 — rows a are the pair's first pose; flag 1 —
    its second, which happens exactly when i > j."""
    blocks = {}
    for k, (_, i, j, _, _) in enumerate(kept):
        blocks.setdefault((i, i), []).append((k, 0))
        blocks.setdefault((j, j), []).append((k, 1))
        if i < j:
            blocks.setdefault((i, j), []).append((k, 0))
        else:
            blocks.setdefault((j, i), []).append((k, 1))
    return dict(sorted(blocks.items()))


def reprojection_variable_images(sc):
    """Images whose pose the reprojection problem makes variable."""
    seen = np.zeros(sc.num_images, bool)
    seen[sc.obs_image] = True
    return {i for i in range(sc.num_images) if seen[i] and not constant_pose(sc, i)}


def semantic_variable_images(sc, kept):
    """(images whose pose only the semantic term makes variable, the
    effective parameters they add: 6 less the masked tvec components)."""
    have = reprojection_variable_images(sc)
    extra = []
    for _, i, j, v1, v2 in kept:
        for img, var in ((i, v1), (j, v2)):
            if var and img not in have and img not in extra:
                extra.append(img)
    mask = sc.image_constant_tvec
    params = sum(6 - bin(int(mask[i]) if mask is not None else 0).count("1") for i in extra)
    return extra, params


def sample_counts(depth, pairs, step):
    """Samples per input pair as semantic_create would count them for a kept
    pair: the first image's grid (y outer, x inner), pixels of depth >= 1e-4."""
    per_image = [int((np.asarray(d, np.float64)[::step, ::step] >= 1e-4).sum()) for d in depth]
    return [per_image[i] for i, _ in np.asarray(pairs).reshape(-1, 2).tolist()]
