"""Ragged scenes that put the LM step on the edges of its four partitions.

Every scene of mi_ba.generate_scene gives each point the same track length,
so the layouts of runtime.hip (context_recycle / build_pair_tiles) are only
ever seen at floor(64 / L) points per chunk, one tile per image and fewer
than 256 pairs per image pair.  The scenes here are cut out of the
full-visibility generator (track_length=0: observation i * P + k is point k
in image i) so that

  * chunk_scene: point chunks filled to exactly 64 by two points and by one,
    splits at 63 + 2 and 60 + 5, multi-pass points of 65, 127, 128 and 129
    blocks;
  * tile_scene: images of 3, 3, 2, 2 (the second of one block), 1 full and 1
    short-by-one camera-major tile, image pairs of 255 ... 2049 co-observed
    points (pair tiles with a last tile of 1, 255 and 256 entries), one image
    with a single observation;
  * shared_chunk_scene: chunk_scene on three shared cameras (the owner-pair
    flush in runs of 256).

Each builder returns (scene, twin): the twin holds the same observations in a
random order (the product sorts them point-major itself, stable).

point_chunks, image_tiles and pair_tile_counts restate the three layout rules
in Python; tests/test_ragged_edges.py uses them to prove that the scenes hit
the edges above.
"""
import numpy as np

import mi_ba

CHUNK_BLOCKS = 64      # point chunks: whole points, <= 64 blocks
TILE_OBS = 1024        # device.h kTileObs: camera-major image tiles
PAIR_TILE = 256        # device.h kPairTile: pair tiles per image pair
OWNER_RUN = 256        # order_owner_flush kRun: entries per owner-pair run

CHUNK_IMAGES = 130
CHUNK_HEAD = (2, 62, 63, 2, 64, 65, 3, 3, 127, 128, 129, 32, 32, 60, 5, 61, 3, 64, 64, 2)
CHUNK_FILLER = 700
# constants variant: the 65-block point (a constant multi-pass chunk), one
# 64-block point, the first point of a full chunk (2 + 62), every 7th filler
CHUNK_CONSTANT_HEAD = (5, 4, 0)

TILE_QUOTAS = (2049, 2049, 2048, 1025, 1024, 1023, 513, 257, 256, 255, 65, 64, 1)


def _subset(sc, keep, seed):
    """(scene with the observations `keep` in generator order, the same scene
    with them randomly permuted), both with the controller's gauge."""
    out = []
    for idx in (keep, np.random.default_rng(seed).permutation(keep)):
        s = sc.copy()
        s.obs_xy, s.obs_image, s.obs_point = sc.obs_xy[idx].copy(), sc.obs_image[idx].copy(), sc.obs_point[idx].copy()
        out.append(s.gauge())
    return tuple(out)


def chunk_track_lengths():
    rng = np.random.default_rng(1)
    lens = np.concatenate([np.array(CHUNK_HEAD), rng.integers(2, 10, CHUNK_FILLER)])
    return lens, rng


def chunk_scene(model, extra, constants=False, trim_mod=None):
    """130 images, 720 points with the track lengths CHUNK_HEAD then 700
    fillers of 2..9, each point on images drawn without replacement.
    constants: the point_config variant.  trim_mod r: filler observations
    dropped from the end (never below two per point) until nb % 64 == r."""
    lens, rng = chunk_track_lengths()
    I, P = CHUNK_IMAGES, len(lens)
    full = mi_ba.generate_scene(mi_ba.synth_config(model, I, P, track_length=0, extra=extra, seed=3))
    img, pts = [], []
    for k, n in enumerate(lens):
        img.append(np.sort(rng.choice(I, int(n), replace=False)))
        pts.append(np.full(int(n), k))
    img, pts = np.concatenate(img), np.concatenate(pts)
    if trim_mod is not None:
        count = lens.copy()
        alive = np.ones(len(img), bool)
        e = len(img) - 1
        while int(alive.sum()) % 64 != trim_mod:
            while count[pts[e]] <= 2:
                e -= 1
            assert pts[e] >= len(CHUNK_HEAD)
            alive[e] = False
            count[pts[e]] -= 1
            e -= 1
        img, pts = img[alive], pts[alive]
    a, b = _subset(full, img * P + pts, seed=11)
    if constants:
        cfg = np.ones(P, np.uint8)
        cfg[list(CHUNK_CONSTANT_HEAD)] = 2
        cfg[len(CHUNK_HEAD)::7] = 2
        a.point_config, b.point_config = cfg, cfg.copy()
    return a, b


def tile_scene(model, extra):
    """13 images, image i observes points 0 .. TILE_QUOTAS[i] - 1 of 2049."""
    I, P = len(TILE_QUOTAS), max(TILE_QUOTAS)
    full = mi_ba.generate_scene(mi_ba.synth_config(model, I, P, track_length=0, extra=extra, seed=4))
    keep = np.concatenate([i * P + np.arange(q) for i, q in enumerate(TILE_QUOTAS)])
    return _subset(full, keep, seed=12)


def shared_chunk_scene(model, extra, ncam=3):
    """chunk_scene with image i on camera i % 3 (the generator gives every
    camera the same intrinsics, so the observations stay consistent)."""
    out = []
    for s in chunk_scene(model, extra):
        s.image_camera = (np.arange(s.num_images) % ncam).astype(np.int32)
        s.camera_params = s.camera_params[:ncam].copy()
        out.append(s)
    return tuple(out)


def drop_observation(sc, k):
    s = sc.copy()
    keep = np.arange(sc.num_obs) != k
    s.obs_xy, s.obs_image, s.obs_point = sc.obs_xy[keep].copy(), sc.obs_image[keep].copy(), sc.obs_point[keep].copy()
    return s


# ---------------------------------------------------------------------------
# The layout rules of runtime.hip, restated (every image in the config, so
# every observation is a reduced block)
# ---------------------------------------------------------------------------
def _variable(sc):
    cfg = sc.point_config
    return np.ones(sc.num_points, bool) if cfg is None else np.asarray(cfg) != 2


def point_chunks(sc):
    """Blocks per point of each point chunk, in chunk order: points by id,
    packed greedily while the chunk stays <= 64 blocks (constant points'
    blocks included); a point of more than 64 blocks is a chunk of its own."""
    n = np.bincount(sc.obs_point, minlength=sc.num_points)
    chunks, cur = [], []
    for c in n[n > 0]:
        if cur and sum(cur) + c > CHUNK_BLOCKS:
            chunks.append(cur)
            cur = []
        cur.append(int(c))
    if cur:
        chunks.append(cur)
    return chunks


def image_tiles(sc):
    """Per image the block counts of its camera-major tiles (<= 1024 each)."""
    n = np.bincount(sc.obs_image, minlength=sc.num_images)
    return [[min(TILE_OBS, int(c) - t) for t in range(0, int(c), TILE_OBS)] for c in n]


def pair_tile_counts(sc):
    """{(ia, ib): [entries per pair tile]} with ia <= ib: the cross pairs
    (variable points observed by both images) and, under (ia, ia), the self
    pairs (blocks of variable points in image ia), cut into tiles of <= 256."""
    var = _variable(sc)
    vis = np.zeros((sc.num_images, sc.num_points), np.int64)
    np.add.at(vis, (sc.obs_image, sc.obs_point), 1)
    assert vis.max() <= 1
    vis = vis[:, var]
    co = vis @ vis.T
    out = {}
    for a in range(sc.num_images):
        for b in range(a, sc.num_images):
            c = int(co[a, b])
            if c:
                out[(a, b)] = [min(PAIR_TILE, c - t) for t in range(0, c, PAIR_TILE)]
    return out


def owner_run_counts(sc):
    """Shared cameras: entries per run of every (pose | camera) owner pair of
    the deterministic pair flush (order_owner_flush): every pair tile adds one
    entry to the (pose, pose), (pose, camera), (camera, pose) and (camera,
    camera) lists of its two images' owners — a self tile to three of them —
    and a list is cut into runs of <= 256 entries."""
    cam = lambda i: ("c", int(sc.image_camera[i]))  # noqa: E731
    lists = {}
    for (a, b), tiles in pair_tile_counts(sc).items():
        for q in range(4):
            if a == b and q == 2:
                continue
            x = cam(a) if q & 2 else ("p", a)
            y = cam(b) if q & 1 else ("p", b)
            key = tuple(sorted((x, y)))
            lists[key] = lists.get(key, 0) + len(tiles)
    return {k: [min(OWNER_RUN, n - t) for t in range(0, n, OWNER_RUN)] for k, n in lists.items()}
