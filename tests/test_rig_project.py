"""The rig projection kernel alone (csrc/rig.hip rig_project_kernel through
mi_ba_rig_reduce_dense): S_rig = T^T S_img T, b_rig = T^T b_img against numpy
in float64.

T maps the rig tangent space (6 per slot: snapshot poses, free images,
variable relative poses; then the intrinsics) to the per-image one (6 per
image, then the intrinsics): rows of image i hold A_i in the columns of its
owner slot and, for an image with a variable relative pose, B_i in the
columns of that slot; T is the identity on the intrinsics.  The tests use
dense random A_i, B_i: the kernel may not rely on their structure.

Bound.  An element of an output block is a sum of 36 * P triple products
M_ia(r, q) S_ij(r, k) M_jb(k, c), P the block's member pairs (for an
intrinsics strip or b: 6 * members double products).  Any order of summation
of L terms of two roundings each has the error (L + 2) eps sum|terms| to first
order (Higham, Accuracy and Stability, 3.1 / 3.5), and sum|terms| is the same
element of |T|^T |S| |T|.  The numpy reference carries the same error, hence
    |S_rig - ref| <= 2 (L + 2) eps (|T|^T |S| |T|),  L = 36 P_max,
elementwise, P_max the most member pairs of any block of the case.
The strict lower triangle of S_img holds NaN: only the stored triangle may be
read.  Two runs must agree bit for bit (no floating-point atomics).
"""
import numpy as np
import pytest

import mi_ba

pytestmark = pytest.mark.gpu

EPS = np.finfo(np.float64).eps


def rig_table(num_cameras, num_snapshots, ref_pos, num_free, seed, shuffle_slots=False):
    """One rig of num_cameras x num_snapshots images (snapshot-major, camera
    minor), then num_free images of no rig.  The camera at position ref_pos
    is the reference camera (constant relative pose: no relative-pose slot).
    Slots: snapshots, free images, then one per non-reference camera."""
    rng = np.random.default_rng(seed)
    I = num_cameras * num_snapshots + num_free
    ns = num_snapshots + num_free + (num_cameras - 1)
    slot_of = rng.permutation(ns) if shuffle_slots else np.arange(ns)
    owner = np.zeros(I, np.int32)
    rel = np.full(I, -1, np.int32)
    for s in range(num_snapshots):
        for c in range(num_cameras):
            i = s * num_cameras + c
            owner[i] = slot_of[s]
            if c != ref_pos:
                rel[i] = slot_of[num_snapshots + num_free + (c if c < ref_pos else c - 1)]
    for f in range(num_free):
        owner[num_cameras * num_snapshots + f] = slot_of[num_snapshots + f]
    A = rng.uniform(-1, 1, (I, 6, 6))
    B = rng.uniform(-1, 1, (I, 6, 6))
    A[num_cameras * num_snapshots:] = np.eye(6)  # an image of no rig
    return owner, rel, A, B, ns


def dense_T(owner, rel, A, B, ns, nc):
    I = len(owner)
    T = np.zeros((6 * I + nc, 6 * ns + nc))
    for i in range(I):
        T[6 * i:6 * i + 6, 6 * owner[i]:6 * owner[i] + 6] = A[i]
        if rel[i] >= 0:
            T[6 * i:6 * i + 6, 6 * rel[i]:6 * rel[i] + 6] = B[i]
    T[6 * I:, 6 * ns:] = np.eye(nc)
    return T


def spd(n, seed):
    rng = np.random.default_rng(seed)
    G = rng.standard_normal((n, max(1, n // 2)))
    return G @ G.T / n + np.diag(rng.uniform(0.5, 2.0, n))


def max_member_pairs(owner, rel, ns):
    members = np.bincount(owner, minlength=ns) + np.bincount(rel[rel >= 0], minlength=ns)
    return int(members.max()) ** 2, int(members.max())


CASES = {
    # name: (cameras, snapshots, reference camera position, free images, intrinsics, shuffled slots)
    "2x3": (2, 3, 0, 0, 0, False),
    "2x3_free_intrinsics": (2, 3, 0, 3, 5, True),
    "2x70": (2, 70, 0, 1, 4, False),
    "ref_not_first": (3, 4, 2, 2, 6, True),
}


@pytest.mark.parametrize("name", list(CASES))
def test_reduce_dense_against_numpy(gpu, name):
    ncam, nsnap, ref_pos, nfree, nc, shuffle = CASES[name]
    owner, rel, A, B, ns = rig_table(ncam, nsnap, ref_pos, nfree, seed=len(name), shuffle_slots=shuffle)
    n_img = 6 * len(owner) + nc
    S = spd(n_img, seed=7 + nsnap)
    b = np.random.default_rng(3).standard_normal(n_img)
    pairs, members = max_member_pairs(owner, rel, ns)
    chunk, lanes = mi_ba.rig_project_chunk()
    if name == "2x70":
        # the relative-pose slot has one member per snapshot: more than one pass
        # of the kernel's member loop (32 pairs, two lanes each), and its diagonal
        # block more pairs than one chunk (1024), so the chunked route and its
        # combine run
        assert (chunk, lanes) == (1024, 32)
        assert members == 70 and members > lanes and pairs > chunk
    else:
        assert pairs <= chunk
    S_in = np.triu(S) + np.tril(np.full_like(S, np.nan), -1)
    S_rig, b_rig = mi_ba.rig_reduce_dense(S_in, b, owner, rel, A, B, ns, nc)

    T = dense_T(owner, rel, A, B, ns, nc)
    ref = T.T @ S @ T
    mag = np.abs(T).T @ np.abs(S) @ np.abs(T)
    bound = 2 * (36 * pairs + 2) * EPS * mag
    iu = np.triu_indices(ref.shape[0])
    err = np.abs(S_rig - ref)
    print(f"{name}: max err/bound {np.max(err[iu] / bound[iu]):.3g}, max|S_rig| {np.abs(ref).max():.3g}")
    assert np.all(np.isfinite(S_rig))
    assert np.all(err[iu] <= bound[iu])
    assert np.all(S_rig[np.tril_indices(ref.shape[0], -1)] == 0.0)
    ref_b = T.T @ b
    bound_b = 2 * (6 * members + 2) * EPS * (np.abs(T).T @ np.abs(b))
    assert np.all(np.abs(b_rig - ref_b) <= bound_b)

    # bitwise repeatable
    S2, b2 = mi_ba.rig_reduce_dense(S_in, b, owner, rel, A, B, ns, nc)
    assert np.array_equal(S_rig, S2) and np.array_equal(b_rig, b2)


def test_identity_table_copies(gpu):
    """Every image its own slot with A = I: T is a permutation, S_rig is S
    with its blocks permuted, exactly."""
    I, nc = 5, 3
    rng = np.random.default_rng(11)
    owner = rng.permutation(I).astype(np.int32)
    rel = np.full(I, -1, np.int32)
    A = np.tile(np.eye(6), (I, 1, 1))
    S = spd(6 * I + nc, seed=2)
    b = rng.standard_normal(6 * I + nc)
    S_rig, b_rig = mi_ba.rig_reduce_dense(np.triu(S), b, owner, rel, A, A, I, nc)
    T = dense_T(owner, rel, A, A, I, nc)
    assert np.array_equal(S_rig, np.triu(T.T @ S @ T))
    assert np.array_equal(b_rig, T.T @ b)


def test_reduce_dense_rejects_bad_tables(gpu):
    owner, rel, A, B, ns = rig_table(2, 3, 0, 0, seed=1)
    S = spd(36, seed=1)
    for bad_owner, bad_rel, slots in ((owner + 1, rel, ns),          # owner slot out of range
                                      (owner, np.where(rel >= 0, ns, rel), ns),  # relative slot out of range
                                      (owner, owner, ns)):            # one slot twice for an image
        with pytest.raises(mi_ba.MiBaError) as e:
            mi_ba.rig_reduce_dense(S, None, bad_owner, bad_rel, A, B, slots, 0)
        assert e.value.status == mi_ba.ERR_INVALID_ARGUMENT
    with pytest.raises(mi_ba.MiBaError) as e:  # n_img does not match the table
        mi_ba.rig_reduce_dense(S[:30, :30], None, owner, rel, A, B, ns, 0)
    assert e.value.status == mi_ba.ERR_INVALID_ARGUMENT
