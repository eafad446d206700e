"""Soft clustering on the CPU: the restatement (tests/soft_reference.py) against a hand-worked tree
written out below, and the host paths of hdb_exemplars / hdb_membership_vectors (csrc/soft.cpp,
ctx = NULL, no device) against both.  Every comparison is on bits.

The hand-worked tree (tree labels; birth / death / eps_max):

    1 root (NaN / 8 / 0.25)
    +-- 2 (8 / 4 / 0.5)
    |   +-- 4 (4 / 1    / 1)     flat label 1
    |   +-- 5 (4 / 0.5  / 0.5)   flat label 2
    +-- 3 (8 / 2 / 0.25)         flat label 3
        +-- 6 (2 / 1    / 1)
        +-- 7 (2 / 0.25 / 0.25)

The distances of the hand-worked queries are chosen so that every intermediate value is a power of
two or a sum of two: each expected number below can be checked on paper."""
import functools

import numpy as np
import pytest

from soft_reference import exemplar_distances_ref, exemplars_ref, membership_ref
from test_outlier_scores import bits
from test_predict_host import blob_tree_edges, tie_heavy

NAN, INF = float("nan"), float("inf")

PARENT = np.array([0, 1, 1, 2, 2, 3, 3], np.int32)
BIRTH = np.array([NAN, 8.0, 8.0, 4.0, 4.0, 2.0, 2.0])
DEATH = np.array([8.0, 4.0, 2.0, 1.0, 0.5, 1.0, 0.25])
FLAT = np.array([0, 0, 3, 1, 2, 0, 0], np.int32)
FLAT2 = np.array([0, 2, 0, 0, 0, 1, 0], np.int32)  # cluster 2 -> 2, leaf 6 -> 1; leaf 7 is under nothing
POINT_CLUSTER = np.array([4, 4, 4, 5, 5, 6, 6, 7, 7, 2, 3, 1], np.int32)
POINT_LEVEL = np.array([1.0, 1.0, 2.0, 0.5, 0.75, 1.0, 1.5, 0.25, 0.25, 6.0, 2.5, 9.0])

# (anchor, level, dmin row, prob, vectors, label)
HAND = [
    # anchored at 2, an ancestor of the selected 4 and 5: B = 4, 4, 8; M = 8; dv = 1/4, 1/4, 1/2;
    # p = 1/32, 1/64, 1/64; P = 1/16
    (2, 8.0, [4.0, 4.0, 2.0], 0.125, [0.0625, 0.03125, 0.03125], 1),
    # inside the selected 3 (its leaf 6): B = 8, 8, -inf; M = 8, 8, 1; t = 1/8, 1/16, 1/4;
    # dv = 1/4, 1/2, 1/4; p = 1/32, 1/32, 1/16; P = 1/8
    (6, 1.0, [2.0, 1.0, 2.0], 0.25, [0.0625, 0.0625, 0.125], 3),
    # an exemplar of 4: Z = {1}, dv one-hot; t = 1, 1/8, 1/32
    (4, 1.0, [0.0, 3.0, 5.0], 1.0, [1.0, 0.0, 0.0], 1),
    # a tie in Z of size 2: dv = 1/2, 1/2, 0; t = 1/4, 1/8, 1/32; p = 1/8, 1/16, 0; P = 3/16
    (2, 4.0, [0.0, 0.0, 7.0], 0.25, [0.25 * (0.125 / 0.1875), 0.25 * (0.0625 / 0.1875), 0.0], 1),
    # l == 0 inside 3 (leaf 7), a -0.0 distance: M = 0 gives t = 1
    (7, 0.0, [2.0, 2.0, -0.0], 1.0, [0.0, 0.0, 1.0], 3),
    # no anchor
    (0, 3.0, [1.0, 2.0, 3.0], 0.0, [0.0, 0.0, 0.0], 0),
    # no exemplar anywhere: S == 0, a zero row; prob is still the tree's (0.5 / 1 for its own cluster 5)
    (5, 1.0, [INF, INF, INF], 0.5, [0.0, 0.0, 0.0], 0),
]


def hand_tree(pkg):
    z = np.zeros(7)
    return pkg.ClusterTree(PARENT, BIRTH, DEATH, z, z.astype(np.int32), z.astype(np.int32), FLAT, POINT_CLUSTER,
                           POINT_LEVEL, 3)


def hand_inputs():
    return (np.array([h[0] for h in HAND], np.int32), np.array([h[1] for h in HAND]),
            np.array([h[2] for h in HAND]))


def check_hand(got):
    vec, prob, lab = got
    assert np.asarray(lab).dtype == np.int32
    assert np.array_equal(bits(np.asarray(vec)), bits(np.array([h[4] for h in HAND])))
    assert np.array_equal(bits(np.asarray(prob)), bits(np.array([h[3] for h in HAND])))
    assert np.array_equal(lab, np.array([h[5] for h in HAND], np.int32))


def test_restatement_membership_on_the_hand_tree(pkg):
    check_hand(membership_ref(hand_tree(pkg), *hand_inputs()))


def test_host_membership_on_the_hand_tree(pkg):
    r = pkg.membership_rows(hand_tree(pkg), *hand_inputs())
    check_hand((r.vectors, r.prob, r.labels))
    assert np.array_equal(bits(r.dist), bits(hand_inputs()[2]))


@pytest.mark.parametrize("flat, C, ids, offsets", [(FLAT, 3, [0, 1, 3, 5, 7, 8], [0, 2, 3, 6]),
                                                   (FLAT2, 2, [5, 0, 1, 3], [0, 1, 4])])
def test_exemplars_on_the_hand_tree(pkg, flat, C, ids, offsets):
    t = hand_tree(pkg)
    for got in (exemplars_ref(t, flat, C), pkg.exemplars(t, flat)):
        assert got[0].dtype == np.int32 and got[1].dtype == np.int64
        assert np.array_equal(got[0], np.array(ids, np.int32)) and np.array_equal(got[1], np.array(offsets, np.int64))


def test_exemplars_skip_nan_levels_and_allow_empty_segments(pkg):
    t = hand_tree(pkg)
    t.point_level = POINT_LEVEL.copy()
    t.point_level[3] = NAN  # leaf 5 keeps point 4 at 0.75
    t.point_level[7] = -0.0
    t.point_level[8] = 0.0  # -0.0 == 0.0: both stay exemplars of leaf 7
    flat = np.array([0, 0, 4, 1, 2, 0, 0], np.int32)  # C = 4, flat label 3 carried by no cluster
    want = (np.array([0, 1, 4, 5, 7, 8], np.int32), np.array([0, 2, 3, 3, 6], np.int64))
    for got in (exemplars_ref(t, flat, 4), pkg.exemplars(t, flat)):
        assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1])


# --------------------------------------------------------------------------- trees of real data
CASES = [(300, 2, 40, 4, 2), (420, 3, 60, 4, 4), (600, 3, 150, 4, 25)]  # n, d, duplicates, minPts, minClSize


@functools.lru_cache(maxsize=None)
def fitted(pkg, case):
    n, d, dup, min_pts, mcs = case
    va, vb, w = blob_tree_edges(n, d, dup, min_pts)
    return tie_heavy(n, d, dup), pkg.cluster_tree(va, vb, w, n, mcs)


def constrained_selection(pkg, t, seed):
    """a selection that differs from the tree's own: cannot-link pairs inside the flat clusters"""
    rng = np.random.default_rng(seed)
    lab = t.flat_labels()
    inside = np.flatnonzero(lab > 0)
    a = rng.choice(inside, 40)
    b = np.array([rng.choice(np.flatnonzero(lab == lab[x])) for x in a])
    r = pkg.constrained_flat_labels(t, a.astype(np.int32), b.astype(np.int32), np.ones(40, np.int32))
    return r.flat_label


def selections(pkg, t, case):
    return [("own", None), ("constrained", constrained_selection(pkg, t, case[0]))]


@pytest.mark.parametrize("case", CASES)
def test_host_exemplars_equal_the_restatement(pkg, case):
    X, t = fitted(pkg, case)
    assert t.n_tree > 2
    for name, flat in selections(pkg, t, case):
        ids, off = pkg.exemplars(t, flat)
        want = exemplars_ref(t, flat)
        assert np.array_equal(ids, want[0]) and np.array_equal(off, want[1]), name
        assert ids.shape[0] > 0 and np.all(np.diff(off) >= 0)
        # every exemplar carries its cluster's flat label
        lab = t.flat_labels() if flat is None else pkg.predict_labels(t, np.arange(t.n, dtype=np.int32), t.point_level,
                                                                        flat)[1]
        assert np.array_equal(lab[ids], np.repeat(np.arange(1, off.shape[0]), np.diff(off)))


@pytest.mark.parametrize("case", CASES)
def test_host_membership_equals_the_restatement(pkg, case):
    X, t = fitted(pkg, case)
    rng = np.random.default_rng(case[0] + 1)
    for name, flat in selections(pkg, t, case):
        ids, off = exemplars_ref(t, flat)
        dmin = exemplar_distances_ref(X, ids, off, X)
        # every training point under its own anchor, then arbitrary anchors and levels: clusters
        # anywhere in the tree, levels at births (M == B ties), zero, and no anchor
        anchor = np.r_[t.point_cluster, rng.integers(0, t.n_tree + 1, 200)].astype(np.int32)
        level = np.r_[t.point_level, rng.choice(np.r_[t.birth[1:], 0.0, t.point_level[:5]], 200)]
        rows = np.r_[np.arange(t.n), rng.integers(0, t.n, 200)]
        r = pkg.membership_rows(t, anchor, level, dmin[rows], flat)
        vec, prob, lab = membership_ref(t, anchor, level, dmin[rows], flat)
        assert not np.isnan(vec).any()
        assert np.array_equal(bits(r.vectors), bits(vec)), name
        assert np.array_equal(bits(r.prob), bits(prob)), name
        assert r.labels.dtype == np.int32 and np.array_equal(r.labels, lab), name
        # an exemplar's row is zero off Z and its label is its flat label
        seg = np.repeat(np.arange(1, off.shape[0]), np.diff(off))
        assert np.array_equal(r.labels[ids], seg), name
        assert np.all(r.vectors[ids][dmin[ids] > 0] == 0), name
        assert np.all(r.prob >= 0) and np.all(r.prob <= 1)


def test_host_validation(pkg):
    t = hand_tree(pkg)
    anchor, level, dmin = hand_inputs()
    bad_flat = FLAT.copy()
    bad_flat[4] = 4  # C stays 3 when the call is given C directly
    L = pkg.lib()
    import ctypes as C
    vec = np.full((len(HAND), 3), 7.0)

    def member(flat, an, K=7):
        return L.hdb_membership_vectors(None, pkg._capi.ptr(PARENT), pkg._capi.ptr(BIRTH), pkg._capi.ptr(DEATH),
                                        pkg._capi.ptr(flat), K, 3, pkg._capi.ptr(an), pkg._capi.ptr(level),
                                        pkg._capi.ptr(dmin), len(HAND), pkg._capi.ptr(vec), None, None)

    for flat, an in ((bad_flat, anchor), (np.where(FLAT == 1, -1, FLAT).astype(np.int32), anchor),
                     (FLAT, np.where(anchor == 7, 8, anchor).astype(np.int32)),
                     (FLAT, np.where(anchor == 0, -1, anchor).astype(np.int32))):
        assert member(flat, an) == -1
        assert np.all(vec == 7.0)
    bad_parent = PARENT.copy()
    bad_parent[3] = 5
    ids, off = np.full(12, -7, np.int32), np.full(4, -7, np.int64)
    E = C.c_int64(-7)

    def exemplars(parent, flat, pc):
        return L.hdb_exemplars(None, pkg._capi.ptr(parent), pkg._capi.ptr(flat), 7, 3, pkg._capi.ptr(pc),
                               pkg._capi.ptr(POINT_LEVEL), 12, pkg._capi.ptr(ids), pkg._capi.ptr(off), C.byref(E))

    bad_pc = POINT_CLUSTER.copy()
    bad_pc[5] = 8
    for parent, flat, pc in ((bad_parent, FLAT, POINT_CLUSTER), (PARENT, bad_flat, POINT_CLUSTER),
                             (PARENT, FLAT, bad_pc)):
        assert exemplars(parent, flat, pc) == -1
        assert np.all(ids == -7) and np.all(off == -7) and E.value == -7
    assert exemplars(PARENT, FLAT, POINT_CLUSTER) == 0 and E.value == 6
    # m == 0 and C == 0
    r = pkg.membership_rows(t, anchor[:0], level[:0], dmin[:0])
    assert r.vectors.shape == (0, 3)
    t0 = hand_tree(pkg)
    t0.flat_label, t0.n_clusters = np.zeros(7, np.int32), 0
    r = pkg.membership_rows(t0, anchor, level, np.zeros((len(HAND), 0)))
    assert r.vectors.shape == (len(HAND), 0) and np.all(r.labels == 0)
    assert np.array_equal(r.prob, np.zeros(len(HAND)))
    ids0, off0 = pkg.exemplars(t0)
    assert ids0.shape[0] == 0 and np.array_equal(off0, [0])
