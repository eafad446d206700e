"""hdb_predict_labels, host path (csrc/flat.cpp, ctx = NULL): out-of-sample labels read out of a
cluster tree.

Identity: a training point attached to itself at its own level gets its own last cluster, flat
label and GLOSH score (bit for bit).  Level cuts: for any level at or above the point's own, the
tree label is the row of labels_at_levels.  Everything equals the plain-loop restatement
(tests/predict_ref.py), and the hand-worked trees, the empty input and every validation error
behave as include/hdbmi.h states."""
import functools

import numpy as np
import pytest

from metric_kruskal import rounded_blobs
from path_helpers import kruskal_mst
from predict_ref import JMAX, predict_ref
from test_cluster_tree import K_VA, K_VB, K_W
from test_outlier_scores import bits

NAN = float("nan")
INF = float("inf")


def tie_heavy(n, d, dup):
    """rounded blobs whose first `dup` rows appear twice"""
    X = rounded_blobs(n - dup, d)
    return np.ascontiguousarray(np.vstack([X, X[:dup]]), np.float64)


@functools.lru_cache(maxsize=None)
def blob_tree_edges(n, d, dup, min_pts):
    """(va, vb, w) of the exact MRD MST of tie_heavy(n, d, dup), oracle cores, computed once"""
    from oracle import oracle as O
    X = tie_heavy(n, d, dup)
    core = O.core_distances(X, min_pts)
    lo, hi, w = kruskal_mst(X, core)
    return np.asarray(lo, np.int32), np.asarray(hi, np.int32), np.asarray(w, np.float64)


CASES = [(300, 2, 40, 4, 5), (257, 3, 0, 2, 2), (180, 5, 90, 4, 3)]  # n, d, duplicates, minPts, minClSize


def same_prediction(got, want, where=None):
    for g, w, k in zip(got, want, ("tree_label", "labels", "scores")):
        if k == "scores":
            assert np.array_equal(bits(g), bits(w)), (k, where)
        else:
            assert np.asarray(g).dtype == np.int32 and np.array_equal(g, w), (k, where)


@pytest.mark.parametrize("case", CASES)
def test_identity_property(pkg, case):
    n, d, dup, min_pts, mcs = case
    va, vb, w = blob_tree_edges(n, d, dup, min_pts)
    t = pkg.cluster_tree(va, vb, w, n, mcs)
    assert t.n_tree > 1
    tl, lab, sc = pkg.predict_labels(t, np.arange(n, dtype=np.int32), t.point_level)
    assert np.array_equal(tl, t.point_cluster)
    assert np.array_equal(lab, t.flat_labels())
    assert np.array_equal(lab, pkg.flat_labels(va, vb, w, n, mcs)[0])
    with np.errstate(all="ignore"):
        assert np.array_equal(bits(sc), bits(t.outlier_scores()))
    assert np.array_equal(bits(sc), bits(pkg.outlier_scores(va, vb, w, n, mcs)[0]))
    same_prediction((tl, lab, sc), predict_ref(t, np.arange(n), t.point_level), case)


@pytest.mark.parametrize("case", CASES)
def test_level_cut_property(pkg, case):
    n, d, dup, min_pts, mcs = case
    va, vb, w = blob_tree_edges(n, d, dup, min_pts)
    t = pkg.cluster_tree(va, vb, w, n, mcs)
    rng = np.random.default_rng(n)
    births = t.birth[1:]
    below = min(float(t.point_level.min()), float(births.min())) - 1.0
    levels = np.r_[births[:: max(1, births.shape[0] // 12)], INF, below, rng.uniform(0, float(w.max()) * 1.1, 6),
                   t.point_level[:3]]
    rows = pkg.labels_at_levels(t, levels)
    for e, row in zip(levels.tolist(), rows):
        y = np.flatnonzero(t.point_level <= e).astype(np.int32)  # the cut's noise rule is not predict's
        lv = np.full(y.shape[0], e)
        tl, lab, sc = pkg.predict_labels(t, y, lv)
        assert np.array_equal(tl, row[y]), e
        same_prediction((tl, lab, sc), predict_ref(t, y, lv), e)
        if e == INF:
            assert y.shape[0] == n and np.all(tl == 1) and np.all(lab == 0)
    # a level below every level: the walk does not move, whatever point is asked
    y = np.arange(n, dtype=np.int32)
    tl, lab, sc = pkg.predict_labels(t, y, np.full(n, below))
    assert np.array_equal(tl, t.point_cluster) and np.array_equal(lab, t.flat_labels())
    same_prediction((tl, lab, sc), predict_ref(t, y, np.full(n, below)))


def test_known_tree_by_hand(pkg):
    """test_cluster_tree's n = 8 path: parent [0,1,1,3,3], birth [NaN,5,5,3,3], death [5,1,3,1,0.5],
    flat_label [0,1,0,2,3], point_cluster [2,2,2,4,4,4,5,5], point_level [1,1,2,1,1,1,.5,.5]"""
    t = pkg.cluster_tree(K_VA, K_VB, K_W, 8, 2)
    nearest = np.array([0, 0, 3, 3, 3, 6, 6, 2, -1], np.int32)
    level = np.array([0.25, 5.0, 2.9, 3.0, 4.9, 3.0, 7.0, 2.0, NAN])
    tl, lab, sc = pkg.predict_labels(t, nearest, level)
    assert tl.tolist() == [2, 1, 4, 3, 3, 3, 1, 2, 0]
    assert lab.tolist() == [1, 0, 2, 0, 0, 0, 0, 1, 0]
    # eps_max by label: root min(1, 3, 1, .5) = .5, 2: 1, 3: .5, 4: 1, 5: .5; eps = max(level, point_level)
    want = [1 - 1 / 1.0, 1 - 0.5 / 5.0, 1 - 1 / 2.9, 1 - 0.5 / 3.0, 1 - 0.5 / 4.9, 1 - 0.5 / 3.0, 1 - 0.5 / 7.0,
            1 - 1 / 2.0, 1.0]
    assert np.array_equal(bits(sc), bits(want))
    same_prediction((tl, lab, sc), predict_ref(t, nearest, level))


def test_root_that_never_splits(pkg):
    """K = 1: every query lands in the root, label 0, eps_max = Double.MAX_VALUE"""
    va, vb, w = np.arange(4, dtype=np.int32), np.arange(1, 5, dtype=np.int32), np.array([1.0, 2.0, 3.0, 4.0])
    t = pkg.cluster_tree(va, vb, w, 5, 4)
    assert t.n_tree == 1
    nearest, level = np.array([0, 4, 2, -1], np.int32), np.array([0.5, 9.0, INF, 1.0])
    tl, lab, sc = pkg.predict_labels(t, nearest, level)
    assert tl.tolist() == [1, 1, 1, 0] and lab.tolist() == [0, 0, 0, 0]
    with np.errstate(over="ignore"):
        eps = np.maximum(level[:3], t.point_level[nearest[:3]])
        assert np.array_equal(bits(sc), bits(np.r_[1.0 - JMAX / eps, 1.0]))
    # a zero level on a zero-level point scores 0
    t1 = pkg.cluster_tree(np.zeros(0, np.int32), np.zeros(0, np.int32), np.zeros(0), 1, 2)
    tl, lab, sc = pkg.predict_labels(t1, [0], [0.0])
    assert tl.tolist() == [1] and lab.tolist() == [0] and bits(sc).tolist() == bits([0.0]).tolist()
    tl, lab, sc = pkg.predict_labels(t1, [0], [-0.0])
    assert bits(sc).tolist() == bits([0.0]).tolist()


def test_empty_and_null_outputs(pkg):
    import ctypes as C
    t = pkg.cluster_tree(K_VA, K_VB, K_W, 8, 2)
    tl, lab, sc = pkg.predict_labels(t, np.zeros(0, np.int32), np.zeros(0))
    assert tl.shape == lab.shape == sc.shape == (0,)
    A, L = pkg._capi, pkg.lib()
    # m == 0 is HDB_OK even with nothing else given
    assert L.hdb_predict_labels(None, None, None, None, None, 0, None, None, 0, None, None, 0, None, None, None) == 0
    nearest, level = np.array([0, 6, -1], np.int32), np.array([4.0, 0.5, 1.0])
    full = pkg.predict_labels(t, nearest, level)
    args = [A.ptr(np.ascontiguousarray(getattr(t, k))) for k in ("parent", "birth", "death", "flat_label")]
    pc, pl = A.ptr(np.ascontiguousarray(t.point_cluster)), A.ptr(np.ascontiguousarray(t.point_level))
    for keep in range(3):  # every output may be NULL on its own
        outs = [np.empty(3, np.int32), np.empty(3, np.int32), np.empty(3, np.float64)]
        ptrs = [A.ptr(o) if k == keep else None for k, o in enumerate(outs)]
        assert L.hdb_predict_labels(None, *args, 5, pc, pl, 8, A.ptr(nearest), A.ptr(level), 3, *ptrs) == 0
        assert np.array_equal(outs[keep], full[keep])
    assert L.hdb_predict_labels(None, *args, 5, pc, pl, 8, A.ptr(nearest), A.ptr(level), 3, None, None, None) == 0
    # n == 0: only queries without a neighbour are possible
    t0 = pkg.cluster_tree(np.zeros(0, np.int32), np.zeros(0, np.int32), np.zeros(0), 0, 2)
    tl, lab, sc = pkg.predict_labels(t0, [-1, -1], [1.0, NAN])
    assert tl.tolist() == [0, 0] and lab.tolist() == [0, 0] and sc.tolist() == [1.0, 1.0]


class Tree:
    def __init__(self, t, **kw):
        for k in ("parent", "birth", "death", "flat_label", "point_cluster", "point_level"):
            setattr(self, k, np.array(kw.get(k, getattr(t, k))))


BAD = [
    (dict(nearest=[8]), "nearest"), (dict(nearest=[-2]), "nearest"), (dict(nearest=[0, 2 ** 31 - 1]), "nearest"),
    (dict(level=[NAN]), "level"),
    (dict(point_cluster=[2, 2, 2, 4, 4, 4, 5, 6]), "point_cluster"), (dict(point_cluster=[0] * 8), "point_cluster"),
    (dict(parent=[1, 1, 1, 3, 3]), "parent"), (dict(parent=[0, 1, 3, 3, 3]), "parent"),
    (dict(parent=[0, 1, 1, 3, -1]), "parent"),
]


@pytest.mark.parametrize("change,field", BAD)
def test_validation_errors(pkg, change, field):
    t = pkg.cluster_tree(K_VA, K_VB, K_W, 8, 2)
    nearest = np.array(change.get("nearest", [0]), np.int32)
    level = np.array(change.get("level", [1.0] * nearest.shape[0]), np.float64)
    bad = Tree(t, **{k: np.array(v, np.int32) for k, v in change.items() if k in ("parent", "point_cluster")})
    with pytest.raises(pkg.HdbError, match=field) as ei:
        pkg.predict_labels(bad, nearest, level)
    assert ei.value.code == -1
    # a NaN level is only an error where there is a neighbour
    tl, _, sc = pkg.predict_labels(t, [-1, 0], [NAN, 1.0])
    assert tl.tolist() == [0, 2] and sc[0] == 1.0


def test_constrained_flat_label(pkg):
    """flat_label may be the selection of constrained_flat_labels: the training points attached to
    themselves then get the constrained partition"""
    n, d, dup, min_pts, mcs = CASES[0]
    va, vb, w = blob_tree_edges(n, d, dup, min_pts)
    t = pkg.cluster_tree(va, vb, w, n, mcs)
    base = t.flat_labels()
    # two selected siblings below a cluster that is not the root: must-links across them move the
    # selection up to their parent
    sel = np.flatnonzero((t.flat_label != 0) & (t.parent > 1))
    pairs = [(c, s) for c in sel for s in sel if c < s and t.parent[c] == t.parent[s]]
    assert pairs
    c, s = pairs[0]
    a = np.flatnonzero(base == t.flat_label[c])[:4]
    b = np.flatnonzero(base == t.flat_label[s])[:4]
    k = min(a.shape[0], b.shape[0])
    res = pkg.constrained_flat_labels(t, a[:k].astype(np.int32), b[:k].astype(np.int32), np.zeros(k, np.int32))
    assert not np.array_equal(res.labels, base)
    y = np.arange(n, dtype=np.int32)
    tl, lab, sc = pkg.predict_labels(t, y, t.point_level, flat_label=res.flat_label)
    assert np.array_equal(lab, res.labels) and np.array_equal(tl, t.point_cluster)
    same_prediction((tl, lab, sc), predict_ref(t, y, t.point_level, res.flat_label))
