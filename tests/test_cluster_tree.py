"""The cluster tree and the level cuts, host path (csrc/flat.cpp, ctx = NULL).

hdb_flat_cluster_tree exports the condensed tree hdb_flat_labels builds: it must equal the
test-side reference (tests/cluster_tree_reference.py: the plain top-down restatement) in every
array, doubles bit for bit, and stay consistent with flat_labels and outlier_scores.
hdb_labels_at_levels (the walk rule) must equal the reference's label snapshots (brute force, no
walk).  The hierarchy and cluster-tree texts are host formatting."""
import numpy as np
import pytest

from cluster_tree_reference import cluster_tree_reference
from test_outlier_scores import bits, random_tree

NAN = float("nan")
INF = float("inf")

# the issue's known-answer vector: n = 8, minClSize 2, a path
K_EDGES = [(0, 1, 1), (1, 2, 2), (2, 3, 5), (3, 4, 1), (4, 5, 1), (5, 6, 3), (6, 7, 0.5)]
K_VA = np.array([e[0] for e in K_EDGES], np.int32)
K_VB = np.array([e[1] for e in K_EDGES], np.int32)
K_W = np.array([e[2] for e in K_EDGES], np.float64)
K_TREE = dict(
    parent=[0, 1, 1, 3, 3], birth=[NAN, 5, 5, 3, 3], death=[5, 1, 3, 1, 0.5],
    stability=[NAN, 0.3 + 1.6, 5 * (1 / 3 - 1 / 5), 2.0, 3.3333333333333335], size=[8, 3, 5, 3, 2],
    min_id=[0, 0, 3, 3, 6], flat_label=[0, 1, 0, 2, 3], point_cluster=[2, 2, 2, 4, 4, 4, 5, 5],
    point_level=[1, 1, 2, 1, 1, 1, 0.5, 0.5])
K_CUTS = [(7, [1] * 8), (5, [1] * 8), (4, [2, 2, 2, 3, 3, 3, 3, 3]), (2, [2, 2, 2, 4, 4, 4, 5, 5]),
          (1.5, [2, 2, 0, 4, 4, 4, 5, 5]), (0.75, [0, 0, 0, 0, 0, 0, 5, 5]), (0.25, [0] * 8)]
K_HIER = ("5.0,1,1,1,1,1,1,1,1\n3.0,2,2,2,3,3,3,3,3\n2.0,2,2,2,4,4,4,5,5\n0,0,0,0,0,0,0,0,0\n")
K_TEXT = ("1,NaN,5.0,NaN,0,0,0,0\n2,5.0,1.0,1.9000000000000001,0,0,20,1\n3,5.0,3.0,0.6666666666666665,0,0,20,1\n"
          "4,3.0,1.0,2.0,0,0,40,3\n5,3.0,0.5,3.3333333333333335,0,0,40,3\n")
DOUBLES = ("birth", "death", "stability", "point_level")
INTS = ("parent", "size", "min_id", "flat_label", "point_cluster")


def same_tree(t, ref, where=None):
    for k in INTS:
        assert np.array_equal(np.asarray(getattr(t, k)), np.asarray(getattr(ref, k))), (k, where)
    for k in DOUBLES:
        assert np.array_equal(bits(getattr(t, k)), bits(getattr(ref, k))), (k, where, getattr(t, k), getattr(ref, k))
    assert t.n_clusters == ref.n_clusters, where


def test_known_answer_bit_exact(pkg):
    t = pkg.cluster_tree(K_VA, K_VB, K_W, 8, 2)
    assert t.n_tree == 5 and t.n_clusters == 3
    for k in INTS:
        assert np.array_equal(getattr(t, k), np.array(K_TREE[k], np.int32)), k
    for k in DOUBLES:
        assert np.array_equal(bits(getattr(t, k)), bits(K_TREE[k])), (k, getattr(t, k))
    same_tree(t, cluster_tree_reference(K_VA, K_VB, K_W, 8, 2))  # the reference agrees with the hand check too
    assert np.array_equal(pkg.flat_labels(K_VA, K_VB, K_W, 8, 2)[0], [1, 1, 1, 2, 2, 2, 3, 3])
    assert np.array_equal(t.flat_labels(), [1, 1, 1, 2, 2, 2, 3, 3])
    rows = pkg.labels_at_levels(t, [c[0] for c in K_CUTS])
    assert rows.dtype == np.int32 and rows.shape == (len(K_CUTS), 8)
    for (eps, want), row in zip(K_CUTS, rows):
        assert np.array_equal(row, want), eps


def test_known_answer_formats_byte_exact(pkg):
    t = pkg.cluster_tree(K_VA, K_VB, K_W, 8, 2)
    assert pkg.hierarchy_levels(t).tolist() == [5.0, 3.0, 2.0]
    assert pkg.hierarchy_levels(t, compact=False).tolist() == [5.0, 3.0, 2.0, 1.0, 0.5]
    text, offsets = pkg.format_hierarchy(t)
    assert text == K_HIER
    assert offsets.tolist() == [0, 20, 20, 40, 40]
    assert pkg.format_cluster_tree(t, offsets) == K_TEXT
    full, _ = pkg.format_hierarchy(t, compact=False)
    assert full.startswith(K_HIER[:-18]) and full.endswith("1.0,2,2,0,4,4,4,5,5\n0.5,0,0,0,0,0,0,5,5\n" + "0," * 8 + "0\n")


def trees():
    rng = np.random.default_rng(20250307)
    for t in range(240):
        n, mcs = int(rng.integers(2, 61)), int(rng.integers(2, 6))
        yield t, n, mcs, random_tree(rng, n, ties=t % 2 == 1)


def test_host_equals_reference_on_random_trees(pkg):
    split = 0
    for t, n, mcs, (va, vb, w) in trees():
        tr = pkg.cluster_tree(va, vb, w, n, mcs)
        ref = cluster_tree_reference(va, vb, w, n, mcs)
        same_tree(tr, ref, (t, n, mcs))
        K = tr.n_tree
        assert 1 <= K <= pkg.cluster_tree_bound(n, mcs) == max(1, 2 * (n // mcs) - 1)
        assert np.all(tr.parent[1:] < np.arange(2, K + 1)) and np.all(tr.parent[1:] >= 1) and tr.parent[0] == 0
        split += K > 1
    assert split > 100


def test_consistent_with_flat_labels_and_outlier_scores(pkg):
    for t, n, mcs, (va, vb, w) in trees():
        tr = pkg.cluster_tree(va, vb, w, n, mcs)
        labels, k = pkg.flat_labels(va, vb, w, n, mcs)
        assert np.array_equal(tr.flat_labels(), labels) and tr.n_clusters == k, t
        assert np.array_equal(cluster_tree_reference(va, vb, w, n, mcs).flat, labels), t
        s, e = pkg.outlier_scores(va, vb, w, n, mcs)
        assert np.array_equal(bits(tr.point_level), bits(e)), t
        with np.errstate(over="ignore", invalid="ignore", divide="ignore"):
            assert np.array_equal(bits(tr.outlier_scores()), bits(s)), t


def test_cuts_equal_the_snapshots(pkg):
    rng = np.random.default_rng(5)
    for t, n, mcs, (va, vb, w) in trees():
        tr = pkg.cluster_tree(va, vb, w, n, mcs)
        ref = cluster_tree_reference(va, vb, w, n, mcs)
        proc = [lv for lv, _ in ref.snapshots]  # every level, descending
        rows = pkg.labels_at_levels(tr, proc)
        for (lv, snap), row in zip(ref.snapshots, rows):
            assert np.array_equal(row, snap), (t, lv)
        # the reference's processed levels are the point levels and the birth levels, and cover every row
        assert set(pkg.hierarchy_levels(tr, compact=False).tolist()) <= set(proc)
        mids = [(a + b) / 2 for a, b in zip(proc, proc[1:])]
        extra = mids + [proc[0] + 1, proc[-1] - 1, INF, -INF] + [proc[0], proc[0]] + rng.random(3).tolist()
        extra += [float(x) for x in tr.birth[1:3]] + [float(x) for x in tr.point_level[:2]]  # exactly at a birth / a point level
        order = rng.permutation(len(extra))  # unsorted, with duplicates
        extra = [extra[i] for i in order]
        rows = pkg.labels_at_levels(tr, extra)
        for eps, row in zip(extra, rows):
            assert np.array_equal(row, ref.cut(eps)), (t, eps)
        assert np.all(rows[[i for i, e in enumerate(extra) if e == INF]] == 1)
        assert np.all(rows[[i for i, e in enumerate(extra) if e == -INF]] == 0)


def path(ws):
    n = len(ws) + 1
    return np.arange(n - 1, dtype=np.int32), np.arange(1, n, dtype=np.int32), np.array(ws, np.float64)


def test_degenerate_inputs(pkg):
    e = np.zeros(0, np.int32)
    t = pkg.cluster_tree(e, e, np.zeros(0), 0, 2)
    assert t.n_tree == 0 and t.n == 0 and t.n_clusters == 0
    assert pkg.labels_at_levels(t, [1.0]).shape == (1, 0)
    t = pkg.cluster_tree(e, e, np.zeros(0), 1, 2)  # one point: the root alone, no level
    assert t.n_tree == 1 and t.parent.tolist() == [0] and t.size.tolist() == [1] and t.min_id.tolist() == [0]
    assert np.isnan(t.birth[0]) and bits(t.death)[0] == 0 and t.flat_label.tolist() == [0]
    assert t.point_cluster.tolist() == [1] and bits(t.point_level)[0] == 0
    assert pkg.labels_at_levels(t, [-1.0, 0.0, 1.0]).tolist() == [[0], [1], [1]]
    assert pkg.format_hierarchy(t)[0] == "0.0,1\n0,0\n"
    for n, mcs, ws in [(2, 2, [3.0]), (3, 4, [1.0, 2.0]), (4, 5, [2.0, 7.0, 7.0])]:  # n = 2; n < minClSize
        t = pkg.cluster_tree(*path(ws), n, mcs)
        same_tree(t, cluster_tree_reference(*path(ws), n, mcs))
        top = max(ws)
        assert t.n_tree == 1 and np.all(t.point_cluster == 1) and np.all(t.point_level == top) and t.death[0] == top
        assert np.isnan(t.stability[0]) and t.n_clusters == 0
        assert pkg.labels_at_levels(t, [top, np.nextafter(top, 0)]).tolist() == [[1] * n, [0] * n]
    # a root that never splits: one valid part at every level
    va, vb, w = path([5.0, 4.0, 3.0, 2.0, 1.0])
    t = pkg.cluster_tree(va, vb, w, 6, 3)
    same_tree(t, cluster_tree_reference(va, vb, w, 6, 3))
    assert t.n_tree == 1 and t.point_level.tolist() == [5.0, 4.0, 3.0, 2.0, 2.0, 2.0] and t.death[0] == 2.0
    # one tie group for all edges
    va, vb, w = path([2.0] * 6)
    t = pkg.cluster_tree(va, vb, w, 7, 2)
    same_tree(t, cluster_tree_reference(va, vb, w, 7, 2))
    assert t.n_tree == 1 and np.all(t.point_level == 2.0)
    # zero weights: duplicate points; an infinite stability comes out as computed
    va, vb, w = path([0.0, 0.0, 3.0, 0.0, 4.0, 0.0, -0.0])
    t = pkg.cluster_tree(va, vb, w, 8, 2)
    with np.errstate(divide="ignore"):
        same_tree(t, cluster_tree_reference(va, vb, np.abs(w), 8, 2))
    assert np.isinf(t.stability[1:]).any() and not np.signbit(t.point_level).any() and not np.signbit(t.death).any()
    assert "Infinity" in pkg.format_cluster_tree(t)


def raw_tree(pkg, va, vb, w, n, mcs, cap):
    L = pkg.lib()
    par = np.full(max(cap, 1) + 2, -7, np.int32)
    kt = np.full(1, -1, np.int64)
    rc = L.hdb_flat_cluster_tree(None, va.ctypes.data, vb.ctypes.data, w.ctypes.data, w.shape[0], n, mcs, cap,
                                 kt.ctypes.data, par.ctypes.data, *[None] * 9)
    return rc, int(kt[0]), par, L.hdb_last_error().decode()


def test_statuses(pkg):
    rc, K, par, msg = raw_tree(pkg, K_VA, K_VB, K_W, 8, 2, 4)  # cap < K
    assert rc == -1 and K == 5 and "4" in msg and "5" in msg and np.all(par[4:] == -7)
    rc, K, par, _ = raw_tree(pkg, K_VA, K_VB, K_W, 8, 2, 5)  # nullable outputs: the parents alone
    assert rc == 0 and K == 5 and par[:5].tolist() == [0, 1, 1, 3, 3] and np.all(par[5:] == -7)
    t = pkg.cluster_tree(K_VA, K_VB, K_W, 8, 2)
    with pytest.raises(pkg.HdbError, match="NaN level"):
        pkg.labels_at_levels(t, [1.0, NAN])
    assert pkg.labels_at_levels(t, []).shape == (0, 8)
    for field, bad in [("point_cluster", [2, 2, 2, 4, 4, 4, 5, 6]), ("point_cluster", [0, 2, 2, 4, 4, 4, 5, 5]),
                       ("point_cluster", [2, 2, -3, 4, 4, 4, 5, 5]), ("parent", [0, 1, 1, 4, 3]),
                       ("parent", [0, 1, 1, 3, -1]), ("parent", [1, 1, 1, 3, 3]), ("parent", [0, 1, 1, 3, 9])]:
        t2 = pkg.cluster_tree(K_VA, K_VB, K_W, 8, 2)
        setattr(t2, field, np.array(bad, np.int32))
        with pytest.raises(pkg.HdbError, match="out of range|must have parent 0") as ei:
            pkg.labels_at_levels(t2, [2.0])
        assert ei.value.code == -1
    # the input errors of hdb_flat_labels, unchanged
    cases = [(K_VA[:-1], K_VB[:-1], K_W[:-1], 8, 2), (K_VA, K_VB, K_W, 8, 1),
             (np.where(np.arange(7) == 0, 11, K_VA).astype(np.int32), K_VB, K_W, 8, 2),
             (K_VA, K_VB, np.where(np.arange(7) == 2, NAN, K_W), 8, 2),
             (np.array([0, 1, 0, 3, 4, 5, 6], np.int32), np.array([1, 2, 2, 4, 5, 6, 7], np.int32), K_W, 8, 2)]
    for va, vb, w, n, mcs in cases:
        with pytest.raises(pkg.HdbError) as e1:
            pkg.flat_labels(va, vb, w, n, mcs)
        with pytest.raises(pkg.HdbError) as e2:
            pkg.cluster_tree(va, vb, w, n, mcs)
        assert e1.value.code == e2.value.code == -1
        assert str(e1.value).split(": ", 2)[-1] == str(e2.value).split(": ", 2)[-1]
