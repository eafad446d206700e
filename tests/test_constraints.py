"""Constraint-aware (semi-supervised) flat extraction, host path (csrc/constraints.cpp, ctx =
NULL): hdb_constrained_flat_labels over the arrays of hdb_flat_cluster_tree must equal the
hand-worked vectors below in every output, the top-down restatement of the Java rule
(tests/constraints_reference.py) on random trees, doubles bit for bit, and with no constraints
the unconstrained selection exactly.  parse_constraints and the constraint columns of the
cluster-tree text are host formatting."""
import ctypes as C

import numpy as np
import pytest

from cluster_tree_reference import cluster_tree_reference
from constraints_reference import big_tree, constraints_reference, random_constraints
from test_cluster_tree import K_TEXT, K_VA, K_VB, K_W
from test_outlier_scores import bits

ML, CL = 0, 1
ARRAYS = ("num_sat", "prop_sat", "flat_label", "labels")

# Tree A: the known-answer tree of test_cluster_tree.py (n = 8, minClSize 2).  Tree labels:
# 1 = root, 2 = {0,1,2}, 3 = {3..7} with children 4 = {3,4,5} and 5 = {6,7}; no point leaves 1 or
# 3 as noise.  By stability alone the children of 3 win (0.67 < 2.0 + 3.33).
A_STAB = [float("nan"), 0.3 + 1.6, 5 * (1 / 3 - 1 / 5), 2.0, 3.3333333333333335]
# Tree B: the same shape with point 8 hung on point 3 at weight 4 -- it leaves cluster 3 as noise
# before 3 splits (the virtual child of 3) -- and inner weights 2.5, so that by stability alone
# cluster 3 is kept (0.72 >= 0.2 + 0.13).
B_EDGES = [(0, 1, 1), (1, 2, 2), (2, 3, 5), (3, 4, 2.5), (4, 5, 2.5), (5, 6, 3), (6, 7, 2.5), (3, 8, 4)]
B_STAB = [float("nan"), 0.3 + 1.6, 1 * (1 / 4 - 1 / 5) + 5 * (1 / 3 - 1 / 5), 3 * (1 / 2.5 - 1 / 3), 2 * (1 / 2.5 - 1 / 3)]

# (tree, constraints (a, b, type), num_sat, prop_sat, prop_stability as (tree stabilities) -> list,
#  flat_label, labels, satisfied fraction)
HAND = [
    # A1.  ML(3,6): LCA 3 -> 3 and the root gain 2: the parent beats children that stability
    # alone prefers.  ML(0,3): across two children of the root, only the root gains.  ML(1,1):
    # a == b, cluster 2 and the root gain 2.  CL(6,6): a == b in a leaf: nothing (its virtual
    # child is never read).  CL(0,7): LCA root: 2 gains 1; 5 and 3 gain 1.
    ("A", [(3, 6, ML), (0, 3, ML), (1, 1, ML), (6, 6, CL), (0, 7, CL)],
     [6, 3, 3, 0, 1], [6, 0, 1, 0, 0], lambda s: [0.0 + s[1] + s[2], 0.0, 0.0 + s[3] + s[4], 0.0, 0.0],
     [0, 1, 2, 0, 0], [1, 1, 1, 2, 2, 2, 2, 2], 0.5 * 6 / 5),
    # A2.  CL(3,6) gives 4 and 5 one each, ML(4,7) gives 3 two: the counts tie at 2, stability
    # decides, and on tree A it prefers the children.
    ("A", [(3, 6, CL), (4, 7, ML)],
     [2, 0, 2, 1, 1], [2, 0, 2, 0, 0], lambda s: [0.0 + s[1] + (0.0 + s[3] + s[4]), 0.0, 0.0 + s[3] + s[4], 0.0, 0.0],
     [0, 1, 0, 2, 3], [1, 1, 1, 2, 2, 2, 3, 3], 0.5 * 2 / 2),
    # B1.  CL(3,6): 4 and 5 gain 1: the children beat a parent that stability alone keeps.
    # CL(8,0): 8 is noise that left 3: its virtual child gains 1 (cluster 3 splits), 3 gains 1 on
    # the path to the root, 2 gains 1.  CL(8,8): a == b, both endpoints in the virtual child of 3.
    # ML(2,2): 2 and the root gain 2.
    ("B", [(3, 6, CL), (8, 0, CL), (8, 8, CL), (2, 2, ML)],
     [2, 3, 1, 1, 1], [8, 0, 5, 0, 0], lambda s: [0.0 + s[1] + (0.0 + s[3] + s[4]), 0.0, 0.0 + s[3] + s[4], 0.0, 0.0],
     [0, 1, 0, 2, 3], [1, 1, 1, 2, 2, 2, 3, 3, 0], 0.5 * 8 / 4),
    # B2.  the tie of A2 on tree B: stability keeps the parent, and point 8 is labelled with it.
    ("B", [(3, 6, CL), (4, 7, ML)],
     [2, 0, 2, 1, 1], [2, 0, 2, 0, 0], lambda s: [0.0 + s[1] + s[2], 0.0, 0.0 + s[3] + s[4], 0.0, 0.0],
     [0, 1, 2, 0, 0], [1, 1, 1, 2, 2, 2, 2, 2, 2], 0.5 * 2 / 2),
]


def hand_tree(pkg, which):
    if which == "A":
        t = pkg.cluster_tree(K_VA, K_VB, K_W, 8, 2)
        want, pc = A_STAB, [2, 2, 2, 4, 4, 4, 5, 5]
        ref = cluster_tree_reference(K_VA, K_VB, K_W, 8, 2)
    else:
        va, vb, w = (np.array([e[k] for e in B_EDGES], dt) for k, dt in ((0, np.int32), (1, np.int32), (2, np.float64)))
        t = pkg.cluster_tree(va, vb, w, 9, 2)
        want, pc = B_STAB, [2, 2, 2, 4, 4, 4, 5, 5, 3]
        ref = cluster_tree_reference(va, vb, w, 9, 2)
    # the tree the hand work assumes
    assert t.parent.tolist() == [0, 1, 1, 3, 3] and t.point_cluster.tolist() == pc and t.min_id.tolist() == [0, 0, 3, 3, 6]
    assert np.array_equal(bits(t.stability), bits(want))
    return t, ref


def cons(rows):
    a = np.array(rows, np.int32).reshape(-1, 3)
    return a[:, 0].copy(), a[:, 1].copy(), a[:, 2].copy()


def same_result(got, want, where=None):
    for k in ARRAYS:
        assert np.array_equal(np.asarray(getattr(got, k)), np.asarray(getattr(want, k))), (k, where)
    assert np.array_equal(bits(got.prop_stability), bits(want.prop_stability)), (where, got.prop_stability)
    assert got.n_clusters == want.n_clusters, where


@pytest.mark.parametrize("case", range(len(HAND)))
def test_hand_worked_vectors(pkg, case):
    which, rows, num, prop, pstab, flat, labels, frac = HAND[case]
    t, ref = hand_tree(pkg, which)
    r = pkg.constrained_flat_labels(t, *cons(rows))
    assert r.num_sat.tolist() == num and r.prop_sat.tolist() == prop
    assert np.array_equal(bits(r.prop_stability), bits(pstab(t.stability.tolist())))
    assert r.flat_label.tolist() == flat and r.labels.tolist() == labels and r.n_clusters == max(flat)
    assert r.num_sat.dtype == r.prop_sat.dtype == r.flat_label.dtype == r.labels.dtype == np.int32
    assert r.satisfied_fraction == frac and r.m == len(rows)
    same_result(r, constraints_reference(ref, *cons(rows)), case)  # the reference agrees with the hand work too
    # the unconstrained selections the cases are set against
    assert t.flat_label.tolist() == ([0, 1, 0, 2, 3] if which == "A" else [0, 1, 2, 0, 0])


@pytest.fixture(scope="module")
def trees2000(pkg):
    """(ties, mcs) -> (host tree, reference tree); the O(levels x n) reference once each"""
    out = {}
    for ties in (False, True):
        va, vb, w = big_tree(2000, 6 if ties else None, 7 + ties)
        for mcs in (2, 5):
            out[ties, mcs] = (pkg.cluster_tree(va, vb, w, 2000, mcs), cluster_tree_reference(va, vb, w, 2000, mcs))
    return out


def test_host_equals_reference_on_random_trees(pkg, trees2000):
    differs = cases = 0
    for (ties, mcs), (t, ref) in trees2000.items():
        for m in (1, 64, 5000):
            c = random_constraints(2000, m, 100 * m + mcs + ties)
            r = pkg.constrained_flat_labels(t, *c)
            same_result(r, constraints_reference(ref, *c), (ties, mcs, m))
            assert 0 <= r.prop_sat.min() and r.prop_sat.max() <= 2 * m and 0 <= r.num_sat.min() and r.num_sat.max() <= 2 * m
            cases += 1
            differs += not np.array_equal(r.flat_label, t.flat_label)
    # not vacuous: the constrained rule changes the selection (42 of 48 such inputs in the design check)
    assert cases == 12 and differs >= 6, differs


def test_no_constraints_is_the_unconstrained_selection(pkg, trees2000):
    e = np.zeros(0, np.int32)
    big = big_tree(20000, 50, 11)
    cases = [(t, None) for t, _ in trees2000.values()] + [(pkg.cluster_tree(*big, 20000, 3), big)]
    for t, edges in cases:
        r = pkg.constrained_flat_labels(t, e, e, e)
        assert np.array_equal(r.flat_label, t.flat_label) and r.n_clusters == t.n_clusters
        assert np.array_equal(r.labels, t.flat_labels())
        assert not r.num_sat.any() and not r.prop_sat.any() and np.isnan(r.satisfied_fraction)
        if edges is not None:
            assert np.array_equal(r.labels, pkg.flat_labels(*edges, 20000, 3)[0])


def raw(pkg, t, ca, cb, ct, m=None, outs="nplfLk", ctx=None, K=None, n=None):
    """the C call with chosen outputs (n: num_sat, p: prop_sat, l: prop_stability, f: flat_label,
    L: labels, k: n_clusters); returns (status, message, outputs by letter)"""
    K = t.n_tree if K is None else K
    n = t.n if n is None else n
    arr = dict(n=np.full(K + 1, -7, np.int32), p=np.full(K + 1, -7, np.int32), l=np.full(K + 1, -7.0),
               f=np.full(K + 1, -7, np.int32), L=np.full(n + 1, -7, np.int32), k=np.full(1, -7, np.int64))
    p = lambda x: C.c_void_p(np.ascontiguousarray(x).ctypes.data)
    keep = [np.ascontiguousarray(x) for x in (t.parent, t.stability, t.min_id, t.point_cluster, ca, cb, ct)]
    L = pkg.lib()
    rc = L.hdb_constrained_flat_labels(ctx, *[p(x) for x in keep[:3]], K, p(keep[3]), n, *[p(x) for x in keep[4:]],
                                       len(ca) if m is None else m,
                                       *[p(arr[c]) if c in outs else None for c in "nplfLk"])
    return rc, L.hdb_last_error().decode(), arr


def test_statuses_and_validation(pkg):
    t, _ = hand_tree(pkg, "A")
    one = np.zeros(1, np.int32)
    rc, msg, arr = raw(pkg, t, one, one, one, m=2 ** 30)  # checked before any array is read
    assert rc == -1 and "2^30" in msg and all(np.all(a == -7) for a in arr.values())
    assert raw(pkg, t, one, one, one, m=1)[0] == 0  # the same arrays are fine
    assert raw(pkg, t, one, one, one, m=-1)[0] == -1
    ca, cb, ct = cons(HAND[0][1])
    bad = [("parent", [1, 1, 1, 3, 3], "parent"), ("parent", [0, 1, 1, 4, 3], "parent"), ("parent", [0, 1, 1, 3, -1], "parent"),
           ("parent", [0, 1, 1, 3, 9], "parent"), ("point_cluster", [2, 2, 2, 4, 4, 4, 5, 6], "point_cluster"),
           ("point_cluster", [0, 2, 2, 4, 4, 4, 5, 5], "point_cluster"), ("point_cluster", [2, 2, -3, 4, 4, 4, 5, 5], "point_cluster")]
    for field, values, word in bad:
        t2, _ = hand_tree(pkg, "A")
        setattr(t2, field, np.array(values, np.int32))
        with pytest.raises(pkg.HdbError, match=word) as ei:
            pkg.constrained_flat_labels(t2, ca, cb, ct)
        assert ei.value.code == -1
    for k, (a, b, ty, word) in enumerate([(8, 0, ML, "point id"), (0, -1, CL, "point id"), (0, 2 ** 31 - 1, ML, "point id"),
                                          (0, 1, 2, "ctype"), (0, 1, -1, "ctype")]):
        xa, xb, xt = ca.copy(), cb.copy(), ct.copy()
        xa[k % 5], xb[k % 5], xt[k % 5] = a, b, ty
        with pytest.raises(pkg.HdbError, match=word) as ei:
            pkg.constrained_flat_labels(t, xa, xb, xt)
        assert ei.value.code == -1
    with pytest.raises(ValueError):
        pkg.constrained_flat_labels(t, ca, cb[:-1], ct)
    # every output may be NULL on its own; the others are written as with all of them
    rc, _, full = raw(pkg, t, ca, cb, ct)
    assert rc == 0 and full["k"][0] == 2 and full["n"][:5].tolist() == HAND[0][2] and full["n"][5] == -7 and full["L"][8] == -7
    for skip in "nplfLk":
        rc, _, arr = raw(pkg, t, ca, cb, ct, outs="nplfLk".replace(skip, ""))
        assert rc == 0 and np.all(arr[skip] == -7)
        for c in "nplfLk".replace(skip, ""):
            assert np.array_equal(arr[c], full[c]), (skip, c)
    assert raw(pkg, t, ca, cb, ct, outs="")[0] == 0


def test_degenerate_trees(pkg):
    e = np.zeros(0, np.int32)
    # K = 1: nothing below the root to select; the root still counts its must-links
    va, vb, w = np.arange(3, dtype=np.int32), np.arange(1, 4, dtype=np.int32), np.array([2.0, 7.0, 7.0])
    t = pkg.cluster_tree(va, vb, w, 4, 5)
    assert t.n_tree == 1
    r = pkg.constrained_flat_labels(t, *cons([(0, 1, ML), (2, 2, ML), (0, 3, CL), (1, 1, CL)]))
    assert r.n_clusters == 0 and r.labels.tolist() == [0] * 4 and r.num_sat.tolist() == [4] and r.flat_label.tolist() == [0]
    assert r.prop_sat.tolist() == [0] and bits(r.prop_stability)[0] == 0  # a root without children is a leaf
    # n = 0: no tree at all
    t0 = pkg.cluster_tree(e, e, np.zeros(0), 0, 2)
    r = pkg.constrained_flat_labels(t0, e, e, e)
    assert r.n_clusters == 0 and r.labels.shape == (0,) and r.num_sat.shape == (0,) and np.isnan(r.satisfied_fraction)
    # n = 1: the root alone
    with pytest.raises(pkg.HdbError, match="point id"):
        pkg.constrained_flat_labels(pkg.cluster_tree(e, e, np.zeros(0), 1, 2), *cons([(0, 1, ML)]))
    r = pkg.constrained_flat_labels(pkg.cluster_tree(e, e, np.zeros(0), 1, 2), *cons([(0, 0, ML), (0, 0, CL)]))
    assert r.num_sat.tolist() == [2] and r.labels.tolist() == [0] and r.satisfied_fraction == 0.0


def test_parse_constraints(pkg):
    ca, cb, ct = pkg.parse_constraints("0,3,ml\n12,7,cl\n5,5,cl\n")
    assert ca.tolist() == [0, 12, 5] and cb.tolist() == [3, 7, 5] and ct.tolist() == [ML, CL, CL]
    assert ca.dtype == cb.dtype == ct.dtype == np.int32
    assert [x.tolist() for x in pkg.parse_constraints("1,2,ml")] == [[1], [2], [ML]]  # no trailing newline
    assert [x.shape for x in pkg.parse_constraints("")] == [(0,)] * 3
    assert [x.tolist() for x in pkg.parse_constraints(b"1,2,cl\r\n3,4,ml\r\n")] == [[1, 3], [2, 4], [CL, ML]]
    for text, line in [("0,1,ml\n0,1,xx\n", 2), ("0,1\n", 1), ("0,1,ml\n\n2,3,cl\n", 2), ("a,1,ml", 1), ("0,-1,cl", 1),
                       ("0,1,ml,9", 1), ("0, 1,ml", 1), ("0,1,ML", 1), ("1,2,ml\n3,4,cl\n4294967296,1,ml\n", 3), ("1.0,2,ml", 1)]:
        with pytest.raises(ValueError, match=f"line {line}"):
            pkg.parse_constraints(text)


def test_cluster_tree_text_with_constraint_columns(pkg):
    t, _ = hand_tree(pkg, "A")
    off = np.array([0, 20, 20, 40, 40])
    assert pkg.format_cluster_tree(t, off) == K_TEXT  # the default is unchanged
    r = pkg.constrained_flat_labels(t, *cons(HAND[0][1]))  # num_sat 6 3 3 0 1, prop_sat 6 0 1 0 0, m = 5
    want = ("1,NaN,5.0,NaN,0.6,0.6,0,0\n2,5.0,1.0,1.9000000000000001,0.3,0.0,20,1\n3,5.0,3.0,0.6666666666666665,0.3,0.1,20,1\n"
            "4,3.0,1.0,2.0,0.0,0.0,40,3\n5,3.0,0.5,3.3333333333333335,0.1,0.0,40,3\n")
    assert pkg.format_cluster_tree(t, off, constrained=r) == want
    e = np.zeros(0, np.int32)
    none = pkg.format_cluster_tree(t, off, constrained=pkg.constrained_flat_labels(t, e, e, e))  # 0.0 / 0
    assert none == K_TEXT.replace(",0,0,", ",NaN,NaN,")
