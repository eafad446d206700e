"""The membership half of soft clustering on the host over deep, wide and forest-shaped cluster
trees (tests/soft_trees.py): the inputs hold what they claim, and the host path of
hdb_membership_vectors (csrc/soft.cpp, ctx = NULL, no device) equals the restatement
(tests/soft_reference.py) on them -- which is what lets test_gpu_soft_trees.py take the host path as
its reference where the Python walk over every row is too slow.  hdb_exemplars on the host against
the restatement over the trees of tests/hierarchy_weights.py.  Every comparison is on bits; the
restatement has no NaN for any of these inputs, and no row is left out of a comparison."""
import numpy as np
import pytest

import hierarchy_weights as H
import soft_trees as T
from soft_reference import exemplars_ref, membership_ref
from test_outlier_scores import bits

INF = float("inf")


def same_rows(r, want, rows, where):
    vec, prob, lab = want
    assert not np.isnan(vec).any() and not np.isnan(prob).any(), where
    assert np.array_equal(bits(r.vectors[rows]), bits(vec)), where
    assert np.array_equal(bits(r.prob[rows]), bits(prob)), where
    assert r.labels.dtype == np.int32 and np.array_equal(r.labels[rows], lab), where


# ------------------------------------------------------------- the inputs do what they are for
DEPTH = {"comb-40": 41, "comb-600": 601, "star-299": 2, "forest": 17}
DEPTH.update({"chain-%d" % K: K for K in T.CHAINS})
DEPTH.update({"binary-%d" % h: h for h in (1, 2, 3, 4, 5, 6, 11)})
SIZE = {"comb-40": 81, "comb-600": 1201, "star-299": 300, "forest": 64, "random-500-1": 500, "random-500-2": 500,
        "binary-11": 2047}
ROWS = {1: 1, 2: 1, 3: 2, 4: 2, 5: 3, 8: 3, 9: 4, 16: 4, 17: 5, 64: 6, 65: 7, 1024: 10, 1025: 11}  # chain K -> J


@pytest.mark.parametrize("name", list(T.SHAPES))
def test_shapes_hold_what_they_claim(name):
    parent, birth, death, depth = T.shape(name)
    K = parent.shape[0]
    assert K == SIZE.get(name, K) and parent[0] == 0
    assert all(0 <= parent[i] <= i for i in range(K))  # the contract's parent labels
    if name in DEPTH:
        assert depth.max() == DEPTH[name]
    assert depth.max() <= K <= 2 ** T.table_rows(K)
    if name.startswith("chain"):
        assert T.table_rows(K) == ROWS[K]
        if K in (2, 4, 8, 16, 64, 1024):  # the longest lift, K - 1 steps, sets every bit
            assert K - 1 == 2 ** T.table_rows(K) - 1
    if name.startswith("random"):
        assert depth.max() > 8
    roots = np.flatnonzero(parent == 0) + 1
    assert (roots.shape[0] == 6 and np.all(roots[1:] > 1)) if name == "forest" else roots.shape[0] == 1
    # births: NaN for every root, finite and positive elsewhere, one level per parent, falling with the depth
    assert np.isnan(birth[roots - 1]).all() and np.isnan(birth).sum() == roots.shape[0]
    rest = np.flatnonzero(parent > 0)
    assert np.all(np.isfinite(birth[rest])) and np.all(birth[rest] > 0)
    for i in rest:
        p = parent[i]
        sib = np.flatnonzero(parent == p)
        assert np.all(birth[sib] == birth[i])
        assert parent[p - 1] == 0 or birth[i] < birth[p - 1]
    assert np.all(np.isfinite(death)) and np.all(death > 0) and np.all(death[rest] <= birth[rest])


def test_selections_hold_what_they_claim():
    for name, kind, _ in T.CASES:
        parent, _, _, depth = T.shape(name)
        K = parent.shape[0]
        flat, C, wit = T.selection(name, kind)
        assert flat.shape[0] == K and flat.min() >= 0 and flat.max() <= C
        if kind == "all":
            assert C == K <= 65 and np.array_equal(flat, np.arange(1, K + 1))
        if kind == "sampled":
            assert C == 48 and np.array_equal(np.sort(flat[flat > 0]), np.arange(1, 49))
            assert flat[0] > 0 and flat[1] > 0 and flat[K - 1] > 0 and flat[np.argmax(depth) - 1] > 0
            picked = np.flatnonzero(flat) + 1  # one selected cluster under another
            assert any(T.related(parent, int(a), int(b)) for a in picked[:5] for b in picked[5:])
        if kind == "multi":
            f, a, b = wit["nested"]  # one label on two clusters, one an ancestor of the other
            assert flat[a - 1] == flat[b - 1] == f and a != b and a in T.ancestors(parent, b)
            f, a, b = wit["pair"]
            assert flat[a - 1] == flat[b - 1] == f and a != b
            assert name.startswith("chain") or not T.related(parent, a, b)
            three = wit["three"][1:]
            assert len(three) == 3 and (flat == 4).sum() == 3 and (flat == 1).sum() == 2 and (flat == 2).sum() == 2
            assert any(x in T.ancestors(parent, y) for x in three for y in three if x != y)
            assert not (flat == 3).any() and C == 5  # a label in the middle that no cluster carries
    # the forest: anchors and selected clusters in different trees
    parent = T.shape("forest")[0]
    flat = T.selection("forest", "sampled")[0]
    tops = {T.ancestors(parent, int(c))[-1] for c in np.flatnonzero(flat) + 1}
    assert len(tops) >= 4


@pytest.mark.parametrize("name", ["chain-9", "binary-4", "forest", "comb-40"])
def test_queries_hold_what_they_claim(name):
    parent, birth, death, depth = T.shape(name)
    K = parent.shape[0]
    anchor, level, dmin = T.queries(name, 5)
    m = anchor.shape[0]
    assert m == 4 * (K + 1) + 3 and dmin.shape == (m, 5)
    assert np.array_equal(anchor[:4 * (K + 1)], np.repeat(np.arange(K + 1), 4))  # every anchor, 0 included
    assert not np.isnan(level).any() and np.all(level >= 0)
    for a in range(1, K + 1):
        four = level[4 * a:4 * a + 4]
        assert 0.0 in four and INF in four
        if parent[a - 1] > 0:
            assert four[0] == birth[a - 1]  # the birth of its siblings: M == B
            if parent[parent[a - 1] - 1] > 0:
                assert birth[a - 1] < four[3] < birth[parent[a - 1] - 1]
    assert np.isin(dmin, T.PALETTE).all() and all((dmin == v).any() for v in T.PALETTE)
    assert np.signbit(dmin[dmin == 0]).any() and not np.signbit(dmin[dmin == 0]).all()
    assert (dmin > 0).all(1).sum() > m // 2  # rows without a zero: the sum branch
    assert np.all(dmin[m - 3] == INF) and np.isfinite(dmin[m - 1]).sum() == 1
    assert (dmin[m - 2] == 0).sum() >= 2 and np.signbit(dmin[m - 2, 0]) and not np.signbit(dmin[m - 2, -1])
    assert np.all(anchor[m - 3:] == np.argmax(depth))


def test_a_root_without_children_is_asked_at_zero_and_infinity():
    """eps_max of such a root is Double.MAX_VALUE: a finite positive level overflows the tree part"""
    anchor, level, _ = T.queries("chain-1", 1)
    assert np.array_equal(anchor, [0, 0, 0, 0, 1, 1, 1, 1, 1, 1, 1]) and np.isin(level[4:], [0.0, INF]).all()


# ------------------------------------------------------------------- host against restatement
@pytest.mark.parametrize("case", T.CASES, ids=T.CASE_IDS)
def test_host_membership_equals_the_restatement(pkg, case):
    """every row where the case's reference is the restatement (all pairs of the tree for K <= 65);
    the "host" cases: the host path runs every row, the Python walk a fixed sample of them"""
    tree, flat, C, anchor, level, dmin = T.case_inputs(pkg, case)
    r = pkg.membership_rows(tree, anchor, level, dmin, flat)
    rows = np.arange(anchor.shape[0]) if case[2] == "restatement" else T.sample_rows(anchor.shape[0])
    assert case[2] == "restatement" or rows[-1] == anchor.shape[0] - 1
    same_rows(r, membership_ref(tree, anchor[rows], level[rows], dmin[rows], flat), rows, case)
    assert not np.isnan(r.vectors).any() and not np.isnan(r.prob).any()
    assert np.all(r.prob >= 0) and np.all(r.prob <= 1)
    assert np.all(r.vectors[anchor == 0] == 0) and np.all(r.prob[anchor == 0] == 0) and np.all(r.labels[anchor == 0] == 0)
    assert tree.n_tree == 1 or len(set(r.labels.tolist())) > min(C, 5) // 2  # the rows are not all alike


def test_a_count_above_every_carried_label(pkg):
    """C = 8 with labels 1, 2, 4, 5 carried: empty clusters in the middle and at the end.  The C ABI
    directly: the wrapper takes C from the largest label"""
    A = pkg._capi
    parent, birth, death, _ = T.shape("forest")
    flat = T.selection("forest", "multi")[0]
    C = 8
    anchor, level, dmin = T.queries("forest", C)
    m = anchor.shape[0]
    vec, prob, lab = np.full((m, C), 7.0), np.full(m, 7.0), np.full(m, 7, np.int32)
    rc = pkg.lib().hdb_membership_vectors(None, A.ptr(parent), A.ptr(birth), A.ptr(death), A.ptr(flat), parent.shape[0], C,
                                          A.ptr(anchor), A.ptr(level), A.ptr(dmin), m, A.ptr(vec), A.ptr(prob), A.ptr(lab))
    assert rc == 0
    want = membership_ref(T.make_tree(pkg, "forest", flat, C), anchor, level, dmin, flat, C)
    assert not np.isnan(want[0]).any()
    assert np.array_equal(bits(vec), bits(want[0])) and np.array_equal(bits(prob), bits(want[1]))
    assert np.array_equal(lab, want[2])
    assert np.all(vec[:, [2, 5, 6, 7]] == 0) and (vec[:, [0, 1, 3, 4]] > 0).any(0).all()


# ------------------------------------------------------------- exemplars on the weight families
# the trees test_gpu_soft_trees.py runs: every family at n = 300 under both minClSize values, the deep
# tiny_normal tree, the shapes and the cosine and Pearson MSTs
WEIGHT_TREES = [((f, 300), mcs) for f in H.FAMILIES for mcs in H.MCS]
WEIGHT_TREES += [(("tiny_normal", 1500), 2), (("wide", None), 2), (("caterpillar", None), 2)]
WEIGHT_TREES += [((metric, None), mcs) for metric in H.MSTS for mcs in H.MCS]
WEIGHT_IDS = ["%s-mcs%d" % (H.case_id(c), m) for c, m in WEIGHT_TREES]


def weight_tree(pkg, case, mcs):
    """the host tree, which test_hierarchy_weights.py pins to the top-down reference"""
    va, vb, w, n = H.tree_case(case)
    return pkg.cluster_tree(va, vb, w, n, mcs)


@pytest.mark.parametrize("case,mcs", WEIGHT_TREES, ids=WEIGHT_IDS)
def test_host_exemplars_on_the_weight_families(pkg, case, mcs):
    t = weight_tree(pkg, case, mcs)
    ids, off = pkg.exemplars(t)
    want = exemplars_ref(t)
    assert ids.dtype == np.int32 and off.dtype == np.int64
    assert np.array_equal(ids, want[0]) and np.array_equal(off, want[1]), (case, mcs)
    assert off.shape[0] == t.n_clusters + 1
    pl = t.point_level
    if case[0] == "all_inf":
        assert t.n_tree == 1 and t.n_clusters == 0 and ids.shape[0] == 0 and np.all(pl == INF)
    if case[0] in ("inf_tenth", "extremes"):
        assert np.isposinf(pl).any()
    if case[0] in H.SIGNED_ZERO + ("inf_tenth", "tiny_mixed_zero", "caterpillar", "wide"):
        assert (pl == 0).any()
        # a tree stores +0.0; with some of the zeros flipped to -0.0 the exemplars are the same points
        zero = np.flatnonzero(pl == 0)
        t.point_level = pl.copy()
        t.point_level[zero[::2]] = -0.0
        got = pkg.exemplars(t)
        assert np.array_equal(got[0], ids) and np.array_equal(got[1], off)
        again = exemplars_ref(t)
        assert np.array_equal(again[0], ids) and np.array_equal(again[1], off)
