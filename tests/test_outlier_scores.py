"""GLOSH outlier scores over the merged MST, host path (csrc/flat.cpp, ctx = NULL).

The host algorithm (bottom-up dendrogram, one top-down condensation) must equal the test-side
reference (tests/glosh_reference.py: the plain top-down restatement, tie groups removed in
descending level and split by BFS) bit for bit -- the arithmetic is one exact min, one division
and one subtraction per point -- and the hand-checked vectors, the never-split-root value
(1 - DBL_MAX / eps) included.  Ranking and the output file are host formatting."""
import ctypes as C
import functools
import sys

import numpy as np
import pytest

from conftest import load_iris
from glosh_reference import glosh_reference

DBL_MAX = sys.float_info.max

# (edges (a, b, w), n, minClSize, eps, scores): hand-checked
KNOWN = [
    ([(0, 1, 1), (1, 2, 2), (3, 4, 1.5), (2, 3, 5), (4, 5, 4)], 6, 2,
     [1, 1, 2, 1.5, 1.5, 4], [0, 0, 0.5, 0, 0, 0.625]),
    ([(0, 1, 1), (1, 2, 1), (2, 3, 6), (3, 4, 2), (4, 5, 2), (5, 6, 9)], 7, 2,
     [1, 1, 1, 2, 2, 2, 9], [0, 0, 0, 0, 0, 0, 1 - 1.0 / 9.0]),          # the root takes its descendants only
    ([(0, 1, 0.5), (1, 2, 2), (2, 3, 3)], 4, 3,
     [2, 2, 2, 3], [1 - DBL_MAX / 2] * 3 + [1 - DBL_MAX / 3]),            # the root never splits
    ([(0, 1, 0), (1, 2, 0), (2, 3, 3), (3, 4, 0)], 5, 2, [0] * 5, [0] * 5),  # duplicate points
]


def edges_of(case):
    e = case[0]
    return (np.array([x[0] for x in e], np.int32), np.array([x[1] for x in e], np.int32),
            np.array([x[2] for x in e], np.float64))


def bits(x):
    return np.ascontiguousarray(np.asarray(x, np.float64)).view(np.uint64)


def random_tree(rng, n, ties):
    """random recursive tree under a random relabelling; ties: weights from a few small integers
    (heavy ties, zero weights), else continuous"""
    va = np.array([int(rng.integers(0, i)) for i in range(1, n)], np.int64)
    vb = np.arange(1, n, dtype=np.int64)
    w = rng.integers(0, 6, n - 1).astype(np.float64) if ties else rng.random(n - 1)
    perm = rng.permutation(n)
    return perm[va].astype(np.int32), perm[vb].astype(np.int32), w


@pytest.mark.parametrize("case", range(len(KNOWN)))
def test_known_answers_bit_exact(pkg, case):
    _, n, mcs, eps, scores = KNOWN[case]
    va, vb, w = edges_of(KNOWN[case])
    s, e = pkg.outlier_scores(va, vb, w, n, mcs)
    assert np.array_equal(bits(e), bits(eps)), e
    assert np.array_equal(bits(s), bits(scores)), s
    rs, re = glosh_reference(va, vb, w, n, mcs)  # the reference agrees with the hand check too
    assert np.array_equal(bits(re), bits(eps)) and np.array_equal(bits(rs), bits(scores))


def test_negative_zero_weights_are_level_zero(pkg):
    """-0.0 == 0.0 is one level; the noise level comes back as +0.0"""
    va, vb, w = edges_of(KNOWN[3])
    s, e = pkg.outlier_scores(va, vb, np.where(w == 0, -0.0, w), 5, 2)
    assert np.array_equal(bits(e), bits(np.zeros(5))) and np.array_equal(bits(s), bits(np.zeros(5)))


def test_host_equals_reference_on_random_trees(pkg):
    rng = np.random.default_rng(20240611)
    never_split = small = 0
    for t in range(240):
        n = int(rng.integers(1, 301)) if t % 12 else int(rng.integers(1, 8))
        mcs = int(rng.integers(2, 9))
        va, vb, w = random_tree(rng, n, ties=t % 2 == 1)
        s, e = pkg.outlier_scores(va, vb, w, n, mcs)
        rs, re = glosh_reference(va, vb, w, n, mcs)
        assert np.array_equal(bits(e), bits(re)), (t, n, mcs)
        assert np.array_equal(bits(s), bits(rs)), (t, n, mcs)
        never_split += bool((s < -1e300).any())
        small += n < mcs
    assert never_split >= 10 and small >= 5  # both corners were exercised


def test_host_equals_reference_on_iris_mst(pkg, oracle):
    X = load_iris()
    core = oracle.core_distances(X, 4, semantics=oracle.EXCL_SELF)
    for self_edges in (False, True):  # the self edges are ignored
        va, vb, w = oracle.prim_mst(X, core, self_edges=self_edges)
        for mcs in (2, 4, 10):
            s, e = pkg.outlier_scores(va, vb, w, X.shape[0], mcs)
            rs, re = glosh_reference(va, vb, w, X.shape[0], mcs)
            assert np.array_equal(bits(e), bits(re)) and np.array_equal(bits(s), bits(rs)), (self_edges, mcs)


def test_combined_call_gives_flat_labels(pkg):
    rng = np.random.default_rng(5)
    for t in range(30):
        n = int(rng.integers(1, 400))
        mcs = int(rng.integers(2, 9))
        va, vb, w = random_tree(rng, n, ties=t % 2 == 1)
        s, e, lab, k = pkg.outlier_scores(va, vb, w, n, mcs, with_labels=True)
        ref, kr = pkg.flat_labels(va, vb, w, n, mcs)
        s2, e2 = pkg.outlier_scores(va, vb, w, n, mcs)
        assert k == kr and np.array_equal(lab, ref)
        assert np.array_equal(bits(s), bits(s2)) and np.array_equal(bits(e), bits(e2))
    s, e, lab, k = pkg.outlier_scores(np.zeros(0, np.int32), np.zeros(0, np.int32), np.zeros(0), 1, 4, with_labels=True)
    assert s.tolist() == [0.0] and e.tolist() == [0.0] and lab.tolist() == [0] and k == 0
    s, e = pkg.outlier_scores(np.zeros(0, np.int32), np.zeros(0, np.int32), np.zeros(0), 0, 4)
    assert s.shape == (0,) and e.shape == (0,)


def test_error_statuses_equal_flat_labels(pkg):
    """each malformed input gives hdb_flat_labels's status, through the C-ABI with ctx = NULL"""
    rng = np.random.default_rng(9)
    n = 40
    va, vb, w = random_tree(rng, n, ties=False)
    bad = {
        "not spanning": (va[:-1], vb[:-1], w[:-1], n, 4),
        "cycle": (np.r_[va[:-1], va[0]].astype(np.int32), np.r_[vb[:-1], vb[0]].astype(np.int32), w, n, 4),
        "nan": (va, vb, np.where(np.arange(n - 1) == 7, np.nan, w), n, 4),
        "range": (np.where(np.arange(n - 1) == 3, n + 5, va).astype(np.int32), vb, w, n, 4),
        "negative id": (np.where(np.arange(n - 1) == 3, -1, va).astype(np.int32), vb, w, n, 4),
        "minClSize": (va, vb, w, n, 1),
    }
    L = pkg.lib()
    p = lambda a: C.c_void_p(a.ctypes.data)
    for name, (a, b, ww, nn, mcs) in bad.items():
        a, b, ww = np.ascontiguousarray(a, np.int32), np.ascontiguousarray(b, np.int32), np.ascontiguousarray(ww, np.float64)
        lab, s, e, k = np.zeros(nn, np.int32), np.zeros(nn), np.zeros(nn), np.zeros(1, np.int64)
        r_lab = L.hdb_flat_labels(None, p(a), p(b), p(ww), ww.shape[0], nn, mcs, p(lab), p(k))
        r_out = L.hdb_flat_outlier_scores(None, p(a), p(b), p(ww), ww.shape[0], nn, mcs, p(s), p(e), p(lab), p(k))
        assert r_lab != 0 and r_out == r_lab, (name, r_lab, r_out)
        with pytest.raises(pkg.HdbError):
            pkg.outlier_scores(a, b, ww, nn, mcs)
    # a required output missing is an argument error; the optional ones may be NULL
    a, b, ww = va, vb, np.ascontiguousarray(w)
    s = np.zeros(n)
    assert L.hdb_flat_outlier_scores(None, p(a), p(b), p(ww), n - 1, n, 4, None, None, None, None) == -1
    assert L.hdb_flat_outlier_scores(None, p(a), p(b), p(ww), n - 1, n, 4, p(s), None, None, None) == 0
    assert np.array_equal(bits(s), bits(pkg.outlier_scores(va, vb, w, n, 4)[0]))


def test_outlier_ranking_is_compare_to_order(pkg):
    """ascending (score, core distance, id) with > / < comparisons (OutlierScore.compareTo):
    ties in score, equal cores, and -0.0 == 0.0"""
    scores = np.array([0.5, 0.0, -0.0, 0.5, 0.25, 0.0, -1e308, 0.5, -np.inf, 0.0])
    core = np.array([1.0, 2.0, 2.0, 1.0, 9.0, 1.0, 0.0, 0.5, 3.0, 2.0])

    def compare(i, j):
        for x, y in ((scores[i], scores[j]), (core[i], core[j]), (i, j)):
            if x > y:
                return 1
            if x < y:
                return -1
        return 0

    want = sorted(range(len(scores)), key=functools.cmp_to_key(compare))
    got = pkg.outlier_ranking(scores, core)
    assert got.tolist() == want
    assert want[:2] == [8, 6] and want.index(2) < want.index(9)  # -0.0 ties 0.0: the id decides
    rng = np.random.default_rng(2)
    scores = rng.integers(0, 4, 500) / 4.0
    core = rng.integers(0, 3, 500).astype(np.float64)
    want = sorted(range(500), key=lambda i: (scores[i], core[i], i))
    assert pkg.outlier_ranking(scores, core).tolist() == want


def test_format_outlier_scores_case_1(pkg):
    _, n, mcs, _, _ = KNOWN[0]
    va, vb, w = edges_of(KNOWN[0])
    s, _ = pkg.outlier_scores(va, vb, w, n, mcs)
    core = np.array([1.0, 1.0, 2.0, 1.5, 1.5, 4.0])
    p = pkg.outlier_ranking(s, core)
    text = pkg.format_outlier_scores(s[p], p)
    assert text == "0.0,0\n0.0,1\n0.0,3\n0.0,4\n0.5,2\n0.625,5\n"
    va, vb, w = edges_of(KNOWN[2])  # Double.toString of the never-split-root scores
    s, _ = pkg.outlier_scores(va, vb, w, 4, 3)
    assert pkg.format_outlier_scores(s[3:], [3]) == "-5.992310449541053E307,3\n"
