"""The hierarchy on the host (csrc/flat.cpp, csrc/constraints.cpp; ctx = NULL) over negative,
signed-zero, subnormal and infinite edge weights -- what the exact cosine and Pearson MSTs and
non-finite rows hand it -- against the test-side references, on every weight family and tree shape
of tests/hierarchy_weights.py: the tree's arrays, flat labels (also oracle/flat_labels.py), GLOSH
scores and noise levels, constrained labels, level cuts and predict_labels.

Doubles compare bit for bit, except that a NaN compares as a NaN (path_helpers.bits_eq): inf - inf
has no defined sign or payload.  "-0.0 and 0.0 are one level": the signed-zero families fail on a
host that takes a tie group's level from its first edge as it is."""
import numpy as np
import pytest

import hierarchy_weights as H
from path_helpers import bits_eq
from predict_ref import predict_ref

INTS = ("parent", "size", "min_id", "flat_label", "point_cluster")
DOUBLES = ("birth", "death", "stability", "point_level")
CASE_MCS = [(c, mcs) for c in H.CASES for mcs in H.case_mcs(c)]
IDS = ["%s-mcs%d" % (H.case_id(c), m) for c, m in CASE_MCS]


def same_tree(t, ref, where=None):
    """test_cluster_tree.same_tree with a NaN as a class"""
    for k in INTS:
        assert np.array_equal(np.asarray(getattr(t, k)), np.asarray(getattr(ref, k))), (k, where)
    for k in DOUBLES:
        assert bits_eq(getattr(t, k), getattr(ref, k)), (k, where, getattr(t, k), getattr(ref, k))
    assert t.n_clusters == ref.n_clusters, where


def same_constrained(got, want, where=None):
    for k in ("num_sat", "prop_sat", "flat_label", "labels"):
        assert np.array_equal(np.asarray(getattr(got, k)), np.asarray(getattr(want, k))), (k, where)
    assert bits_eq(got.prop_stability, want.prop_stability), (where, got.prop_stability)
    assert got.n_clusters == want.n_clusters, where


def same_prediction(got, want, where=None):
    for g, w, k in zip(got, want, ("tree_label", "labels", "scores")):
        if k == "scores":
            assert bits_eq(g, w), (k, where)
        else:
            assert np.asarray(g).dtype == np.int32 and np.array_equal(g, w), (k, where)


# ------------------------------------------------------------- the inputs do what they are for
@pytest.fixture(scope="module")
def stats():
    """family or shape -> summed tree_stats of its reference trees"""
    out = {}
    for case, mcs in CASE_MCS:
        s = H.tree_stats(H.ref_tree(case, mcs))
        acc = out.setdefault(case[0], dict.fromkeys(s, 0))
        for k, v in s.items():
            acc[k] = max(acc[k], v) if k in ("depth", "widest") else acc[k] + v
    return out


def test_families_hold_what_they_claim(stats):
    for name, s in stats.items():
        print(name, s)
    for name in ("tiny_normal", "tiny_mixed", "tiny_mixed_zero", "extremes", "signed_zero_first", "signed_zero_last",
                 "caterpillar", "wide", "cosine", "pearson"):
        assert stats[name]["negative"] > 0, name
    for name in ("extremes", "caterpillar"):
        assert stats[name]["nan"] > 0, name
    for name in ("inf_tenth", "extremes"):  # all_inf is one tie group: the root alone
        assert stats[name]["inf_birth"] > 0, name
    assert stats["caterpillar"]["depth"] >= 200 and stats["wide"]["widest"] > H.FO_CHUNK
    for name in ("caterpillar", "wide", "tiny_normal", "extremes"):  # the general FOSC walk on a wave's path
        assert stats[name]["general"], name
    # the walker's fast path, its general path inside a chunk of non-negative values, and both in one chunk
    assert min(stats["caterpillar"][k] for k in ("fast", "guarded", "both")) > 0


def test_tiny_normal_1500_has_hundreds_of_negative_stabilities():
    assert H.tree_stats(H.ref_tree(("tiny_normal", 1500), 2))["negative"] >= 100


def test_weights_hold_what_they_claim():
    for name in H.FAMILIES:
        w = np.concatenate([H.tree_case((name, n))[2] for n in H.SIZES])
        if name in ("tiny_normal", "tiny_mixed", "tiny_mixed_zero", "extremes", "all_negative") + H.SIGNED_ZERO:
            assert (w < 0).any(), name
        if name == "all_negative":
            assert (w < 0).all() and np.unique(w).shape[0] <= 4
        if name in ("inf_tenth", "all_inf", "extremes"):
            assert np.isposinf(w).any(), name
        if name == "extremes":
            assert (np.abs(w[w != 0]) < 2.3e-308).any()  # subnormals
    for name, lead in zip(H.SIGNED_ZERO, (True, False)):
        for n in H.SIZES:
            w = H.tree_case((name, n))[2]
            zero = np.flatnonzero(w == 0.0)
            assert zero.shape[0] > 0 and bool(np.signbit(w[zero[0]])) == lead, (name, n)
        w = H.tree_case((name, 1500))[2]
        assert np.signbit(w[w == 0.0]).any() and not np.signbit(w[w == 0.0]).all()  # both zeros in one tie group
    for metric in H.MSTS:
        w = H.real_mst(metric)[4]
        print(metric, "MST:", int((w < 0).sum()), "of", w.shape[0], "weights negative")
        assert (w < 0).sum() > 100, metric
    va, vb, w, n = H.caterpillar()
    assert (w == 0.0).any() and (w < 0).any() and np.isin(w, [1e-310, 5e-324]).any()
    runs = [c for arm in H.ARMS for k, c in arm if k != "tie3"]
    assert min(runs) < 8 and max(runs) > 64 and all(c < 8 or c > 64 for c in runs)


# ------------------------------------------------------------------------ host against reference
@pytest.mark.parametrize("case,mcs", CASE_MCS, ids=IDS)
def test_tree_labels_and_scores_equal_the_references(pkg, case, mcs):
    va, vb, w, n = H.tree_case(case)
    ref = H.ref_tree(case, mcs)
    t = pkg.cluster_tree(va, vb, w, n, mcs)
    same_tree(t, ref, (case, mcs))
    assert not np.signbit(t.birth[t.birth == 0]).any() and not np.signbit(t.point_level[t.point_level == 0]).any()
    labels, k = pkg.flat_labels(va, vb, w, n, mcs)
    assert k == ref.n_clusters and np.array_equal(labels, ref.flat), (case, mcs)
    assert np.array_equal(t.flat_labels(), labels)
    s, e, lab2, k2 = pkg.outlier_scores(va, vb, w, n, mcs, with_labels=True)
    rs, re = H.ref_glosh(case, mcs)
    assert bits_eq(e, re) and bits_eq(s, rs), (case, mcs)
    assert k2 == k and np.array_equal(lab2, labels)
    assert bits_eq(e, t.point_level)


@pytest.mark.parametrize("case,mcs", [cm for cm in CASE_MCS if (cm[0][1] or 0) <= 300 or cm[0][0] in H.SIGNED_ZERO],
                         ids=lambda x: H.case_id(x) if isinstance(x, tuple) else str(x))
def test_flat_labels_equal_the_oracle(pkg, case, mcs):
    """oracle/flat_labels.py: the top-down restatement the device tests compare with"""
    from oracle.flat_labels import flat_labels
    va, vb, w, n = H.tree_case(case)
    want, kw = flat_labels(n, va, vb, w, mcs)
    got, kg = pkg.flat_labels(va, vb, w, n, mcs)
    assert kg == kw and np.array_equal(got, want), (case, mcs)
    assert np.array_equal(want, H.ref_tree(case, mcs).flat)


@pytest.mark.parametrize("case,mcs", CASE_MCS, ids=IDS)
def test_constrained_labels_equal_the_reference(pkg, case, mcs):
    va, vb, w, n = H.tree_case(case)
    t = pkg.cluster_tree(va, vb, w, n, mcs)
    got = pkg.constrained_flat_labels(t, *H.constraints_of(case, mcs))
    same_constrained(got, H.ref_constrained(case, mcs), (case, mcs))


@pytest.mark.parametrize("case,mcs", CASE_MCS, ids=IDS)
def test_cuts_and_predictions_equal_the_references(pkg, case, mcs):
    va, vb, w, n = H.tree_case(case)
    ref = H.ref_tree(case, mcs)
    t = pkg.cluster_tree(va, vb, w, n, mcs)
    levels = H.case_levels(case)
    rows = pkg.labels_at_levels(t, levels)
    assert np.array_equal(rows, H.ref_cuts(ref, levels)), (case, mcs)
    for e in (0.0, -1e-17, float(levels[0])):  # the bisection is RefTree.cut
        assert np.array_equal(H.ref_cuts(ref, [e])[0], ref.cut(e))
    assert np.array_equal(rows[levels == 0.0][0], rows[levels == 0.0][1])  # +0.0 and -0.0 cut alike
    nearest, level = H.queries_of(case, mcs)
    same_prediction(pkg.predict_labels(t, nearest, level), predict_ref(ref, nearest, level), (case, mcs))
    y = np.arange(n, dtype=np.int32)  # identity: a point attached to itself at its own level
    tl, lab, sc = pkg.predict_labels(t, y, t.point_level)
    assert np.array_equal(tl, t.point_cluster) and np.array_equal(lab, ref.flat)
    assert bits_eq(sc, H.ref_glosh(case, mcs)[0])


def test_issue_vector_signed_zero_leading_a_tie_group(pkg):
    """n = 9, minClSize 2: the -0.0 edge has the lowest index of its tie group"""
    va = np.array([2, 7, 7, 7, 2, 8, 8, 2], np.int32)
    vb = np.array([7, 8, 3, 6, 1, 0, 5, 4], np.int32)
    w = np.array([1, .5, .5, -2e-16, -0.0, 1e-16, 0.0, 1e-16])
    t = pkg.cluster_tree(va, vb, w, 9, 2)
    assert bits_eq(t.stability[:4], [np.nan, 6.0, np.inf, np.inf])  # not -inf: 1 / eps and 1 / birth at +0.0
    assert -1.1e16 < t.stability[4] < -0.9e16
    same_tree(t, H.cluster_tree_reference(va, vb, w, 9, 2))
    swapped = np.where(w == 0, -w, w)  # the other zero leads: the same tree
    same_tree(pkg.cluster_tree(va, vb, swapped, 9, 2), t)
    assert pkg.flat_labels(va, vb, w, 9, 2)[1] == 3
