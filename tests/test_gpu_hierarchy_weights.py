"""Everything downstream of the MST on the device over negative, signed-zero, subnormal and
infinite edge weights (tests/hierarchy_weights.py): the merge order (csrc/merge.hip), K6 and its
exports (csrc/flat.hip: flat labels, GLOSH, the cluster tree, level cuts, predict_labels), the
constrained extraction (csrc/constraints.hip) -- against the test-side references and the host path,
which test_hierarchy_weights.py pins on the same inputs -- and K2g's cosine and Pearson trees end
to end through the hierarchy and approximate_predict.

Doubles compare bit for bit; a NaN compares as a NaN (path_helpers.bits_eq).  Every hierarchy test
prints whether its tree takes the FOSC walker's general path (fo_walk: a negative, -0.0 or NaN value
on a path a wave walks), decided from the host tree (hierarchy_weights.tree_stats)."""
import numpy as np
import pytest
import torch

import hierarchy_weights as H
from path_helpers import bits_eq, edge_set, options
from predict_ref import attach_ref, predict_ref
from test_gpu_flat import orders
from test_hierarchy_weights import CASE_MCS, IDS, same_constrained, same_prediction, same_tree

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ctx(pkg):
    c = pkg.Context(0)
    c.use_torch_stream()  # the attach scan and K2g are stream-ordered: results are read on torch's stream
    return c


def cuda(x, dt):
    return torch.from_numpy(np.array(x, dtype=dt, order="C")).cuda()


def host(x):
    return x.cpu().numpy() if torch.is_tensor(x) else np.asarray(x)


def dev_edges(va, vb, w):
    return cuda(va, np.int32), cuda(vb, np.int32), cuda(w, np.float64)


def report(where, tree):
    s = H.tree_stats(tree)
    print("%s: general fo_walk path %s (%d negative, %d NaN stabilities, depth %d, widest %d; segments of clean chunks: "
          "%d fast, %d general, %d chunks with both)" % (where, "reached" if s["general"] else "not reached", s["negative"],
                                                       s["nan"], s["depth"], s["widest"], s["fast"], s["guarded"], s["both"]))
    return s


class HostConstrained:
    def __init__(self, r):
        for k in ("num_sat", "prop_sat", "prop_stability", "flat_label", "labels"):
            setattr(self, k, host(getattr(r, k)))
        self.n_clusters = r.n_clusters


# ------------------------------------------------------------------------- sorting and merging
def run_sizes(E, runs, rng):
    """`runs` lengths summing to E, a run of length 0 and one of length 1 among three or more"""
    if runs == 1:
        return [E]
    cut = np.sort(rng.integers(0, E - 1, runs - 3))
    return [0, 1] + np.diff(np.r_[0, cut, E - 1]).tolist()


@pytest.mark.parametrize("E", [1000, 70000])
@pytest.mark.parametrize("family", list(H.FAMILIES))
def test_sort_and_merge_order(pkg, ctx, family, E):
    """sort_edges_desc (sample sort and radix sort) and merge_sorted_runs: the stable descending
    order, -0.0 and +0.0 one key -- they keep their input order and come back with their signs"""
    rng = np.random.default_rng(E + sorted(H.FAMILIES).index(family))
    w = np.ascontiguousarray(H.FAMILIES[family](rng, E), np.float64)
    a, b = np.arange(E, dtype=np.int32), rng.integers(0, 1 << 30, E).astype(np.int32)
    want = np.argsort(-(w + 0.0), kind="stable")
    for ssort in (1, 0):
        with options(ctx, ssort=ssort):
            ga, gb, gw = (host(x) for x in pkg.sort_edges_desc(*dev_edges(a, b, w), ctx))
        assert np.array_equal(ga, a[want]) and np.array_equal(gb, b[want]), (family, E, ssort)
        assert bits_eq(gw, w[want]) and np.array_equal(np.signbit(gw), np.signbit(w[want])), (family, E, ssort)
    for runs in (1, 3, 8):
        sizes = run_sizes(E, runs, rng)
        off = np.r_[0, np.cumsum(sizes)].astype(np.int64)
        assert off[-1] == E and (runs == 1 or (0 in sizes and 1 in sizes))
        pre = np.concatenate([lo + np.argsort(-(w[lo:hi] + 0.0), kind="stable") for lo, hi in zip(off, off[1:])])
        ga, gb, gw = (host(x) for x in pkg.merge_sorted_runs(*dev_edges(a[pre], b[pre], w[pre]), off, ctx=ctx))
        assert np.array_equal(ga, a[want]) and np.array_equal(gb, b[want]), (family, E, runs)
        assert bits_eq(gw, w[want]) and np.array_equal(np.signbit(gw), np.signbit(w[want])), (family, E, runs)
    zero = w[want] == 0.0
    if family in H.SIGNED_ZERO:
        assert np.signbit(w[want][zero]).any() and not np.signbit(w[want][zero]).all()
        assert np.all(np.diff(a[want][zero]) > 0)  # input order inside the zero tie group


# ------------------------------------------------------------------------ small trees, all calls
@pytest.mark.parametrize("case,mcs", CASE_MCS, ids=IDS)
def test_device_equals_reference_and_host(pkg, ctx, case, mcs):
    va, vb, w, n = H.tree_case(case)
    ref = H.ref_tree(case, mcs)
    report("%s mcs %d" % (H.case_id(case), mcs), ref)
    want = pkg.cluster_tree(va, vb, w, n, mcs)  # the host path
    d = dev_edges(va, vb, w)
    # flat labels: descending (no sort), ascending and shuffled (the sort path)
    rng = np.random.default_rng(n + mcs)
    for i, o in enumerate(orders(va, vb, w, rng)):
        lab, k = pkg.flat_labels(*dev_edges(*o), n, mcs, ctx=ctx)
        assert lab.is_cuda and k == ref.n_clusters and np.array_equal(host(lab), ref.flat), (case, mcs, i)
    # GLOSH with labels
    s, e, lab, k = pkg.outlier_scores(*d, n, mcs, ctx=ctx, with_labels=True)
    rs, re = H.ref_glosh(case, mcs)
    assert bits_eq(host(e), re) and bits_eq(host(s), rs), (case, mcs)
    assert k == ref.n_clusters and np.array_equal(host(lab), ref.flat)
    hs, he = pkg.outlier_scores(va, vb, w, n, mcs)
    assert bits_eq(host(e), he) and bits_eq(host(s), hs)
    # the cluster tree, every array
    t = pkg.cluster_tree(*d, n, mcs, ctx=ctx)
    assert t.parent.is_cuda and t.point_level.is_cuda
    th = t.host()
    same_tree(th, ref, (case, mcs, "reference"))
    same_tree(th, want, (case, mcs, "host"))
    assert not np.signbit(th.birth[th.birth == 0]).any() and not np.signbit(th.point_level[th.point_level == 0]).any()
    # level cuts at every level, both zeros, +-inf, +-1e-17 and the midpoints
    levels = H.case_levels(case)
    rows = host(pkg.labels_at_levels(t, cuda(levels, np.float64), ctx=ctx))
    assert np.array_equal(rows, H.ref_cuts(ref, levels)), (case, mcs)
    assert np.array_equal(rows, pkg.labels_at_levels(want, levels))
    # constrained extraction over the device's own tree
    c = H.constraints_of(case, mcs)
    r = pkg.constrained_flat_labels(t, *[cuda(x, np.int32) for x in c], ctx=ctx)
    assert r.labels.is_cuda and r.prop_stability.is_cuda
    same_constrained(HostConstrained(r), H.ref_constrained(case, mcs), (case, mcs, "reference"))
    same_constrained(HostConstrained(r), pkg.constrained_flat_labels(want, *c), (case, mcs, "host"))
    # predict_labels at the same levels, and the identity
    nearest, level = H.queries_of(case, mcs)
    got = pkg.predict_labels(t, cuda(nearest, np.int32), cuda(level, np.float64), ctx=ctx)
    assert all(g.is_cuda for g in got)
    same_prediction([host(g) for g in got], predict_ref(ref, nearest, level), (case, mcs, "reference"))
    same_prediction([host(g) for g in got], pkg.predict_labels(want, nearest, level), (case, mcs, "host"))
    tl, lab, sc = pkg.predict_labels(t, torch.arange(n, dtype=torch.int32, device="cuda"), t.point_level, ctx=ctx)
    assert np.array_equal(host(tl), ref.point_cluster) and np.array_equal(host(lab), ref.flat) and bits_eq(host(sc), rs)


@pytest.mark.parametrize("case,mcs", [(("extremes", 300), 2), (("caterpillar", None), 2)], ids=["extremes-300", "caterpillar"])
def test_host_arrays_staged(pkg, ctx, case, mcs):
    """host arrays with a context: the device algorithm, results in host memory"""
    va, vb, w, n = H.tree_case(case)
    ref = H.ref_tree(case, mcs)
    report("%s staged" % H.case_id(case), ref)
    lab, k = pkg.flat_labels(va, vb, w, n, mcs, ctx=ctx)
    assert isinstance(lab, np.ndarray) and k == ref.n_clusters and np.array_equal(lab, ref.flat)
    s, e = pkg.outlier_scores(va, vb, w, n, mcs, ctx=ctx)
    rs, re = H.ref_glosh(case, mcs)
    assert bits_eq(e, re) and bits_eq(s, rs)
    t = pkg.cluster_tree(va, vb, w, n, mcs, ctx=ctx)
    assert isinstance(t.parent, np.ndarray)
    same_tree(t, ref, case)
    levels = H.case_levels(case)
    assert np.array_equal(pkg.labels_at_levels(t, levels, ctx=ctx), H.ref_cuts(ref, levels))
    c = H.constraints_of(case, mcs)
    same_constrained(pkg.constrained_flat_labels(t, *c, ctx=ctx), H.ref_constrained(case, mcs), case)
    nearest, level = H.queries_of(case, mcs)
    same_prediction(pkg.predict_labels(t, nearest, level, ctx=ctx), predict_ref(ref, nearest, level), case)


# -------------------------------------------------------------------- larger trees against the host
@pytest.fixture(scope="module")
def host20k(pkg):
    out = {}

    def get(family):
        if family not in out:
            va, vb, w, n = H.big_case(family)
            out[family] = {mcs: (pkg.cluster_tree(va, vb, w, n, mcs), pkg.outlier_scores(va, vb, w, n, mcs))
                           for mcs in H.MCS}
        return out[family]
    return get


@pytest.mark.parametrize("family", ["tiny_normal", "extremes", "inf_tenth"])
def test_20000_points_across_k6_settings(pkg, ctx, host20k, family):
    """beyond the 1,024-rank LDS blocks and the 4,096-rank mid depths: every depth split and both
    label schemes give the host's tree, labels and scores"""
    va, vb, w, n = H.big_case(family)
    want = host20k(family)
    for mcs in H.MCS:
        report("%s 20000 mcs %d" % (family, mcs), want[mcs][0])
    d = dev_edges(va, vb, w)
    for mid in (0, 12):
        for blk in (0, 8, 10):
            for relabel in (0, 1):
                with options(ctx, flat_mid_log=mid, flat_block_log=blk, flat_relabel=relabel):
                    for mcs in H.MCS:
                        where = (family, mid, blk, relabel, mcs)
                        tw, (sw, ew) = want[mcs]
                        t = pkg.cluster_tree(*d, n, mcs, ctx=ctx)
                        same_tree(t.host(), tw, where)
                        lab, k = pkg.flat_labels(*d, n, mcs, ctx=ctx)
                        assert k == tw.n_clusters and np.array_equal(host(lab), tw.flat_labels()), where
                        s, e = pkg.outlier_scores(*d, n, mcs, ctx=ctx)
                        assert bits_eq(host(s), sw) and bits_eq(host(e), ew), where
    tw = want[2][0]
    t = pkg.cluster_tree(*d, n, 2, ctx=ctx)
    lv = H.cut_levels(w)
    lv = np.r_[lv[:: max(1, lv.shape[0] // 60)], lv[-6:]]  # a sample of the levels, the special values
    assert np.array_equal(host(pkg.labels_at_levels(t, cuda(lv, np.float64), ctx=ctx)), pkg.labels_at_levels(tw, lv))
    rng = np.random.default_rng(5)
    nearest, level = rng.integers(-1, n, 4000).astype(np.int32), lv[rng.integers(0, lv.shape[0], 4000)]
    got = pkg.predict_labels(t, cuda(nearest, np.int32), cuda(level, np.float64), ctx=ctx)
    same_prediction([host(g) for g in got], pkg.predict_labels(tw, nearest, level), family)
    c = H.random_constraints(n, 4097, 3)
    r = pkg.constrained_flat_labels(t, *[cuda(x, np.int32) for x in c], ctx=ctx)
    same_constrained(HostConstrained(r), pkg.constrained_flat_labels(tw, *c), family)


# ------------------------------------------------------------------------ end to end, non-Euclidean
@pytest.mark.parametrize("metric", H.MSTS)
def test_k2g_tree_through_the_hierarchy_and_predict(pkg, ctx, metric):
    """exactMST (K2g) -> sort_edges_desc -> cluster_tree -> approximate_predict on rays(1500, 5):
    nearly every tree weight is a few ulps below zero"""
    min_pts, mcs, m = 4, 5, 300
    X, core_ref, lo, hi, w_ref, n = H.real_mst(metric)
    star = pkg.HDBSCANStar(ctx)
    core, g = star.exactMST(cuda(X, np.float64), min_pts, metric, pkg.CORE_INCL_SELF_CUMULATIVE, selfEdges=False)
    assert bits_eq(host(core), core_ref)
    assert edge_set(host(g.getVerticeA()), host(g.getVericeB()), host(g.getEges())) == edge_set(lo, hi, w_ref)
    va, vb, w = pkg.sort_edges_desc(g.getVerticeA(), g.getVericeB(), g.getEges(), ctx)
    hw = host(w)
    assert np.all(hw[1:] <= hw[:-1]) and (hw < 0).sum() > 100
    ref = H.ref_tree((metric, None), mcs)
    s = report("%s rays MST" % metric, ref)
    tree = pkg.cluster_tree(va, vb, w, n, mcs, ctx=ctx)
    same_tree(tree.host(), ref, metric)
    assert (ref.birth[1:] < 0).any() and s["negative"] > 0
    # queries: scaled copies (the same direction: distances a few ulps either side of zero), exact copies, fresh rows
    rng = np.random.default_rng(1500 + len(metric))
    from metric_kruskal import rays
    Q = np.ascontiguousarray(rays(m + 9, 5)[:m], np.float64)
    pick, kind = rng.integers(0, n, m), rng.integers(0, 3, m)
    Q[kind == 0] = (X[pick] * np.round(rng.uniform(0.5, 3.0, (m, 1)), 1))[kind == 0]
    Q[kind == 1] = X[pick][kind == 1]
    p = pkg.approximate_predict(tree, cuda(X, np.float64), core, cuda(Q, np.float64), min_pts, distanceFunction=metric,
                                ctx=ctx)
    cq, nearest, level = attach_ref(X, core_ref, Q, min_pts, metric)
    assert np.array_equal(host(p.nearest), nearest) and bits_eq(host(p.level), level) and bits_eq(host(p.core), cq)
    same_prediction((host(p.tree_labels), host(p.labels), host(p.scores)), predict_ref(ref, nearest, level), metric)
    assert (level[nearest >= 0] < 0).any()  # a query attaches at a negative level
