"""Out-of-sample prediction on the device: the attach scan (csrc/attach.hip, hdb_attach_points)
bit for bit against the brute-force restatement (tests/predict_ref.py: oracle distances, strict
insertion, plain arg-min), on the smallest shapes that reach each path -- ragged query and candidate
tiles, n < K, a single row, the dimension-chunk boundary, all five metrics, forced candidate splits
-- and on tie-heavy and non-finite input; hdb_predict_labels on the device against its host path;
and approximate_predict end to end."""
import functools

import numpy as np
import pytest
import torch

from conftest import blobs
from constraints_reference import big_tree
from metric_kruskal import rays, rounded_blobs, zero_row
from predict_ref import JMAX, attach_ref, cross_distances, predict_ref
from test_cluster_tree import K_VA, K_VB, K_W
from test_outlier_scores import bits
from test_predict_host import BAD, CASES, Tree, blob_tree_edges, same_prediction

pytestmark = pytest.mark.gpu

NAN = float("nan")
INF = float("inf")


@pytest.fixture(scope="module")
def ctx(pkg):
    c = pkg.Context(0)
    c.use_torch_stream()  # the attach scan is stream-ordered: results are read on torch's stream
    return c


def cuda(x, dt):
    return torch.from_numpy(np.array(x, dtype=dt, order="C")).cuda()


def host(x):
    return x.cpu().numpy() if torch.is_tensor(x) else np.asarray(x)


FAMILY = {"rounded_blobs": rounded_blobs, "rays": rays, "zero_row": zero_row}


@functools.lru_cache(maxsize=None)
def attach_case(metric, family, n, m, d, min_pts, variant=""):
    """(X, core, Q, reference outputs), computed once.  Training rows: the family, the second half
    copies of the first for "dup".  Queries: scaled copies of training rows (the same direction:
    cosine and Pearson values a few ulps either side of 0), exact copies, and fresh rows.  Cores:
    the oracle's for the metric.  "nonfinite": NaN and +-inf coordinates in both sets and NaN, +inf
    and -0.0 cores."""
    from oracle import oracle as O
    rng = np.random.default_rng(977 * n + 31 * m + d + min_pts)
    X = np.ascontiguousarray(FAMILY[family](max(n, 8), d)[:n], np.float64)
    if "dup" in variant:
        X[n // 2:] = X[: n - n // 2]
    fresh = np.ascontiguousarray(FAMILY[family](m + 9, d)[:m], np.float64)
    Q = fresh.copy()
    pick = rng.integers(0, n, m)
    kind = rng.integers(0, 3, m)
    scale = np.round(rng.uniform(0.5, 3.0, (m, 1)), 1) if family != "rounded_blobs" else np.ones((m, 1))
    Q[kind == 0] = (X[pick] * scale)[kind == 0]
    Q[kind == 1] = X[pick][kind == 1]
    core = O.core_distances(X, min_pts, metric=metric) if n >= 2 else np.zeros(n)
    core = np.ascontiguousarray(core, np.float64).copy()
    if "nonfinite" in variant:
        for k, v in enumerate((NAN, INF, -INF)):
            X[(5 * k + 1) % n, k % d] = v
            Q[(7 * k + 2) % m, (k + 1) % d] = v
        Q[m // 2] = NAN
        core[0 % n], core[3 % n], core[(n // 2) % n] = NAN, INF, -0.0
        core[(n - 1) // 3] = -0.0
    ref = attach_ref(X, core, Q, min_pts, metric)
    for a in (X, core, Q) + ref:
        a.setflags(write=False)
    return X, core, Q, ref


def dev_attach(pkg, ctx, X, core, Q, min_pts, metric, attach_splits=0):
    out = pkg.HDBSCANStar(ctx).attachPoints(cuda(X, np.float64), cuda(core, np.float64), cuda(Q, np.float64), min_pts,
                                            metric, attach_splits)
    assert all(torch.is_tensor(o) and o.is_cuda for o in out)
    return tuple(host(o) for o in out)


def same_attach(got, want, where=None):
    for g, w, k in zip(got, want, ("core_q", "nearest", "level")):
        if k == "nearest":
            assert g.dtype == np.int32 and np.array_equal(g, w), (k, where, np.flatnonzero(g != w)[:5])
        else:
            bad = np.flatnonzero(bits(g) != bits(w))
            assert bad.shape[0] == 0, (k, where, bad[:5], g[bad[:5]], w[bad[:5]])


# every n in {1, 3, 64, 65, 1500}, m in {1, 63, 257}, d in {1, 3, 8, 9, 24}, minPts in {2, 4, 16} (K = KC), every metric
ATTACH = [
    ("euclidean", "rounded_blobs", 1500, 257, 3, 4, ""),
    ("euclidean", "rounded_blobs", 65, 63, 9, 16, "dup"),
    ("euclidean", "rounded_blobs", 64, 1, 8, 2, ""),
    ("euclidean", "rounded_blobs", 3, 63, 1, 16, ""),       # n < K: the lists keep Double.MAX_VALUE
    ("euclidean", "rounded_blobs", 1, 1, 24, 2, ""),        # a single training row
    ("euclidean", "rounded_blobs", 65, 257, 24, 4, "nonfinite"),
    ("manhattan", "rounded_blobs", 1500, 63, 24, 4, "dup"),
    ("manhattan", "rounded_blobs", 3, 1, 1, 16, ""),
    ("manhattan", "rounded_blobs", 65, 63, 9, 2, "nonfinite"),
    ("supremum", "rounded_blobs", 65, 257, 9, 16, ""),
    ("supremum", "rounded_blobs", 64, 63, 8, 4, "nonfinite dup"),
    ("cosine", "rays", 1500, 63, 9, 4, ""),
    ("cosine", "zero_row", 65, 257, 3, 2, ""),
    ("cosine", "rays", 64, 63, 24, 16, "nonfinite"),
    ("pearson", "rays", 65, 257, 24, 2, "dup"),
    ("pearson", "zero_row", 1500, 63, 8, 4, ""),
    ("pearson", "rays", 3, 1, 1, 4, ""),                     # d = 1: no variance, every distance NaN
    ("pearson", "rays", 65, 63, 3, 16, "nonfinite"),
]
# K = minPts - 1 below the list capacity KC of {1, 3, 7, 15, 31}: the kernels for 7 and 31 entries, and the merge
# kernel's "entry K - 1" pick with K < KC; minPts 32 is the largest K.  n = 65: two candidate tiles
ATTACH_KC = [
    ("euclidean", "rounded_blobs", 65, 63, 3, 3, ""),
    ("cosine", "rays", 65, 63, 9, 6, ""),
    ("euclidean", "rounded_blobs", 65, 257, 8, 20, "dup"),
    ("cosine", "rays", 65, 63, 5, 32, ""),
    ("euclidean", "rounded_blobs", 65, 63, 9, 6, "nonfinite"),
    ("cosine", "rays", 9, 63, 3, 20, ""),                    # n < K < KC
]


@pytest.mark.parametrize("case", ATTACH + ATTACH_KC, ids=lambda c: "-".join(str(x) for x in c if x != ""))
def test_attach_equals_reference(pkg, ctx, case):
    metric, family, n, m, d, min_pts, variant = case
    X, core, Q, ref = attach_case(*case)
    got = dev_attach(pkg, ctx, X, core, Q, min_pts, metric)
    same_attach(got, ref, case)
    none = ref[1] < 0
    assert np.all(got[2][none] == JMAX)
    if case == ATTACH[-2]:
        assert none.all() and np.all(got[0] == JMAX)
    if "nonfinite" in variant and metric != "supremum":  # SupremumDistance's 'diff > max' skips a NaN difference
        assert none[m // 2]  # the NaN query row
    if n < min_pts - 1:
        assert np.all(got[0] == JMAX)
    # the inputs do hold what they are there for: ties in w, negative and zero cosine values, NaN pairs
    if case == ATTACH[0]:
        assert np.unique(ref[2]).shape[0] < m
    if case == ATTACH[11]:
        D = cross_distances(Q, X, "cosine")
        assert (D < 0).any() and (D == 0).any()
    if case == ATTACH[12]:
        assert np.isnan(cross_distances(Q, X, "cosine")[:, 7]).all()


@pytest.mark.parametrize("case", [ATTACH[1], ATTACH[0], ATTACH[6], ATTACH[11], ATTACH[5]] + ATTACH_KC,
                         ids=lambda c: "-".join(str(x) for x in c if x != ""))
def test_forced_splits(pkg, ctx, case):
    """the merge kernels at small n: any split count gives the same bits"""
    metric, family, n, m, d, min_pts, variant = case
    X, core, Q, ref = attach_case(*case)
    ctx.set_timing(True)
    try:
        for splits in (1, 2, 7):
            ctx.kernel_time("attach_knn"), ctx.kernel_time("attach_min")
            got = dev_attach(pkg, ctx, X, core, Q, min_pts, metric, attach_splits=splits)
            assert ctx.get_stat("attach_last_splits") == splits
            assert ctx.kernel_time("attach_knn")[1] == 1 and ctx.kernel_time("attach_min")[1] == 1
            same_attach(got, ref, (case, splits))
    finally:
        ctx.set_timing(False)
    dev_attach(pkg, ctx, X, core, Q, min_pts, metric)
    assert 1 <= ctx.get_stat("attach_last_splits") <= -(-n // 64)


def test_core_q_is_the_excl_self_core_distance(pkg, ctx):
    for case in (ATTACH[0], ATTACH[6], ATTACH[11]):
        metric, family, n, m, d, min_pts, variant = case
        X, core, Q, (cq, _, _) = attach_case(*case)
        H = pkg.HDBSCANStar(ctx)
        for i in (0, 1, m // 2, m - 1):
            both = cuda(np.vstack([X, Q[i]]), np.float64)
            c = host(H.calculateCoreDistances(both, min_pts, metric, pkg.CORE_EXCL_SELF))
            assert bits(c[-1:]).tolist() == bits(cq[i:i + 1]).tolist(), (case, i)


def test_pointer_placement_and_status(pkg, ctx):
    case = ATTACH[1]
    metric, family, n, m, d, min_pts, variant = case
    X, core, Q, ref = attach_case(*case)
    H = pkg.HDBSCANStar(ctx)
    out = H.attachPoints(X, core, Q, min_pts, metric)  # all host
    assert all(isinstance(o, np.ndarray) for o in out)
    same_attach(out, ref, "host")
    out = H.attachPoints(cuda(X, np.float64), core, Q, min_pts, metric)  # mixed: results where Q lives
    assert all(isinstance(o, np.ndarray) for o in out)
    same_attach(out, ref, "mixed")
    out = H.attachPoints(X, cuda(core, np.float64), cuda(Q, np.float64), min_pts, metric)
    same_attach(tuple(host(o) for o in out), ref, "mixed2")
    # core_q is nullable
    A, L = pkg._capi, pkg.lib()
    nearest, level = np.empty(m, np.int32), np.empty(m, np.float64)
    args = (A.ptr(X), n, d, A.ptr(core), A.ptr(Q), m, min_pts, 0)
    assert L.hdb_attach_points(ctx.h, *args, None, A.ptr(nearest), A.ptr(level)) == 0
    same_attach((ref[0], nearest, level), ref, "no core_q")
    # m == 0, n == 0, minPts 1, and the statuses
    assert L.hdb_attach_points(ctx.h, A.ptr(X), n, d, A.ptr(core), None, 0, min_pts, 0, None, None, None) == 0
    cq, nr, lv = H.attachPoints(np.zeros((0, d)), np.zeros(0), Q, min_pts, metric)
    assert np.all(cq == JMAX) and np.all(nr == -1) and np.all(lv == JMAX)
    cq, nr, lv = H.attachPoints(X, core, Q, 1, metric)
    assert np.all(cq == 0.0)
    same_attach((ref[0], nr, lv), (ref[0],) + attach_ref(X, core, Q, 1, metric)[1:], "minPts 1")
    for bad_min_pts in (0, 33):
        with pytest.raises(pkg.HdbError) as ei:
            H.attachPoints(X, core, Q, bad_min_pts, metric)
        assert ei.value.code == -1
        with pytest.raises(pkg.HdbError) as ej:
            H.calculateCoreDistances(X, bad_min_pts, metric, pkg.CORE_EXCL_SELF)
        assert str(ei.value).split(": ", 2)[2] == str(ej.value).split(": ", 2)[2]  # the same error
    for bad_splits in (-1, 65536):  # the count is an argument of the call; the context has no such option
        with pytest.raises(pkg.HdbError, match="attach_splits") as ei:
            H.attachPoints(X, core, Q, min_pts, metric, bad_splits)
        assert ei.value.code == -1
    with pytest.raises(pkg.HdbError, match="unknown option"):
        ctx.set_option("attach_splits", 2)
    assert L.hdb_attach_points(ctx.h, A.ptr(X), 2 ** 31, d, A.ptr(core), A.ptr(Q), m, min_pts, 0, None, A.ptr(nearest),
                               A.ptr(level)) == -1


# ------------------------------------------------------------------ hdb_predict_labels on the device
class DevTree:
    def __init__(self, t):
        for k in ("parent", "birth", "death", "flat_label", "point_cluster", "point_level"):
            a = np.ascontiguousarray(getattr(t, k))
            setattr(self, k, torch.from_numpy(a).cuda())


@pytest.mark.parametrize("case", CASES)
def test_predict_device_equals_host(pkg, ctx, case):
    n, d, dup, min_pts, mcs = case
    va, vb, w = blob_tree_edges(n, d, dup, min_pts)
    t = pkg.cluster_tree(va, vb, w, n, mcs)
    rng = np.random.default_rng(n + d)
    m = 1000
    nearest = rng.integers(-1, n, m).astype(np.int32)
    level = np.r_[rng.choice(t.birth[1:], m // 2), rng.uniform(0, float(w.max()) * 1.2, m - m // 2 - 3), INF, -INF, 0.0]
    level = level[rng.permutation(m)]
    want = pkg.predict_labels(t, nearest, level)
    same_prediction(want, predict_ref(t, nearest, level), case)
    dt = DevTree(t)
    got = pkg.predict_labels(dt, cuda(nearest, np.int32), cuda(level, np.float64), ctx=ctx)
    assert all(torch.is_tensor(g) and g.is_cuda for g in got)
    same_prediction([host(g) for g in got], want, ("device", case))
    got = pkg.predict_labels(t, nearest, level, ctx=ctx)  # host arrays through the device path
    same_prediction(got, want, ("staged", case))
    mixed = DevTree(t)
    mixed.birth, mixed.point_cluster = t.birth, t.point_cluster
    got = pkg.predict_labels(mixed, nearest, cuda(level, np.float64), ctx=ctx)
    same_prediction([host(g) for g in got], want, ("mixed", case))
    # identity on the device
    tl, lab, sc = pkg.predict_labels(dt, torch.arange(n, dtype=torch.int32, device="cuda"), dt.point_level, ctx=ctx)
    assert np.array_equal(host(tl), t.point_cluster) and np.array_equal(host(lab), t.flat_labels())
    with np.errstate(all="ignore"):
        assert np.array_equal(bits(host(sc)), bits(t.outlier_scores()))


def test_predict_device_small_trees_and_errors(pkg, ctx):
    t = pkg.cluster_tree(K_VA, K_VB, K_W, 8, 2)
    nearest = np.array([0, 0, 3, 3, 3, 6, 6, 2, -1], np.int32)
    level = np.array([0.25, 5.0, 2.9, 3.0, 4.9, 3.0, 7.0, 2.0, NAN])
    same_prediction(pkg.predict_labels(t, nearest, level, ctx=ctx), pkg.predict_labels(t, nearest, level))
    va, vb, w = np.arange(4, dtype=np.int32), np.arange(1, 5, dtype=np.int32), np.array([1.0, 2.0, 3.0, 4.0])
    t1 = pkg.cluster_tree(va, vb, w, 5, 4)  # K = 1
    nr, lv = np.array([0, 4, 2, -1], np.int32), np.array([0.5, 9.0, INF, 1.0])
    same_prediction(pkg.predict_labels(t1, nr, lv, ctx=ctx), pkg.predict_labels(t1, nr, lv))
    tl, lab, sc = pkg.predict_labels(t, np.zeros(0, np.int32), np.zeros(0), ctx=ctx)
    assert tl.shape == (0,)
    t0 = pkg.cluster_tree(np.zeros(0, np.int32), np.zeros(0, np.int32), np.zeros(0), 0, 2)
    tl, lab, sc = pkg.predict_labels(t0, [-1, -1], [1.0, NAN], ctx=ctx)
    assert tl.tolist() == [0, 0] and lab.tolist() == [0, 0] and sc.tolist() == [1.0, 1.0]
    for change, field in BAD:
        nearest = np.array(change.get("nearest", [0]), np.int32)
        level = np.array(change.get("level", [1.0] * nearest.shape[0]), np.float64)
        bad = Tree(t, **{k: np.array(v, np.int32) for k, v in change.items() if k in ("parent", "point_cluster")})
        with pytest.raises(pkg.HdbError, match=field) as ei:
            pkg.predict_labels(bad, nearest, level, ctx=ctx)
        assert ei.value.code == -1
    # only the outputs asked for
    A, L = pkg._capi, pkg.lib()
    dt = DevTree(t)
    nr, lv = cuda([0, 6, -1], np.int32), cuda([4.0, 0.5, 1.0], np.float64)
    full = pkg.predict_labels(dt, nr, lv, ctx=ctx)
    args = [A.ptr(getattr(dt, k)) for k in ("parent", "birth", "death", "flat_label")]
    for keep in range(3):
        outs = [torch.zeros(3, dtype=torch.int32, device="cuda"), torch.zeros(3, dtype=torch.int32, device="cuda"),
                torch.zeros(3, dtype=torch.float64, device="cuda")]
        ptrs = [A.ptr(o) if k == keep else None for k, o in enumerate(outs)]
        assert L.hdb_predict_labels(ctx.h, *args, 5, A.ptr(dt.point_cluster), A.ptr(dt.point_level), 8, A.ptr(nr),
                                    A.ptr(lv), 3, *ptrs) == 0
        assert torch.equal(outs[keep], full[keep])


def test_predict_on_a_large_real_tree(pkg, ctx):
    """about 1e5 clusters from a real cluster_tree (the doubling rounds over a deep tree)"""
    n, mcs = 260000, 2
    va, vb, w = big_tree(n, None, 23)
    dev = pkg.cluster_tree(cuda(va, np.int32), cuda(vb, np.int32), cuda(w, np.float64), n, mcs, ctx=ctx)
    t = dev.host()
    assert 60000 <= t.n_tree <= pkg.cluster_tree_bound(n, mcs)
    rng = np.random.default_rng(3)
    m = 50000
    nearest = rng.integers(-1, n, m).astype(np.int32)
    level = np.where(rng.random(m) < 0.5, rng.choice(t.birth[1:], m), rng.random(m) * 1.1)
    want = pkg.predict_labels(t, nearest, level)
    got = pkg.predict_labels(dev, cuda(nearest, np.int32), cuda(level, np.float64), ctx=ctx)
    same_prediction([host(g) for g in got], want)
    y = np.arange(n, dtype=np.int32)
    tl, lab, sc = pkg.predict_labels(dev, cuda(y, np.int32), dev.point_level, ctx=ctx)
    assert np.array_equal(host(tl), t.point_cluster) and np.array_equal(host(lab), host(dev.flat_labels()))
    assert np.array_equal(bits(host(sc)), bits(host(dev.outlier_scores())))


def test_approximate_predict_end_to_end(pkg, ctx):
    n, d, m, min_pts, mcs = 3000, 5, 500, 4, 5
    X = np.ascontiguousarray(blobs(n + m, d, 6, 41, spread=10.0), np.float64)
    X, Q = X[:n], X[n:]
    H = pkg.HDBSCANStar(ctx)
    core, g = H.exactMST(cuda(X, np.float64), min_pts)
    tree = pkg.cluster_tree(g.getVerticeA(), g.getVericeB(), g.getEges(), n, mcs, ctx=ctx)
    assert tree.n_clusters >= 2
    p = pkg.approximate_predict(tree, cuda(X, np.float64), core, cuda(Q, np.float64), min_pts, ctx=ctx)
    for k in ("labels", "tree_labels", "nearest", "level", "core", "scores"):
        assert torch.is_tensor(getattr(p, k)) and getattr(p, k).is_cuda and getattr(p, k).shape == (m,), k
    ref = attach_ref(X, host(core), Q, min_pts)
    same_attach((host(p.core), host(p.nearest), host(p.level)), ref, "end to end")
    th = tree.host()
    same_prediction((host(p.tree_labels), host(p.labels), host(p.scores)), predict_ref(th, ref[1], ref[2]))
    assert (host(p.labels) > 0).mean() > 0.5  # fresh draws of the same blobs mostly land in clusters
    # host inputs give host outputs with the same bits
    ph = pkg.approximate_predict(th, X, host(core), Q, min_pts, ctx=ctx)
    assert isinstance(ph.labels, np.ndarray)
    same_attach((ph.core, ph.nearest, ph.level), ref, "host in")
    same_prediction((ph.tree_labels, ph.labels, ph.scores), (host(p.tree_labels), host(p.labels), host(p.scores)))
