"""Constraint-aware flat extraction on the device (csrc/constraints.hip) against the top-down
reference (tests/constraints_reference.py) and the host path (csrc/constraints.cpp): every array
equal, prop_stability bit for bit -- on the smallest shapes that reach each path: constraint
counts that are no multiple of a workgroup, hundreds of siblings born at one level (the child
order of the stability sum), a tree thousands deep (the lifting and the single-launch climb),
10,000 copies of one pair (atomic contention), mixed host and device arrays, and the statuses."""
import numpy as np
import pytest
import torch

from cluster_tree_reference import cluster_tree_reference
from constraints_reference import big_tree, constraints_reference, random_constraints
from test_constraints import HAND, cons, hand_tree, same_result

pytestmark = pytest.mark.gpu
ML, CL = 0, 1


@pytest.fixture(scope="module")
def ctx(pkg):
    return pkg.Context.get(0)


def cuda(x, dt=np.int32):
    return torch.from_numpy(np.ascontiguousarray(x, dt)).cuda()


def dev_tree(pkg, t):
    """the host tree's arrays as device tensors"""
    f = [cuda(getattr(t, k), np.float64 if k in ("birth", "death", "stability", "point_level") else np.int32)
         for k in pkg.ClusterTree.FIELDS]
    return pkg.ClusterTree(*f, t.n_clusters)


class Host:
    def __init__(self, r):
        for k in ("num_sat", "prop_sat", "prop_stability", "flat_label", "labels"):
            x = getattr(r, k)
            setattr(self, k, x.cpu().numpy() if torch.is_tensor(x) else x)
        self.n_clusters = r.n_clusters


def dev_run(pkg, ctx, t, c):
    r = pkg.constrained_flat_labels(dev_tree(pkg, t), *[cuda(x) for x in c], ctx=ctx)
    assert torch.is_tensor(r.labels) and r.labels.is_cuda and r.prop_stability.is_cuda
    return Host(r)


@pytest.mark.parametrize("case", range(len(HAND)))
def test_hand_worked_vectors_on_the_device(pkg, ctx, case):
    which, rows = HAND[case][:2]
    t, _ = hand_tree(pkg, which)
    same_result(dev_run(pkg, ctx, t, cons(rows)), pkg.constrained_flat_labels(t, *cons(rows)), case)


@pytest.fixture(scope="module")
def trees2000(pkg):
    out = {}
    for ties in (False, True):
        va, vb, w = big_tree(2000, 6 if ties else None, 7 + ties)
        for mcs in (2, 5):
            out[ties, mcs] = (pkg.cluster_tree(va, vb, w, 2000, mcs), cluster_tree_reference(va, vb, w, 2000, mcs))
    return out


@pytest.mark.parametrize("ties", [False, True])
@pytest.mark.parametrize("mcs", [2, 5])
def test_device_equals_reference(pkg, ctx, trees2000, ties, mcs):
    t, ref = trees2000[ties, mcs]
    for m in (1, 64, 5000):
        c = random_constraints(2000, m, 100 * m + mcs + ties)
        same_result(dev_run(pkg, ctx, t, c), constraints_reference(ref, *c), (ties, mcs, m))


@pytest.fixture(scope="module")
def host20k(pkg):
    out = {}
    for values in (None, 50):
        va, vb, w = big_tree(20000, values, 11)
        out[values] = {mcs: pkg.cluster_tree(va, vb, w, 20000, mcs) for mcs in (2, 5)}
    return out


@pytest.mark.parametrize("values", [None, 50])
@pytest.mark.parametrize("mcs", [2, 5])
def test_device_equals_host_20000(pkg, ctx, host20k, values, mcs):
    """50 distinct weights: hundreds of siblings born at one level; no m is a multiple of 256"""
    t = host20k[values][mcs]
    if values == 50 and mcs == 2:
        assert np.bincount(t.parent).max() >= 200  # children of one cluster
    differs = 0
    for m in (0, 1, 257, 4097, 100000):
        c = random_constraints(20000, m, m + mcs)
        got = dev_run(pkg, ctx, t, c)
        same_result(got, pkg.constrained_flat_labels(t, *c), (values, mcs, m))
        if m == 0:
            assert np.array_equal(got.flat_label, t.flat_label) and np.array_equal(got.labels, t.flat_labels())
        differs += not np.array_equal(got.flat_label, t.flat_label)
    assert differs >= 2


def test_deep_tree(pkg, ctx):
    """ascending weights along a path, minClSize 2, one straggler per node so that every step is a
    true split: the cluster tree is a chain thousands deep -- one lane climbs it in one launch,
    and the lifting lifts across it"""
    P = 3001
    i = np.arange(P)
    va = np.r_[2 * i, 2 * i[:-1] + 1, 2 * i].astype(np.int32)
    vb = np.r_[2 * i + 1, 2 * i[1:], 2 * P + i].astype(np.int32)
    w = np.r_[1e-3 * (i + 1), 10.0 + i[:-1], 9.5 + i]
    n = 3 * P
    t = pkg.cluster_tree(va, vb, w, n, 2)
    depth, c = 0, int(t.point_cluster[0])
    while c:
        depth, c = depth + 1, int(t.parent[c - 1])
    assert depth > 2990
    rng = np.random.default_rng(3)
    far = (np.r_[rng.integers(0, 20, 500), rng.integers(0, n, 500)].astype(np.int32),  # shallow against deep
           rng.integers(0, n, 1000).astype(np.int32), (rng.random(1000) < 0.5).astype(np.int32))
    differs = 0
    for c in (random_constraints(n, 3001, 5), far, cons([(0, n - 1, ML)])):
        got = dev_run(pkg, ctx, t, c)
        same_result(got, pkg.constrained_flat_labels(t, *c), "deep")
        differs += not np.array_equal(got.flat_label, t.flat_label)
    assert differs


def test_contention_on_one_cluster(pkg, ctx):
    """10,000 copies of one must-link and of one cannot-link pair: every atomic of a kind lands on
    one word, and the counts are exact"""
    t, _ = hand_tree(pkg, "B")
    c = cons([(3, 6, ML)] * 10000 + [(8, 0, CL)] * 10000)
    got = dev_run(pkg, ctx, t, c)
    same_result(got, pkg.constrained_flat_labels(t, *c), "contention")
    # ML(3,6): 20,000 to cluster 3 and the root; CL(8,0): 10,000 to 2, to 3 and to 3's virtual child
    assert got.num_sat.tolist() == [20000, 10000, 30000, 0, 0] and got.prop_sat.tolist() == [40000, 0, 10000, 0, 0]


def test_mixed_host_and_device_arrays(pkg, ctx, trees2000):
    t, _ = trees2000[True, 2]
    c = random_constraints(2000, 777, 9)
    want = pkg.constrained_flat_labels(t, *c)
    staged = pkg.constrained_flat_labels(t, *c, ctx=ctx)  # host arrays + ctx: the device algorithm
    assert isinstance(staged.labels, np.ndarray)
    same_result(staged, want, "staged")
    d = dev_tree(pkg, t)
    same_result(Host(pkg.constrained_flat_labels(d, *c, ctx=ctx)), want, "device tree, host constraints")
    same_result(Host(pkg.constrained_flat_labels(t, *[cuda(x) for x in c], ctx=ctx)), want, "host tree, device constraints")
    mixed = dev_tree(pkg, t)
    mixed.stability, mixed.point_cluster = t.stability, t.point_cluster
    same_result(Host(pkg.constrained_flat_labels(mixed, c[0], cuda(c[1]), c[2], ctx=ctx)), want, "mixed")


def test_statuses_from_the_device(pkg, ctx):
    """the kernels bound-check what they are given: a status, nothing accessed out of range"""
    t, _ = hand_tree(pkg, "A")
    ca, cb, ct = cons(HAND[0][1])
    one = cuda(np.zeros(1))
    d = dev_tree(pkg, t)
    p = lambda x: x.data_ptr()
    rc = pkg.lib().hdb_constrained_flat_labels(ctx.h, p(d.parent), p(d.stability), p(d.min_id), 5, p(d.point_cluster), 8,
                                              p(one), p(one), p(one), 2 ** 30, *[None] * 6)
    assert rc == -1 and "2^30" in pkg.lib().hdb_last_error().decode()
    for field, values, word in [("parent", [1, 1, 1, 3, 3], "parent"), ("parent", [0, 1, 1, 4, 3], "parent"),
                                ("parent", [0, 1, 1, 3, 2 ** 31 - 1], "parent"), ("parent", [0, 1, -1, 3, 3], "parent"),
                                ("point_cluster", [2, 2, 2, 4, 4, 4, 5, 6], "point_cluster"),
                                ("point_cluster", [2, 2, 2, 4, 0, 4, 5, 5], "point_cluster"),
                                ("point_cluster", [2, 2, 2, -4, 4, 4, 5, 5], "point_cluster")]:
        bad = dev_tree(pkg, t)
        setattr(bad, field, cuda(values))
        with pytest.raises(pkg.HdbError, match=word) as ei:
            pkg.constrained_flat_labels(bad, cuda(ca), cuda(cb), cuda(ct), ctx=ctx)
        assert ei.value.code == -1
    for a, b, ty, word in [(8, 0, ML, "point id"), (0, -1, CL, "point id"), (0, 2 ** 31 - 1, ML, "point id"),
                           (0, 1, 2, "ctype"), (0, 1, -1, "ctype")]:
        xa, xb, xt = ca.copy(), cb.copy(), ct.copy()
        xa[2], xb[2], xt[2] = a, b, ty
        with pytest.raises(pkg.HdbError, match=word) as ei:
            pkg.constrained_flat_labels(d, cuda(xa), cuda(xb), cuda(xt), ctx=ctx)
        assert ei.value.code == -1
    # K = 1 and n = 0 on the device; a good call still works after the bad ones
    va, vb, w = np.arange(3, dtype=np.int32), np.arange(1, 4, dtype=np.int32), np.array([2.0, 7.0, 7.0])
    r = dev_run(pkg, ctx, pkg.cluster_tree(va, vb, w, 4, 5), cons([(0, 1, ML), (2, 2, ML), (0, 3, CL)]))
    assert r.n_clusters == 0 and r.labels.tolist() == [0] * 4 and r.num_sat.tolist() == [4] and r.prop_sat.tolist() == [0]
    e = np.zeros(0, np.int32)
    r = pkg.constrained_flat_labels(pkg.cluster_tree(e, e, np.zeros(0), 0, 2), e, e, e, ctx=ctx)
    assert r.n_clusters == 0 and r.labels.shape == (0,)
    same_result(dev_run(pkg, ctx, t, (ca, cb, ct)), pkg.constrained_flat_labels(t, ca, cb, ct), "after errors")


def test_driver_constraints(pkg):
    """MRHDBSCANStar(cluster_tree=True, constraints=...): out["constrained"] beside unchanged labels"""
    from conftest import blobs
    X = blobs(3000, 3, 6, 1)
    kw = dict(minPts=4, minClSize=4, processing_units=300, k=0.1)
    c = random_constraints(3000, 500, 1)
    base = pkg.MRHDBSCANStar(cluster_tree=True, **kw).run(X)
    got = pkg.MRHDBSCANStar(cluster_tree=True, constraints=c, **kw).run(X)
    assert "constrained" not in base and torch.equal(got["labels"], base["labels"])
    same_result(Host(got["constrained"]), pkg.constrained_flat_labels(got["cluster_tree"].host(), *c), "driver")
    with pytest.raises(ValueError):
        pkg.MRHDBSCANStar(constraints=c, **kw)
