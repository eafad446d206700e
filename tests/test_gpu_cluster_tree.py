"""The cluster tree export and the level-cut kernel on the device (csrc/flat.hip sections 7
and 8) against the test-side reference (tests/cluster_tree_reference.py) and the host path
(csrc/flat.cpp): every array, doubles bit for bit, on the smallest shapes that reach each path
-- both K6 label schemes and depth splits, hundreds of clusters born at one level (the
renumbering sort's tie rule), a cluster tree thousands deep (the binary-lifting climb), sizes
that are no multiple of a workgroup, mixed host and device arrays, K = 1, and the statuses."""
import ctypes as C

import numpy as np
import pytest
import torch

from cluster_tree_reference import cluster_tree_reference
from conftest import blobs
from test_cluster_tree import K_VA, K_VB, K_W, same_tree
from test_gpu_outlier_scores import big_tree
from test_outlier_scores import bits

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ctx(pkg):
    return pkg.Context.get(0)


def cuda(x, dt):
    return torch.from_numpy(np.ascontiguousarray(x, dt)).cuda()


def dev_tree(pkg, ctx, va, vb, w, n, mcs):
    """device-resident inputs; the record with device tensors"""
    return pkg.cluster_tree(cuda(va, np.int32), cuda(vb, np.int32), cuda(w, np.float64), n, mcs, ctx=ctx)


def dev_cuts(pkg, ctx, tree, levels):
    return pkg.labels_at_levels(tree, cuda(levels, np.float64), ctx=ctx).cpu().numpy()


@pytest.fixture(scope="module")
def ref2000():
    """the O(levels x n) reference, once per tree and minClSize"""
    out = {}
    for ties in (False, True):
        va, vb, w = big_tree(2000, 6 if ties else None, 7 + ties)
        out[ties] = (va, vb, w, {mcs: cluster_tree_reference(va, vb, w, 2000, mcs) for mcs in (2, 5)})
    return out


@pytest.mark.parametrize("ties", [False, True])
@pytest.mark.parametrize("mcs", [2, 5])
def test_device_equals_reference(pkg, ctx, ref2000, ties, mcs):
    va, vb, w, refs = ref2000[ties]
    ref = refs[mcs]
    t = dev_tree(pkg, ctx, va, vb, w, 2000, mcs)
    assert torch.is_tensor(t.parent) and t.parent.is_cuda and t.point_level.is_cuda
    same_tree(t.host(), ref, (ties, mcs))
    assert t.n_tree <= pkg.cluster_tree_bound(2000, mcs)
    snaps = ref.snapshots[:: max(1, len(ref.snapshots) // 40)]  # rows by brute force, no walk rule
    rows = dev_cuts(pkg, ctx, t, [lv for lv, _ in snaps])
    for (lv, snap), row in zip(snaps, rows):
        assert np.array_equal(row, snap), (ties, mcs, lv)


@pytest.fixture(scope="module")
def host20k(pkg):
    out = {}
    for values in (None, 50):
        va, vb, w = big_tree(20000, values, 11)
        out[values] = (va, vb, w, {mcs: pkg.cluster_tree(va, vb, w, 20000, mcs) for mcs in (2, 5)})
    return out


@pytest.mark.parametrize("values", [None, 50])
@pytest.mark.parametrize("relabel", [0, 1])
@pytest.mark.parametrize("mid", [0, 12])
def test_device_equals_host_across_k6_settings(pkg, ctx, host20k, values, relabel, mid):
    """n = 20,000: beyond the 1,024-rank LDS blocks and the 4,096-rank mid depths"""
    va, vb, w, ref = host20k[values]
    ctx.set_option("flat_relabel", relabel)
    ctx.set_option("flat_mid_log", mid)
    try:
        for mcs in (2, 5):
            t = dev_tree(pkg, ctx, va, vb, w, 20000, mcs)
            same_tree(t.host(), ref[mcs], (values, relabel, mid, mcs))
            lv = np.r_[ref[mcs].birth[1::211], ref[mcs].point_level[::4001], 0.3]
            assert np.array_equal(dev_cuts(pkg, ctx, t, lv), pkg.labels_at_levels(ref[mcs], lv))
    finally:
        ctx.set_option("flat_relabel", 1)
        ctx.set_option("flat_mid_log", 12)


def pair_groups(rng, levels):
    """two-point groups (inner weight 0.5), ids permuted.  levels = 1: 600 groups chained by
    weight-1.0 edges -- the root splits 600 ways.  levels = 2: 12 blocks of 40 groups, chained by
    1.0 inside a block and by 2.0 between blocks -- 12 parents born at 2.0, whose 480 children
    are all born at 1.0 with interleaved smallest members"""
    G = 600 if levels == 1 else 480
    g = np.arange(G)
    va, vb, w = [2 * g], [2 * g + 1], [np.full(G, 0.5)]
    link = g[:-1]
    heavy = np.zeros(G - 1, bool) if levels == 1 else (link % 40 == 39)
    va.append(2 * link + 1), vb.append(2 * (link + 1)), w.append(np.where(heavy, 2.0, 1.0))
    perm = rng.permutation(2 * G)
    return perm[np.concatenate(va)].astype(np.int32), perm[np.concatenate(vb)].astype(np.int32), np.concatenate(w), 2 * G


@pytest.mark.parametrize("levels", [1, 2])
def test_many_clusters_born_at_one_level(pkg, ctx, levels):
    """K = 601 (one level) or 493 (two levels): across 256 and 512; equal births are numbered by
    smallest member, whatever their parents are"""
    va, vb, w, n = pair_groups(np.random.default_rng(levels), levels)
    t = dev_tree(pkg, ctx, va, vb, w, n, 2).host()
    same_tree(t, cluster_tree_reference(va, vb, w, n, 2), levels)
    assert t.n_tree == (601 if levels == 1 else 1 + 12 + 480)
    first = 1 if levels == 1 else 13
    assert np.all(t.birth[first:] == 1.0) and np.all(np.diff(t.min_id[first:]) > 0)
    if levels == 2:
        assert np.all(t.birth[1:13] == 2.0) and np.all(np.diff(t.min_id[1:13]) > 0)
        assert len(set(t.parent[13:].tolist())) == 12 and np.any(np.diff(t.parent[13:]) < 0)  # parents interleave


def test_deep_cluster_tree_and_cuts(pkg, ctx):
    """3,001 pairs chained by bridges of weight 10 + i, one straggler per pair (the GLOSH tests'
    deep shape): every bridge is a true split, the cluster tree is about 3,000 deep and most
    stragglers sit thousands of parents below the clusters a high cut names.  65 levels (two
    LDS chunks of the cut kernel): every 97th birth level exactly, levels between, the ends"""
    P = 3001
    i = np.arange(P)
    va = np.r_[2 * i, 2 * i[:-1] + 1, 2 * i].astype(np.int32)
    vb = np.r_[2 * i + 1, 2 * i[1:], 2 * P + i].astype(np.int32)
    w = np.r_[1e-3 * (i + 1), 10.0 + i[:-1], 9.5 + i]
    n = 3 * P
    want = pkg.cluster_tree(va, vb, w, n, 2)
    t = dev_tree(pkg, ctx, va, vb, w, n, 2)
    same_tree(t.host(), want, "deep")
    depth, c = 0, int(want.point_cluster[0])
    while c:
        depth, c = depth + 1, int(want.parent[c - 1])
    assert depth > 2990
    births = np.unique(want.birth[1:])[::-1]
    lv = np.r_[births[::97], (births[5::97] + 0.25)[:28], 9.75, 1e-3, 2.5e-3, np.inf, -np.inf, 0.0]
    assert lv.shape[0] == 65
    rows = dev_cuts(pkg, ctx, t, lv)
    assert np.array_equal(rows, pkg.labels_at_levels(want, lv))
    # by hand: at the weight of the bridge between pairs j and j + 1, point 0 carries the label of
    # the cluster born (one bridge higher) with pairs 0..j + 1 and their stragglers
    k = int(np.flatnonzero(lv == births[97])[0])
    j = int(births[97] - 10)
    inner = rows[k][0]
    assert want.size[inner - 1] == 3 * (j + 2) and rows[k][2 * (j + 1)] == inner and rows[k][2 * (j + 2)] != inner


@pytest.mark.parametrize("n", [257, 100003])
def test_other_sizes_and_mixed_memory(pkg, ctx, n):
    """sizes that are no multiple of the workgroup; L = 1; host levels with a device tree, device
    levels with a host tree (staged), one array of the tree on the other side"""
    va, vb, w = big_tree(n, 30, 5)
    want = pkg.cluster_tree(va, vb, w, n, 3)
    t = dev_tree(pkg, ctx, va, vb, w, n, 3)
    same_tree(t.host(), want, n)
    staged = pkg.cluster_tree(va, vb, w, n, 3, ctx=ctx)  # host arrays + ctx: the device algorithm
    assert isinstance(staged.parent, np.ndarray)
    same_tree(staged, want, (n, "staged"))
    lv = np.array([float(np.median(want.birth[1:]))])
    ref = pkg.labels_at_levels(want, lv)
    assert ref.shape == (1, n) and ref.min() == 0 and ref.max() > 1
    a = pkg.labels_at_levels(t, lv, ctx=ctx)  # device tree, host levels
    assert torch.is_tensor(a) and np.array_equal(a.cpu().numpy(), ref)
    b = pkg.labels_at_levels(want, cuda(lv, np.float64), ctx=ctx)  # host tree, device levels
    assert isinstance(b, np.ndarray) and np.array_equal(b, ref)
    mixed = t.host()
    mixed.birth, mixed.point_cluster = t.birth, t.point_cluster
    assert np.array_equal(pkg.labels_at_levels(mixed, lv, ctx=ctx).cpu().numpy(), ref)
    assert np.array_equal(t.flat_labels().cpu().numpy(), pkg.flat_labels(va, vb, w, n, 3)[0])


def test_single_cluster_and_capacity(pkg, ctx):
    z = np.zeros(0, np.int32)
    t = dev_tree(pkg, ctx, z, z, np.zeros(0), 1, 4).host()  # n = 1
    same_tree(t, pkg.cluster_tree(z, z, np.zeros(0), 1, 4), "n = 1")
    assert dev_cuts(pkg, ctx, dev_tree(pkg, ctx, z, z, np.zeros(0), 1, 4), [-1.0, 0.0]).tolist() == [[0], [1]]
    va, vb, w = np.arange(39, dtype=np.int32), np.arange(1, 40, dtype=np.int32), 1.0 + np.arange(39) / 7.0
    t = dev_tree(pkg, ctx, va, vb, w, 40, 64)  # n < minClSize: K = 1, all leave at the heaviest weight
    same_tree(t.host(), pkg.cluster_tree(va, vb, w, 40, 64), "K = 1")
    assert t.n_tree == 1 and np.all(t.point_level.cpu().numpy() == w[-1])
    assert dev_cuts(pkg, ctx, t, [w[-1], w[-2]]).tolist() == [[1] * 40, [0] * 40]
    assert dev_tree(pkg, ctx, z, z, np.zeros(0), 0, 2).n_tree == 0
    # cap < K: the status, K, and nothing written
    d = [cuda(K_VA, np.int32), cuda(K_VB, np.int32), cuda(K_W, np.float64)]
    par = torch.full((8,), -7, dtype=torch.int32, device="cuda")
    kt = np.full(1, -1, np.int64)
    p = lambda x: C.c_void_p(x.data_ptr())
    L = pkg.lib()
    rc = L.hdb_flat_cluster_tree(ctx.h, p(d[0]), p(d[1]), p(d[2]), 7, 8, 2, 4, kt.ctypes.data, p(par), *[None] * 9)
    msg = L.hdb_last_error().decode()
    assert rc == -1 and kt[0] == 5 and "4" in msg and "5" in msg and par.cpu().tolist() == [-7] * 8
    rc = L.hdb_flat_cluster_tree(ctx.h, p(d[0]), p(d[1]), p(d[2]), 7, 8, 2, 5, kt.ctypes.data, p(par), *[None] * 9)
    assert rc == 0 and kt[0] == 5 and par.cpu().tolist() == [0, 1, 1, 3, 3, -7, -7, -7]  # the other outputs NULL


def test_bad_trees_and_levels_give_a_status(pkg, ctx):
    """the cut kernel bound-checks what it is given: a status, nothing read out of range"""
    good = dev_tree(pkg, ctx, K_VA, K_VB, K_W, 8, 2)
    for field, bad in [("point_cluster", [2, 2, 2, 4, 4, 4, 5, 6]), ("point_cluster", [2, 2, 2, 4, 0, 4, 5, 5]),
                       ("point_cluster", [2, 2, 2, -4, 4, 4, 5, 5]), ("parent", [0, 1, 1, 4, 3]),
                       ("parent", [0, 1, 1, 3, 2 ** 31 - 1]), ("parent", [2, 1, 1, 3, 3]), ("parent", [0, 1, -1, 3, 3])]:
        t = dev_tree(pkg, ctx, K_VA, K_VB, K_W, 8, 2)
        setattr(t, field, cuda(bad, np.int32))
        with pytest.raises(pkg.HdbError, match="out of range") as ei:
            pkg.labels_at_levels(t, [2.0], ctx=ctx)
        assert ei.value.code == -1
    with pytest.raises(pkg.HdbError, match="NaN level"):
        dev_cuts(pkg, ctx, good, [1.0, float("nan")])
    assert dev_cuts(pkg, ctx, good, []).shape == (0, 8)
    assert dev_cuts(pkg, ctx, good, [4.0, 4.0, 0.75]).tolist() == [[2, 2, 2, 3, 3, 3, 3, 3]] * 2 + [[0] * 6 + [5, 5]]
    with pytest.raises(pkg.HdbError):  # the errors of flat_labels
        dev_tree(pkg, ctx, K_VA[:-1], K_VB[:-1], K_W[:-1], 8, 2)


def test_existing_calls_unchanged_after_a_tree_call(pkg, ctx):
    n, mcs = 3000, 4
    va, vb, w = big_tree(n, 20, 3)
    d = [cuda(va, np.int32), cuda(vb, np.int32), cuda(w, np.float64)]
    lab0, k0 = pkg.flat_labels(*d, n, mcs, ctx=ctx)
    s0, e0 = pkg.outlier_scores(*d, n, mcs, ctx=ctx)
    t = pkg.cluster_tree(*d, n, mcs, ctx=ctx)
    pkg.labels_at_levels(t, [0.5, 1.5], ctx=ctx)
    lab1, k1 = pkg.flat_labels(*d, n, mcs, ctx=ctx)
    s1, e1 = pkg.outlier_scores(*d, n, mcs, ctx=ctx)
    assert k0 == k1 == t.n_clusters and torch.equal(lab0, lab1) and torch.equal(t.flat_labels(), lab0)
    assert np.array_equal(bits(s0.cpu().numpy()), bits(s1.cpu().numpy()))
    assert np.array_equal(bits(e0.cpu().numpy()), bits(e1.cpu().numpy()))
    assert np.array_equal(bits(t.point_level.cpu().numpy()), bits(e0.cpu().numpy()))
    assert np.array_equal(bits(t.outlier_scores().cpu().numpy()), bits(s0.cpu().numpy()))


def test_driver_cluster_tree(pkg):
    """MRHDBSCANStar(cluster_tree=True): one hierarchy call; labels, count and scores as without
    it, the tree that of the host path on the returned edges"""
    X = blobs(3000, 3, 6, 1)
    kw = dict(minPts=4, minClSize=4, processing_units=300, k=0.1)
    base = pkg.MRHDBSCANStar(outlier_scores=True, **kw).run(X)
    got = pkg.MRHDBSCANStar(cluster_tree=True, outlier_scores=True, **kw).run(X)
    assert "cluster_tree" not in base
    assert got["n_clusters"] == base["n_clusters"] and torch.equal(got["labels"], base["labels"])
    for key in ("outlier_scores", "noise_levels"):
        assert np.array_equal(bits(got[key].cpu().numpy()), bits(base[key].cpu().numpy())), key
    va, vb, w = (x.cpu().numpy() for x in got["edges"])
    same_tree(got["cluster_tree"].host(), pkg.cluster_tree(va, vb, w, X.shape[0], 4), "driver")
    only = pkg.MRHDBSCANStar(cluster_tree=True, **kw).run(X)
    assert "outlier_scores" not in only and torch.equal(only["labels"], base["labels"])
