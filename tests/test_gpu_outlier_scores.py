"""GLOSH outlier scores on the device (csrc/flat.hip section 6) against the test-side reference
(tests/glosh_reference.py) and the host path (csrc/flat.cpp): the same bits in scores and noise
levels -- the arithmetic is an exact min, one division and one subtraction -- and the labels
of flat_labels, on shapes that cross every path of K6 and of the new passes (pointer jumping
over chains of invalid nodes, a cluster tree thousands deep, a root that never splits)."""
import numpy as np
import pytest
import torch

from conftest import blobs
from glosh_reference import glosh_reference
from test_outlier_scores import DBL_MAX, KNOWN, bits, edges_of, random_tree

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ctx(pkg):
    return pkg.Context.get(0)


def dev_scores(pkg, ctx, va, vb, w, n, mcs, with_labels=False):
    """device-resident inputs; results as numpy"""
    t = (torch.from_numpy(np.ascontiguousarray(va, np.int32)).cuda(), torch.from_numpy(np.ascontiguousarray(vb, np.int32)).cuda(),
         torch.from_numpy(np.ascontiguousarray(w, np.float64)).cuda())
    out = pkg.outlier_scores(*t, n, mcs, ctx=ctx, with_labels=with_labels)
    return tuple(x.cpu().numpy() if torch.is_tensor(x) else x for x in out)


def assert_same(got, want, what):
    for g, r, name in zip(got[:2], want[:2], ("scores", "noise levels")):
        assert np.array_equal(bits(g), bits(r)), (what, name, int((bits(g) != bits(r)).sum()))


def big_tree(n, values, seed):
    """random recursive tree; weights continuous (values None) or from `values` distinct values"""
    rng = np.random.default_rng(seed)
    va = (rng.random(n - 1) * np.arange(1, n)).astype(np.int64)
    vb = np.arange(1, n, dtype=np.int64)
    w = rng.random(n - 1) if values is None else rng.integers(0, values, n - 1) / 8.0
    perm = rng.permutation(n)
    return perm[va].astype(np.int32), perm[vb].astype(np.int32), w


@pytest.fixture(scope="module")
def ref2000():
    """the O(levels x n) reference, once per tree and minClSize"""
    out = {}
    for ties in (False, True):
        va, vb, w = big_tree(2000, 6 if ties else None, 7 + ties)
        out[ties] = (va, vb, w, {mcs: glosh_reference(va, vb, w, 2000, mcs) for mcs in (2, 5)})
    return out


@pytest.mark.parametrize("ties", [False, True])
@pytest.mark.parametrize("mcs", [2, 5])
def test_device_equals_reference(pkg, ctx, ref2000, ties, mcs):
    va, vb, w, ref = ref2000[ties]
    assert_same(dev_scores(pkg, ctx, va, vb, w, 2000, mcs), ref[mcs], (ties, mcs))


@pytest.fixture(scope="module")
def host20k(pkg):
    out = {}
    for values in (None, 50):
        va, vb, w = big_tree(20000, values, 11)
        out[values] = (va, vb, w, {mcs: pkg.outlier_scores(va, vb, w, 20000, mcs, with_labels=True) for mcs in (2, 5)})
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
            got = dev_scores(pkg, ctx, va, vb, w, 20000, mcs, with_labels=True)
            assert_same(got, ref[mcs], (values, relabel, mid, mcs))
            assert got[3] == ref[mcs][3] and np.array_equal(got[2], ref[mcs][2])
        assert ctx.get_stat("flat_global_depths") >= (1 if mid else 4)
    finally:
        ctx.set_option("flat_relabel", 1)
        ctx.set_option("flat_mid_log", 12)


@pytest.mark.parametrize("opts", [dict(ssort=0), dict(flat_block_log=8), dict(flat_block_log=9, ssort=0)])
def test_device_equals_host_other_sort_and_block_paths(pkg, ctx, host20k, opts):
    """the rocPRIM sort of the stability terms and the smaller LDS blocks leave the scratch the
    score passes reuse in the same state"""
    from path_helpers import options
    va, vb, w, ref = host20k[50]
    with options(ctx, **opts):
        got = dev_scores(pkg, ctx, va, vb, w, 20000, 5, with_labels=True)
    assert_same(got, ref[5], opts)
    assert got[3] == ref[5][3] and np.array_equal(got[2], ref[5][2])


@pytest.mark.parametrize("stragglers", [False, True])
def test_device_deep_cluster_tree(pkg, ctx, stragglers):
    """5,000 pairs (intra-pair weight 1e-3 (i + 1)) chained by bridges of weight 10 + i,
    minClSize 2: every bridge is a true split, so the cluster tree is a chain about 5,000 deep.
    In that shape every point leaves from a leaf cluster, whose eps_max is its own level; with
    `stragglers` one more point hangs off pair i at weight 9.5 + i and leaves from the inner
    cluster {pairs 0..i}, whose eps_max = 1e-3 comes from pair 0, i clusters below it -- a fixed
    number of parent hops, or a doubling bounded too low, gives another value there"""
    P = 5000
    i = np.arange(P)
    va = np.r_[2 * i, 2 * i[:-1] + 1].astype(np.int32)
    vb = np.r_[2 * i + 1, 2 * i[1:]].astype(np.int32)
    w = np.r_[1e-3 * (i + 1), 10.0 + i[:-1]]
    n = 2 * P
    if stragglers:
        va, vb, w = np.r_[va, 2 * i].astype(np.int32), np.r_[vb, 2 * P + i].astype(np.int32), np.r_[w, 9.5 + i]
        n = 3 * P
    want = pkg.outlier_scores(va, vb, w, n, 2)
    if stragglers:
        assert np.array_equal(want[1][2 * P:], 9.5 + i) and np.array_equal(want[0][2 * P:], 1.0 - 1e-3 / (9.5 + i))
    assert_same(dev_scores(pkg, ctx, va, vb, w, n, 2), want, "deep")


@pytest.mark.parametrize("n", [4096, 40])
def test_device_long_noise_chains(pkg, ctx, n):
    """a path with strictly ascending weights, minClSize 64: points climb up to 63 invalid nodes
    to their first valid ancestor; n = 40 < minClSize: every point leaves at the root's level"""
    va, vb = np.arange(n - 1, dtype=np.int32), np.arange(1, n, dtype=np.int32)
    w = 1.0 + np.arange(n - 1) / 7.0
    want = pkg.outlier_scores(va, vb, w, n, 64)
    if n < 64:
        assert np.array_equal(want[1], np.full(n, w[-1])) and (want[0] < -1e300).all()
    assert_same(dev_scores(pkg, ctx, va, vb, w, n, 64), want, n)


@pytest.mark.parametrize("case", [1, 2])
def test_device_root_rules_known_answers(pkg, ctx, case):
    """case 2: eps_max(root) from the descendants only; case 3: the root never splits (DBL_MAX)"""
    _, n, mcs, eps, scores = KNOWN[case]
    got = dev_scores(pkg, ctx, *edges_of(KNOWN[case]), n, mcs)
    assert_same(got, (np.array(scores, np.float64), np.array(eps, np.float64)), case)
    if case == 2:
        assert got[0][3] == 1 - DBL_MAX / 3


def test_device_edge_sizes(pkg, ctx):
    z = np.zeros(0, np.int32)
    s, e, lab, k = dev_scores(pkg, ctx, z, z, np.zeros(0), 1, 4, with_labels=True)
    assert s.tolist() == [0.0] and e.tolist() == [0.0] and lab.tolist() == [0] and k == 0
    a, b, w = np.array([0], np.int32), np.array([1], np.int32), np.array([0.5])
    want = pkg.outlier_scores(a, b, w, 2, 2, with_labels=True)
    got = dev_scores(pkg, ctx, a, b, w, 2, 2, with_labels=True)
    assert_same(got, want, "n = 2")
    assert got[3] == want[3] and np.array_equal(got[2], want[2])
    assert want[1].tolist() == [0.5, 0.5]


def test_device_inputs_and_optional_outputs(pkg, ctx):
    """device tensors and host arrays staged through a context give the same bits; the optional
    outputs may be NULL; labels and K are flat_labels's"""
    import ctypes as C
    n, mcs = 3000, 4
    va, vb, w = big_tree(n, 20, 3)
    dev = dev_scores(pkg, ctx, va, vb, w, n, mcs, with_labels=True)
    staged = pkg.outlier_scores(va, vb, w, n, mcs, ctx=ctx, with_labels=True)  # host arrays + ctx: device algorithm
    host = pkg.outlier_scores(va, vb, w, n, mcs, with_labels=True)
    lab, k = pkg.flat_labels(va, vb, w, n, mcs, ctx=ctx)
    for got in (dev, staged):
        assert_same(got, host, "inputs")
        assert got[3] == k and np.array_equal(got[2], lab)
    L = pkg.lib()
    t = [torch.from_numpy(x).cuda() for x in (va, vb, w)]
    s = torch.empty(n, dtype=torch.float64, device="cuda")
    e = torch.empty(n, dtype=torch.float64, device="cuda")
    p = lambda x: C.c_void_p(x.data_ptr())
    pkg._capi.check(L.hdb_flat_outlier_scores(ctx.h, p(t[0]), p(t[1]), p(t[2]), n - 1, n, mcs, p(s), None, None, None), "scores only")
    assert np.array_equal(bits(s.cpu().numpy()), bits(host[0]))
    s.zero_()
    pkg._capi.check(L.hdb_flat_outlier_scores(ctx.h, p(t[0]), p(t[1]), p(t[2]), n - 1, n, mcs, p(s), p(e), None, None), "no labels")
    assert np.array_equal(bits(s.cpu().numpy()), bits(host[0])) and np.array_equal(bits(e.cpu().numpy()), bits(host[1]))
    with pytest.raises(pkg.HdbError):  # the errors of flat_labels
        dev_scores(pkg, ctx, va[:-1], vb[:-1], w[:-1], n, mcs)


def test_driver_outlier_scores(pkg):
    """MRHDBSCANStar(outlier_scores=True): one combined call; labels and edges as without it,
    the scores those of the host path on the returned edges"""
    X = blobs(3000, 3, 6, 1)
    kw = dict(minPts=4, minClSize=4, processing_units=300, k=0.1)
    base = pkg.MRHDBSCANStar(**kw).run(X)
    got = pkg.MRHDBSCANStar(outlier_scores=True, **kw).run(X)
    assert "outlier_scores" not in base and "noise_levels" not in base
    assert got["n_clusters"] == base["n_clusters"]
    assert np.array_equal(got["labels"].cpu().numpy(), base["labels"].cpu().numpy())
    for x, y in zip(got["edges"], base["edges"]):
        assert np.array_equal(bits(x.cpu().numpy()) if x.dtype == torch.float64 else x.cpu().numpy(),
                              bits(y.cpu().numpy()) if y.dtype == torch.float64 else y.cpu().numpy())
    va, vb, w = (x.cpu().numpy() for x in got["edges"])
    want = pkg.outlier_scores(va, vb, w, X.shape[0], 4)
    assert_same((got["outlier_scores"].cpu().numpy(), got["noise_levels"].cpu().numpy()), want, "driver")
