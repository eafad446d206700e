"""K6's alpha-edge contraction (csrc/flat.hip section 2b) against the host algorithm, bit for
bit: labels and cluster count on every shape, outlier scores and the cluster tree (which read
|C(e)| and the smallest id of every edge) on the hub trees, the second comb and a real MST.
Every tree has at least 2^18 edges, above any value the dispatch constant may take, and every
case asserts that the contraction ran."""
import numpy as np
import pytest
import torch

from conftest import blobs
from path_helpers import bits_eq
from test_flat_labels import lib_flat

pytestmark = pytest.mark.gpu

N = (1 << 18) + 1000
MCS = (2, 5)


@pytest.fixture(scope="module")
def ctx(pkg):
    return pkg.Context.get(0)


def permuted(va, vb, w, n, seed):
    perm = np.random.default_rng(seed).permutation(n).astype(np.int32)
    return perm[np.asarray(va)], perm[np.asarray(vb)], np.asarray(w, np.float64), n


def path(equal):
    w = np.ones(N - 1) if equal else np.arange(N - 1, dtype=np.float64)
    return permuted(np.arange(N - 1), np.arange(1, N), w, N, 1)


def hub(wmax, spoil=None):
    """the random hub trees of test_gpu_flat.py: every edge tied, heavy ties, continuous.  spoil:
    the edge of the last vertex (a leaf) becomes a copy of the first edge ("duplicate"), or joins
    vertex 0 to the first vertex that is no child of it ("cycle": the tree's path between them
    closes one); either way n - 1 edges remain"""
    rng = np.random.default_rng(N + (0 if wmax is None else wmax + 1))
    par = np.where(rng.random(N - 1) < 0.3, 0, (rng.random(N - 1) * np.arange(1, N)).astype(np.int64))
    child = np.arange(1, N)
    w = rng.random(N - 1) if wmax is None else rng.integers(0, wmax + 1, N - 1).astype(np.float64)
    if spoil == "duplicate":
        par[-1], child[-1] = par[0], child[0]
    elif spoil == "cycle":
        par[-1], child[-1] = 0, child[np.flatnonzero(par != 0)[0]]
    return permuted(par, child, w, N, 2)


def comb(single):
    """teeth of 5 points on a spine of rising weights.  single: a single point sits on the spine
    between consecutive teeth, and two leaves of every tooth are looser than the spine edge that
    reaches the tooth: together the chain above every alpha edge (the spine edge into the next
    tooth) has three edges, each adding one point"""
    rng = np.random.default_rng(5 + single)
    unit = 6 if single else 5
    teeth = -(-N // unit)
    base = np.arange(teeth, dtype=np.int64) * unit
    ta = np.repeat(base, 4)
    tb = (base[:, None] + np.arange(1, 5)[None, :]).ravel()
    tw = rng.random((teeth, 4)) * 0.5
    i = np.arange(teeth - 1, dtype=np.float64)
    if not single:
        va, vb = np.r_[ta, base[:-1]], np.r_[tb, base[1:]]
        w = np.r_[tw.ravel(), 1.0 + i]
        return (*permuted(va, vb, w, teeth * unit, 3), teeth - 1)
    tw[1:, 2:] = 3.0 * np.arange(1, teeth)[:, None] + np.array([0.3, 0.6])[None, :]  # after the edge into the tooth
    s = base[:-1] + 5
    va, vb = np.r_[ta, base[:-1], s], np.r_[tb, s, base[1:]]
    w = np.r_[tw.ravel(), 3.0 * i + 1.0, 3.0 * i + 2.0]
    return (*permuted(va, vb, w, teeth * unit - 1, 4), teeth - 1)


def binary_tree():
    """complete binary tree, weights rising toward the root and random within a level"""
    rng = np.random.default_rng(6)
    child = np.arange(2, N + 1, dtype=np.int64)  # heap numbering from 1
    depth = np.floor(np.log2(child)).astype(np.int64)
    w = (depth.max() - depth) + rng.random(N - 1)
    return permuted(child // 2 - 1, child - 1, w, N, 7)


def descending(va, vb, w):
    d = np.argsort(-w, kind="stable")
    return va[d], vb[d], w[d]


def orders(va, vb, w):
    """merged order (descending, stable: the presorted branch), ascending, shuffled (radix sort)"""
    a = np.argsort(w, kind="stable")
    p = np.random.default_rng(8).permutation(w.shape[0])
    return [descending(va, vb, w), (va[a], vb[a], w[a]), (va[p], vb[p], w[p])]


def alpha_count(va, vb, n):
    """alpha edges of a list in rank order: edges that are the lightest at neither end"""
    m = va.shape[0]
    mp = np.full(n, m, np.int64)
    r = np.arange(m)
    np.minimum.at(mp, va, r)
    np.minimum.at(mp, vb, r)
    return int(np.count_nonzero((mp[va] != r) & (mp[vb] != r)))


def dev(t):
    return [torch.from_numpy(np.ascontiguousarray(x)).cuda() for x in t]


def check_labels(pkg, ctx, edge_lists, n, alpha=None):
    """every list is the same tree; returns the alpha count the device reports"""
    m = n - 1
    assert m >= 1 << 18
    got_alpha = None
    for mcs in MCS:
        ref, kr = lib_flat(pkg, *edge_lists[0], n, mcs)
        for i, el in enumerate(edge_lists):
            lab, k = pkg.flat_labels(*dev(el), n, mcs, ctx=ctx)
            assert ctx.get_stat("flat_contract") == 1
            got_alpha = ctx.get_stat("flat_alpha_edges")
            print(f"n={n} mcs={mcs} order={i}: alpha edges {got_alpha} of {m}, K={k}")
            assert 2 * got_alpha < m
            if alpha is not None and i == 0:
                assert got_alpha == alpha
            assert k == kr and np.array_equal(lab.cpu().numpy(), ref), (mcs, i)
    return got_alpha


def check_scores_and_tree(pkg, ctx, va, vb, w, n):
    for mcs in MCS:
        want = pkg.outlier_scores(va, vb, w, n, mcs, with_labels=True)
        got = pkg.outlier_scores(*dev((va, vb, w)), n, mcs, ctx=ctx, with_labels=True)
        assert ctx.get_stat("flat_contract") == 1
        assert bits_eq(got[0].cpu().numpy(), want[0]) and bits_eq(got[1].cpu().numpy(), want[1]), mcs
        assert np.array_equal(got[2].cpu().numpy(), want[2]) and got[3] == want[3], mcs
        tw = pkg.cluster_tree(va, vb, w, n, mcs)
        tg = pkg.cluster_tree(*dev((va, vb, w)), n, mcs, ctx=ctx)
        assert ctx.get_stat("flat_contract") == 1
        assert tg.n_clusters == tw.n_clusters
        for f in tw.FIELDS:
            a, b = getattr(tg, f).cpu().numpy(), getattr(tw, f)
            assert bits_eq(a, b) if b.dtype == np.float64 else np.array_equal(a, b), (mcs, f)


@pytest.mark.parametrize("equal", [False, True])
def test_paths_have_no_alpha_edge(pkg, ctx, equal):
    """one super-vertex, one bottom chain; with every weight equal the ranks are positions alone"""
    va, vb, w, n = path(equal)
    check_labels(pkg, ctx, [descending(va, vb, w)], n, alpha=0)


@pytest.mark.parametrize("wmax", [0, 3, None])
def test_hub_trees(pkg, ctx, wmax):
    va, vb, w, n = hub(wmax)
    check_labels(pkg, ctx, orders(va, vb, w), n)
    check_scores_and_tree(pkg, ctx, *descending(va, vb, w), n)


def test_hub_tree_point_order_vertex_labels(pkg, ctx):
    """flat_relabel = 0: the super-vertices are numbered by their root's smaller point id, not by
    its rank"""
    va, vb, w, n = hub(None)
    ctx.set_option("flat_relabel", 0)
    try:
        check_labels(pkg, ctx, orders(va, vb, w)[::2], n)
        check_scores_and_tree(pkg, ctx, *descending(va, vb, w), n)
    finally:
        ctx.set_option("flat_relabel", 1)


def test_comb_spine_is_the_alpha_tree(pkg, ctx):
    """every spine edge is alpha: the alpha dendrogram is a caterpillar as tall as the spine, the
    lifting search of the tooth edges above it runs deep"""
    va, vb, w, n, spine = comb(False)
    d = descending(va, vb, w)
    assert alpha_count(d[0][::-1], d[1][::-1], n) == spine
    check_labels(pkg, ctx, orders(va, vb, w), n, alpha=spine)


def test_comb_with_chains_above_alpha_edges(pkg, ctx):
    va, vb, w, n, spine = comb(True)
    d = descending(va, vb, w)
    assert alpha_count(d[0][::-1], d[1][::-1], n) == spine
    check_labels(pkg, ctx, orders(va, vb, w), n, alpha=spine)
    check_scores_and_tree(pkg, ctx, *d, n)


def test_binary_tree_many_alpha_edges(pkg, ctx):
    va, vb, w, n = binary_tree()
    d = descending(va, vb, w)
    # an inner node's heavier child edge is alpha unless the child is a leaf: a quarter of the edges
    check_labels(pkg, ctx, [d], n, alpha=alpha_count(d[0][::-1], d[1][::-1], n))


def test_exact_mst_with_ties(pkg, ctx):
    X = np.round(blobs(300_000, 3, 12, 5), 1)
    _, g = pkg.HDBSCANStar(ctx).exactMST(torch.from_numpy(X).cuda(), 4, None, 2, selfEdges=True)
    va, vb, w = pkg.sort_edges_desc(g.getVerticeA(), g.getVericeB(), g.getEges(), ctx)
    el = tuple(t.cpu().numpy() for t in (va, vb, w))
    check_labels(pkg, ctx, [el], X.shape[0])
    check_scores_and_tree(pkg, ctx, *el, X.shape[0])


@pytest.mark.parametrize("how", ["duplicate", "cycle"])
def test_malformed_input_raises_and_context_recovers(pkg, ctx, how):
    va, vb, w, n = hub(None)
    va, vb, w = descending(va, vb, w)
    ref, kr = lib_flat(pkg, va, vb, w, n, 5)
    ba, bb, bw, _ = hub(None, spoil=how)
    ba, bb, bw = descending(ba, bb, bw)
    with pytest.raises(pkg.HdbError):
        pkg.flat_labels(*dev((ba, bb, bw)), n, 5, ctx=ctx)
    lab, k = pkg.flat_labels(*dev((va, vb, w)), n, 5, ctx=ctx)
    assert ctx.get_stat("flat_contract") == 1
    assert k == kr and np.array_equal(lab.cpu().numpy(), ref)
