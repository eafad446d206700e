"""The exact leaf (hdb_exact_mst / hdb_mst_boruvka: K1t and the K2b Boruvka over the Morton/BVH
index) on the inputs of tests/degenerate_inputs.py, where its three arguments are thinnest: box
lower bounds under underflow and overflow, the strict total edge order (w, s, lo, hi) when every
edge ties, a Morton quantisation whose span is 0, overflows or is infinite.  Everything is
compared bit for bit -- cores with the oracle, every MST edge with an independent Kruskal
(path_helpers.kruskal_mst), the merged order with sort_edges_desc, the device hierarchy with the
host's, the reference Prim with the oracle's -- and every case asserts through launch counts that
K1t and K2b ran.  Also: the non-finite contract of include/hdbmi.h (NaN pairs are no edges, +inf
weights are edges under the same tie rule, rows that only NaN pairs reach are HDB_EINVAL
"non-finite input"), -0.0 cores, and the BVH level boundaries."""
import functools

import numpy as np
import pytest
import torch

from conftest import blobs
from degenerate_inputs import MST_SETTINGS, NOT_SPANNING, SPANNING, SPANNING_FINITE, family, family_case
from path_helpers import bits_eq, edge_set, kruskal_mst, options, spanning_tree

pytestmark = pytest.mark.gpu

DBL_MAX = np.finfo(np.float64).max


@pytest.fixture(scope="module")
def ctx(pkg):
    c = pkg.Context(0)  # private: no option set here can leak into another module's context
    c.use_torch_stream()
    c.set_timing(True)  # launch counts
    return c


@pytest.fixture(scope="module")
def star(pkg, ctx):
    return pkg.HDBSCANStar(ctx)


def launches(ctx, *names):
    """launch counts of the named kernels since the last call"""
    return tuple(ctx.kernel_time(k, reset=True)[1] for k in names)


# ------------------------------------------------------------------------------------ cores
@pytest.mark.parametrize("mp", [2, 4])
@pytest.mark.parametrize("name", SPANNING)
def test_cores_every_semantics_tree_and_dense(ctx, star, oracle, name, mp):
    X, _ = family(name)
    launches(ctx, "knn_tree")
    for sem in range(3):
        ref = oracle.core_distances(X, mp, semantics=sem)
        with options(ctx, knn_tree=1, knn_tree_min_n=0):
            got = star.calculateCoreDistances(X, mp, None, sem)
        assert launches(ctx, "knn_tree") == (1,), (name, sem)
        assert bits_eq(got, ref), (name, mp, sem, "K1t")
        for screen in (1, 0):
            with options(ctx, knn_tree=0, knn_fp32_screen=screen):
                got = star.calculateCoreDistances(X, mp, None, sem)
            assert launches(ctx, "knn_tree") == (0,), (name, sem)
            assert bits_eq(got, ref), (name, mp, sem, "K1 screen %d" % screen)


# ----------------------------------------------------------------------- exact MST vs Kruskal
K2B_OPTIONS = [dict(), dict(boruvka_knn_seed=0), dict(boruvka_seed=0, boruvka_adj_seed=0), dict(trav_pop_test=3),
               dict(boruvka_wave_pts=16)]


def check_edges(what, va, vb, gw, n, ref):
    assert spanning_tree(va, vb, n)
    got, want = edge_set(va, vb, gw), edge_set(*ref)
    assert got == want, (what, len(got - want), sorted(got - want)[:3], sorted(want - got)[:3])


@pytest.mark.parametrize("kw", K2B_OPTIONS, ids=lambda kw: "-".join(f"{k}{v}" for k, v in kw.items()) or "defaults")
@pytest.mark.parametrize("mp,sem", MST_SETTINGS)
@pytest.mark.parametrize("name", SPANNING)
def test_exact_mst_edges_equal_kruskal(ctx, star, name, mp, sem, kw):
    X, core, ref = family_case(name, mp, sem)
    launches(ctx, "knn_tree", "boruvka_r0")
    inf0 = ctx.get_stat("boruvka_inf_edges")
    with options(ctx, **kw):
        c, g = star.exactMST(X, mp, None, sem, selfEdges=False)
    ran = launches(ctx, "knn_tree", "boruvka_r0")
    print(f"{name} mp={mp} {kw}: knn_tree x{ran[0]}, boruvka_r0 x{ran[1]}, "
          f"inf edges {ctx.get_stat('boruvka_inf_edges') - inf0}")
    assert ran == (1, 1)  # the fused leaf: K1t and K2b, no fallback
    assert bits_eq(c, core), (name, mp, kw)
    check_edges((name, mp, kw), g.getVerticeA(), g.getVericeB(), g.getEges(), X.shape[0], ref)
    assert ctx.get_stat("boruvka_inf_edges") - inf0 == int(np.isinf(ref[2]).sum())


@pytest.mark.parametrize("mp,sem", MST_SETTINGS)
@pytest.mark.parametrize("name", SPANNING)
def test_boruvka_on_oracle_cores_equals_kruskal(ctx, star, name, mp, sem):
    X, core, ref = family_case(name, mp, sem)
    launches(ctx, "boruvka_r0")
    g = star.constructMSTBoruvka(X, core, False)
    assert launches(ctx, "boruvka_r0") == (1,)
    check_edges((name, mp), g.getVerticeA(), g.getVericeB(), g.getEges(), X.shape[0], ref)


# ------------------------------------------------------------------------------ merged order
@pytest.mark.parametrize("ssort", [1, 0])
@pytest.mark.parametrize("name", SPANNING)
def test_merged_order_equals_sort_edges_desc(pkg, ctx, star, name, ssort):
    """all-equal, all-zero and all-+inf weights through both sorts of the edge list"""
    X, _ = family(name)
    for self_edges in (False, True):
        with options(ctx, ssort=ssort):
            _, p = star.exactMST(X, 4, None, 0, selfEdges=self_edges)
            _, m = star.exactMST(X, 4, None, 0, selfEdges=self_edges, merged=True)
        va, vb, w = pkg.sort_edges_desc(p.getVerticeA().copy(), p.getVericeB().copy(), p.getEges().copy(), ctx)
        what = (name, ssort, self_edges)
        assert np.array_equal(m.getVerticeA(), va) and np.array_equal(m.getVericeB(), vb), what
        assert bits_eq(m.getEges(), w) and not np.isnan(w).any(), what


# -------------------------------------------------------------------------------- downstream
@pytest.mark.parametrize("name", SPANNING_FINITE)
def test_downstream_device_equals_host(pkg, ctx, star, name):
    """flat labels, GLOSH scores and noise levels over the merged tree (finite weights: what
    hdb_flat_outlier_scores covers): the device hierarchy equals the host's"""
    X, _ = family(name)
    n = X.shape[0]
    _, m = star.exactMST(X, 4, None, 0, selfEdges=True, merged=True)
    host = (m.getVerticeA(), m.getVericeB(), m.getEges())
    dev = tuple(torch.from_numpy(x).cuda() for x in host)
    for mcs in (2, 5):
        hs, hn, hl, hk = pkg.outlier_scores(*host, n, mcs, with_labels=True)
        ds, dn, dl, dk = pkg.outlier_scores(*dev, n, mcs, ctx=ctx, with_labels=True)
        assert dk == hk and np.array_equal(dl.cpu().numpy(), hl), (name, mcs)
        assert bits_eq(ds.cpu().numpy(), hs) and bits_eq(dn.cpu().numpy(), hn), (name, mcs)
        fl, fk = pkg.flat_labels(*dev, n, mcs, ctx=ctx)
        hfl, hfk = pkg.flat_labels(*host, n, mcs)
        assert fk == hfk == hk and np.array_equal(fl.cpu().numpy(), hfl) and np.array_equal(hfl, hl), (name, mcs)


# ---------------------------------------------------------------------------- reference Prim
def check_prim(ctx, star, oracle, X, what):
    core = oracle.core_distances(X, 4, semantics=0)
    va, vb, w = oracle.prim_mst(X, core)
    g = star.constructMST(X, core, True)
    assert np.array_equal(g.getVerticeA(), va) and np.array_equal(g.getVericeB(), vb), what
    assert bits_eq(g.getEges(), w), what
    return w


@pytest.mark.parametrize("name", SPANNING)
def test_reference_prim_block_kernel(ctx, star, oracle, name):
    """n <= 4096: the block Prim (prim_coop=0 where d >= 8 would take the cooperative kernel from
    1,025 rows on, prim.hip prim_batched_device); edges in the reference's order,
    Double.MAX_VALUE for rows it never relaxes (every MRD to them +inf)"""
    X, _ = family(name)
    wide = X.shape[1] >= 8 and X.shape[0] > 1024
    before = ctx.get_stat("prim_coop_launches")
    with options(ctx, prim_coop=0 if wide else 1):
        w = check_prim(ctx, star, oracle, X, name)
    assert ctx.get_stat("prim_coop_launches") == before
    if wide:
        check_prim(ctx, star, oracle, X, name)
        assert ctx.get_stat("prim_coop_launches") == before + 1
    if name == "huge":
        assert np.all(w[:X.shape[0] - 1] == DBL_MAX)


@pytest.mark.parametrize("name", ["same", "lattice3", "huge", "inf_rows"])
def test_reference_prim_cooperative_kernel(ctx, star, oracle, name):
    X, _ = family(name, 4100)
    assert X.shape[0] == 4100
    before = ctx.get_stat("prim_coop_launches")
    check_prim(ctx, star, oracle, X, name)
    assert ctx.get_stat("prim_coop_launches") > before


# ------------------------------------------------------------------------ negative-zero cores
@functools.lru_cache(maxsize=None)
def negzero_case(kind, mix):
    from oracle import oracle as O
    X = family("same")[0] if kind == "same" else np.round(blobs(3000, 3, 6, 77), 1)
    n = X.shape[0]
    core = np.full(n, -0.0)
    if mix:
        keep = np.random.default_rng(5).random(n) < 0.5
        core = np.where(keep, O.core_distances(X, 4, semantics=2), core)
    assert np.signbit(core).any()
    return X, core, kruskal_mst(X, core)


@pytest.mark.parametrize("mix", [False, True])
@pytest.mark.parametrize("kind", ["blobs", "same"])
def test_negative_zero_cores(ctx, star, kind, mix):
    """caller-supplied -0.0 cores (hdbmi.h): weights compare as numbers, so -0.0 acts as +0.0 --
    compared as raw bits it would be the heaviest weight -- and no tree edge weighs -0.0"""
    X, core, ref = negzero_case(kind, mix)
    g = star.constructMSTBoruvka(X, core, True)
    n = X.shape[0]
    va, vb, w = g.getVerticeA(), g.getVericeB(), g.getEges()
    assert not np.signbit(w[:n - 1]).any()
    check_edges((kind, mix), va[:n - 1], vb[:n - 1], w[:n - 1], n, ref)
    assert np.array_equal(va[n - 1:], np.arange(n)) and bits_eq(w[n - 1:], core)  # self edges: the core as passed


# ---------------------------------------------------------------------------- BVH boundaries
def check_boundary(ctx, star, X, core, pw):
    n = X.shape[0]
    launches(ctx, "knn_tree", "boruvka_r0")
    c, g = star.exactMST(X, 4, None, 2, selfEdges=False)
    assert launches(ctx, "knn_tree", "boruvka_r0") == (1, 1)
    assert bits_eq(c, core), n
    assert spanning_tree(g.getVerticeA(), g.getVericeB(), n)
    assert bits_eq(np.sort(g.getEges()), np.sort(pw)), n


# fan 8 over 64-point tiles: a level fills at 512, 4,096 and 32,768 points.  The oracle's O(n^2)
# core scan and Prim take 10.5 s + 9.3 s on one CPU core at 32,769 points, so the sequential
# oracle covers the smallest boundary with a third level above the tiles (4,096)...
@pytest.mark.parametrize("n", [511, 512, 513, 4095, 4096, 4097])
def test_bvh_level_boundaries(ctx, star, oracle, n):
    X = np.round(blobs(n, 3, 5, n), 1)
    core = oracle.core_distances(X, 4, semantics=2)
    check_boundary(ctx, star, X, core, oracle.prim_mst(X, core, self_edges=False)[2])


# ... and the 32,768 boundary is checked against the device's own independent paths instead, each
# pinned to the oracle at smaller sizes: the dense all-pairs K1 for the cores (test_gpu_parity)
# and the cooperative reference Prim for the weights (test_gpu_parity, test_gpu_paths)
@pytest.mark.parametrize("n", [32767, 32768, 32769])
def test_bvh_level_boundary_32768_vs_dense_scan_and_prim(ctx, star, n):
    X = np.round(blobs(n, 3, 12, n), 1)
    launches(ctx, "knn_tree")
    with options(ctx, knn_tree=0):
        core = star.calculateCoreDistances(X, 4, None, 2)
    assert launches(ctx, "knn_tree") == (0,)
    before = ctx.get_stat("prim_coop_launches")
    pw = star.constructMST(X, core, False).getEges()
    assert ctx.get_stat("prim_coop_launches") == before + 1
    check_boundary(ctx, star, X, core, pw)


# -------------------------------------------------------------------------- the NaN contract
@pytest.fixture(scope="module")
def lattice_ok(ctx, star):
    def check():
        X, core, ref = family_case("lattice3", 4, 0)
        c, g = star.exactMST(X, 4, None, 0, selfEdges=False)
        assert bits_eq(c, core)
        check_edges("lattice3 after an error", g.getVerticeA(), g.getVericeB(), g.getEges(), X.shape[0], ref)
    return check


@pytest.mark.parametrize("entry", ["exactMST", "constructMSTBoruvka"])
@pytest.mark.parametrize("name", NOT_SPANNING)
def test_nan_rows_are_einval_and_the_context_lives(pkg, ctx, star, oracle, lattice_ok, name, entry):
    X, _ = family(name)
    bad = np.flatnonzero(np.isnan(X).any(axis=1))
    msg = r"non-finite input: %d row\(s\) .*first: row %d\)" % (bad.shape[0], bad[0])
    with pytest.raises(pkg.HdbError, match=msg):
        if entry == "exactMST":
            star.exactMST(X, 4, None, 0, selfEdges=True)
        else:
            star.constructMSTBoruvka(X, oracle.core_distances(X, 4, semantics=0), True)
    lattice_ok()


def test_driver_k2b_leaf_rejects_nan_row_prim_leaf_accepts(pkg, oracle):
    """one forced leaf of the whole input: through K2b (prim_leaf_max below n) a NaN row is the
    same error, and a fresh run on clean data succeeds; through the reference Prim
    (exact_prim_leaves) it is the reference's result -- Double.MAX_VALUE records for the row no
    comparison ever relaxes"""
    from oracle import mr_driver as M
    X = np.array(family("nan_row")[0])  # writable copies: the driver wraps its input in a tensor
    n = X.shape[0]
    kw = dict(minPts=4, minClSize=4, processing_units=n, flat_labels=False)
    with pytest.raises(pkg.HdbError, match="non-finite input"):
        pkg.MRHDBSCANStar(prim_leaf_max=64, **kw).run(X)
    clean = np.array(family("lattice3")[0])
    ref = M.run(clean, processing_units=clean.shape[0], flat=False)
    got = pkg.MRHDBSCANStar(minPts=4, minClSize=4, processing_units=clean.shape[0], flat_labels=False,
                            prim_leaf_max=64).run(clean)
    # K2b's tree may differ from Prim's among equal weights: the merged weights are the same
    assert bits_eq(got["edges"][2].cpu().numpy(), ref["edges"][2])
    ref = M.run(X, processing_units=n, flat=False)
    got = pkg.MRHDBSCANStar(exact_prim_leaves=True, **kw).run(X)
    for x, y in zip(got["edges"], ref["edges"]):
        assert bits_eq(x.cpu().numpy(), y) if y.dtype == np.float64 else np.array_equal(x.cpu().numpy(), y)
    assert (ref["edges"][2] == DBL_MAX).sum() == 1
