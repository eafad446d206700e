"""K2g (csrc/boruvka_generic.hip): hdb_mst_boruvka / hdb_exact_mst for every metric and every d.
Everything is compared bit for bit: with K2b through zero-padded columns (which change no
Euclidean distance bit), with the independent Kruskals (path_helpers.kruskal_mst,
metric_kruskal.kruskal_mst_metric) edge for edge, with the cooperative reference Prim's sorted
weights where no CPU reference reaches, and every case asserts through launch counts which scan ran.
On a library without K2g every case ends in HdbError -1 ("euclidean metric only" / "d must be one
of 1,2,3,4,8,16")."""
import functools

import numpy as np
import pytest
import torch

from conftest import blobs
from degenerate_inputs import MST_SETTINGS, NAN_ROWS, SPANNING_FINITE, SPANNING_INF, family, family_case
from metric_kruskal import METRICS, SHAPES, kruskal_mst_metric, metric_case, zero_row
from path_helpers import bits_eq, edge_set, kruskal_mst, spanning_tree

pytestmark = pytest.mark.gpu

K2B_DIMS = (1, 2, 3, 4, 8, 16)


@pytest.fixture(scope="module")
def ctx(pkg):
    c = pkg.Context(0)
    c.use_torch_stream()
    c.set_timing(True)  # launch counts
    return c


@pytest.fixture(scope="module")
def star(pkg, ctx):
    return pkg.HDBSCANStar(ctx)


def launches(ctx, *names):
    return tuple(ctx.kernel_time(k, reset=True)[1] for k in names)


def pad(X):
    """X with zero columns up to the smallest d' > d that K2b has no index for"""
    n, d = X.shape
    dd = d + 1
    while dd in K2B_DIMS:
        dd += 1
    out = np.zeros((n, dd))
    out[:, :d] = X
    return out


def check_edges(what, g, n, ref):
    va, vb, w = g.getVerticeA(), g.getVericeB(), g.getEges()
    assert spanning_tree(va, vb, n)
    got, want = edge_set(va, vb, w), edge_set(*ref)
    assert got == want, (what, len(got - want), sorted(got - want)[:3], sorted(want - got)[:3])
    assert np.all(w[1:] >= w[:-1]), what  # ascending numerically, negative weights first


def same_graph(a, b, what):
    assert np.array_equal(a.getVerticeA(), b.getVerticeA()) and np.array_equal(a.getVericeB(), b.getVericeB()), what
    assert bits_eq(a.getEges(), b.getEges()), what


# ------------------------------------------------------------------ 1. K2g against K2b
@functools.lru_cache(maxsize=None)
def tie_blobs(d0):
    X = np.round(blobs(20000, d0, 8, 300 + d0), 1)
    X.setflags(write=False)
    return X


@pytest.mark.parametrize("d0", [3, 4, 16])
def test_padded_columns_give_k2bs_tree(ctx, star, d0):
    X0 = tie_blobs(d0)
    core = star.calculateCoreDistances(X0, 4)
    launches(ctx, "boruvka_gen_scan", "boruvka_r0")
    plain = star.constructMSTBoruvka(X0, core, True)
    ran = launches(ctx, "boruvka_gen_scan", "boruvka_r0")
    assert ran[0] == 0 and ran[1] == 1, ran
    padded = star.constructMSTBoruvka(pad(X0), core, True)
    ran = launches(ctx, "boruvka_gen_scan", "boruvka_r0")
    assert ran[0] >= 1 and ran[1] == 0, ran
    assert ran[0] == ctx.get_stat("boruvka_gen_rounds")
    same_graph(padded, plain, d0)


# --------------------------------------------------------------------- 2. ragged sizes
def ragged_case(star, oracle, n, d, seed):
    X = np.round(blobs(n, d, 3, seed), 1)
    core = oracle.core_distances(X, 4, semantics=2)
    g = star.constructMSTBoruvka(X, core, False)
    check_edges((n, d), g, n, kruskal_mst(X, core))


def test_ragged_n(ctx, star, oracle):
    qt, ct = ctx.get_stat("boruvka_gen_qt"), ctx.get_stat("boruvka_gen_ct")
    sizes = sorted({1, 2, 3, 63, 64, 65, 257, 1000, qt - 1, qt, qt + 1, ct + 1})
    launches(ctx, "boruvka_gen_scan")
    for n in sizes:
        ragged_case(star, oracle, n, 5, 40 + n)
    assert launches(ctx, "boruvka_gen_scan")[0] >= len(sizes) - 1  # n = 1 has no edge to find


def test_ragged_d_around_the_dimension_chunk(ctx, star, oracle):
    """Euclidean where K2g owns the shape; Manhattan at every d, so that d = DC itself (one of
    K2b's Euclidean shapes when DC is 8) runs the single-chunk kernel too"""
    dc = ctx.get_stat("boruvka_gen_dc")
    for d in (dc - 1, dc, dc + 1, 2 * dc, 2 * dc + 1):
        launches(ctx, "boruvka_gen_scan")
        if d not in K2B_DIMS:
            ragged_case(star, oracle, 300, d, 70 + d)
        X = np.round(blobs(300, d, 3, 170 + d), 1)
        core = oracle.core_distances(X, 4, metric="manhattan", semantics=2)
        g = star.constructMSTBoruvka(X, core, False, "manhattan")
        check_edges(("manhattan", d), g, 300, kruskal_mst_metric(X, core, "manhattan"))
        assert launches(ctx, "boruvka_gen_scan")[0] >= 1


# ----------------------------------------------------- 3. degenerate and non-finite input
@pytest.mark.parametrize("mp,sem", MST_SETTINGS)
@pytest.mark.parametrize("name", SPANNING_FINITE + SPANNING_INF)
def test_degenerate_families_equal_kruskal(ctx, star, name, mp, sem):
    X, core, ref = family_case(name, mp, sem)
    launches(ctx, "boruvka_gen_scan", "boruvka_r0")
    g = star.constructMSTBoruvka(pad(X), core, False)
    ran = launches(ctx, "boruvka_gen_scan", "boruvka_r0")
    assert ran[0] >= 1 and ran[1] == 0, ran
    check_edges((name, mp), g, X.shape[0], ref)
    assert int(np.isinf(g.getEges()).sum()) == int(np.isinf(ref[2]).sum())


@pytest.mark.parametrize("entry", ["exactMST", "constructMSTBoruvka"])
@pytest.mark.parametrize("name", sorted(NAN_ROWS))
def test_nan_rows_are_einval_and_the_context_lives(pkg, ctx, star, oracle, name, entry):
    X = pad(family(name)[0])
    bad = NAN_ROWS[name]
    msg = r"non-finite input: %d row\(s\) .*first: row %d\)" % (len(bad), bad[0])
    with pytest.raises(pkg.HdbError, match=msg) as e:
        if entry == "exactMST":
            star.exactMST(X, 4, None, 0, selfEdges=True)
        else:
            star.constructMSTBoruvka(X, oracle.core_distances(family(name)[0], 4, semantics=0), True)
    assert e.value.code == -1
    Y, core, ref = family_case("lattice3", 4, 0)
    check_edges("lattice3 after an error", star.constructMSTBoruvka(pad(Y), core, False), Y.shape[0], ref)


# -------------------------------------------------------------------- 4. other metrics
@pytest.mark.parametrize("d,n", SHAPES)
@pytest.mark.parametrize("fam", ["rounded_blobs", "rays"])
@pytest.mark.parametrize("metric", METRICS)
def test_other_metrics_equal_kruskal(ctx, star, metric, fam, d, n):
    X, core, ref = metric_case(metric, fam, d, n)
    launches(ctx, "boruvka_gen_scan")
    g = star.constructMSTBoruvka(X, core, False, metric)
    assert launches(ctx, "boruvka_gen_scan")[0] >= 1
    check_edges((metric, fam, d, n), g, n, ref)
    print(f"{metric} {fam} d={d} n={n}: {int((g.getEges() < 0).sum())} negative weights, "
          f"{ctx.get_stat('boruvka_gen_rounds')} rounds")


def test_negative_weights_occur_and_come_back_in_order(star):
    """the point of rays: the tree itself holds weights below zero"""
    X, core, ref = metric_case("cosine", "rays", 5, 1500)
    assert (ref[2] < 0).any() and (ref[2] >= 0).any()
    g = star.constructMSTBoruvka(X, core, False, "cosine")
    check_edges("cosine rays", g, 1500, ref)
    assert bits_eq(g.getEges(), ref[2])


@pytest.mark.parametrize("d,n", [(5, 65), (24, 1500)])
def test_zero_row_under_cosine_is_einval(pkg, star, oracle, d, n):
    X = zero_row(n, d)
    core = oracle.core_distances(X, 4, metric="cosine")
    with pytest.raises(pkg.HdbError, match=r"non-finite input: 1 row\(s\) .*first: row 7\)"):
        star.constructMSTBoruvka(X, core, False, "cosine")


# -------------------------------------------------------------------- 5. hdb_exact_mst
@pytest.mark.parametrize("sem", [0, 1, 2])
def test_exact_mst_d5(pkg, ctx, star, sem):
    X = pad(tie_blobs(4))
    n = X.shape[0]
    want_core = star.calculateCoreDistances(X, 4, None, sem)
    launches(ctx, "boruvka_gen_scan", "boruvka_r0")
    core, g = star.exactMST(X, 4, None, sem, selfEdges=False)
    ran = launches(ctx, "boruvka_gen_scan", "boruvka_r0")
    assert ran[0] >= 1 and ran[1] == 0, ran
    assert bits_eq(core, want_core)
    same_graph(g, star.constructMSTBoruvka(X, core, False), sem)
    for self_edges in (False, True):
        _, p = star.exactMST(X, 4, None, sem, selfEdges=self_edges)
        _, m = star.exactMST(X, 4, None, sem, selfEdges=self_edges, merged=True)
        va, vb, w = pkg.sort_edges_desc(p.getVerticeA().copy(), p.getVericeB().copy(), p.getEges().copy(), ctx)
        assert np.array_equal(m.getVerticeA(), va) and np.array_equal(m.getVericeB(), vb), (sem, self_edges)
        assert bits_eq(m.getEges(), w), (sem, self_edges)
        if self_edges:
            assert np.array_equal(p.getVerticeA()[n - 1:], np.arange(n)) and bits_eq(p.getEges()[n - 1:], core)


def test_exact_mst_d24_euclidean(ctx, star, oracle):
    X = np.round(blobs(3000, 24, 5, 924), 1)
    ctx.kernel_time("knn_mfma", reset=True)
    core, g = star.exactMST(X, 4, None, 2, selfEdges=False)
    assert ctx.kernel_time("knn_mfma", reset=True)[1] >= 1  # the cores are hdb_core_distances': K1m here
    assert bits_eq(core, oracle.core_distances(X, 4, semantics=2))
    check_edges("d24", g, 3000, kruskal_mst(X, core))


def test_exact_mst_d7_manhattan(star, oracle):
    X = np.round(blobs(3000, 7, 5, 907, spread=20.0), 1)
    core, g = star.exactMST(X, 4, "manhattan", 2, selfEdges=False)
    assert bits_eq(core, oracle.core_distances(X, 4, metric="manhattan", semantics=2))
    check_edges("d7 manhattan", g, 3000, kruskal_mst_metric(X, core, "manhattan"))


# ------------------------------------- 6. against the device Prim beyond any CPU reference
@pytest.mark.parametrize("metric", ["euclidean", "manhattan"])
def test_40000_rows_equal_the_cooperative_prim(pkg, ctx, star, metric):
    n = 40000
    X = blobs(n, 24, 10, 6024, spread=30.0, sigma=2.0)
    core = star.calculateCoreDistances(X, 4, metric)
    launches(ctx, "prim_coop", "prim_step_total")
    prim = star.constructMST(X, core, True, metric)
    ran = launches(ctx, "prim_coop", "prim_step_total")
    assert ran[0] >= 1 and ran[1] == 0, ran  # the cooperative Prim, not the stepwise one
    launches(ctx, "boruvka_gen_scan")
    bor = star.constructMSTBoruvka(X, core, True, metric)
    assert launches(ctx, "boruvka_gen_scan")[0] >= 1
    assert spanning_tree(bor.getVerticeA()[:n - 1], bor.getVericeB()[:n - 1], n)
    assert bits_eq(np.sort(bor.getEges()[:n - 1]), np.sort(prim.getEges()[:n - 1]))
    labels = []
    for g in (bor, prim):
        e = pkg.sort_edges_desc(g.getVerticeA().copy(), g.getVericeB().copy(), g.getEges().copy(), ctx)
        labels.append(pkg.flat_labels(*e, n, 8, ctx=ctx))
    assert labels[0][1] == labels[1][1] and np.array_equal(labels[0][0], labels[1][0])


# ------------------------------------------------------------------ 7. device pointers
def test_device_tensors_on_torchs_stream(ctx, star):
    X0 = tie_blobs(3)
    core = star.calculateCoreDistances(X0, 4)
    host = star.constructMSTBoruvka(pad(X0), core, True)
    ctx.use_torch_stream()
    dev = star.constructMSTBoruvka(torch.from_numpy(pad(X0)).cuda(), torch.from_numpy(np.asarray(core)).cuda(), True)
    assert dev.getEges().is_cuda
    assert np.array_equal(dev.getVerticeA().cpu().numpy(), host.getVerticeA())
    assert np.array_equal(dev.getVericeB().cpu().numpy(), host.getVericeB())
    assert bits_eq(dev.getEges().cpu().numpy(), host.getEges())


# -------------------------------------------------------------------------- 8. driver
def test_driver_boruvka_any_leaves(pkg):
    """one forced leaf of 70,000 6-D points: through K2g the merged weights are the stepwise
    Prim's (the default routing for this shape)"""
    n = 70000
    X = blobs(n, 6, 12, 8006, spread=40.0, sigma=1.5)
    kw = dict(minPts=4, minClSize=4, processing_units=n, flat_labels=False)
    got = pkg.MRHDBSCANStar(boruvka_any_leaves=True, **kw).run(np.array(X))
    ref = pkg.MRHDBSCANStar(**kw).run(np.array(X))
    gw, rw = got["edges"][2].cpu().numpy(), ref["edges"][2].cpu().numpy()
    assert gw.shape[0] == 2 * n - 1
    assert bits_eq(np.sort(gw), np.sort(rw))
