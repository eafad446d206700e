"""The point and bubble kernels under cosine, Pearson, Manhattan and supremum, against the CPU
oracle on the inputs of tests/metric_inputs.py: the generic k-NN scan, its merge of partial lists
and the cumulative epilogue (csrc/knn.hip) under the three core semantics; every Prim kernel
(csrc/prim.hip: the four block classes, prim_coop4_kernel<BS, DM> for DM 4, 8 and 16, the
counter-barrier kernel and the stepwise kernel); the batched leaf with leaf_core_kernel; the bubble
k-NN (chunked and plain), the bubble Prim and the local model; and exactMST, which ties the generic
core scan to K2g.

Everything is compared bit for bit (NaN equals NaN), indices with array_equal, and where the oracle
raises the device raises the same code.  No tolerance.  Every case asserts through launch counts
and stats which kernel ran.

On a library whose prim_coop4_kernel keys candidates by the raw bit pattern of the weight, the
cases of that kernel on rays under cosine and Pearson fail: a negative weight's key lies above the
key of +inf, the vertex is never offered, and the kernel leaves its loop with stale edges."""
import numpy as np
import pytest
import torch

import metric_inputs as M
from metric_kruskal import METRICS, metric_case
from path_helpers import bits_eq, edge_set, options, spanning_tree

pytestmark = pytest.mark.gpu

HDB_EINVAL = -1


@pytest.fixture(scope="module")
def ctx(pkg):
    c = pkg.Context(0)  # private: no option set here can leak into another module's context
    c.use_torch_stream()
    c.set_timing(True)  # launch counts
    return c


@pytest.fixture(scope="module")
def star(pkg, ctx):
    return pkg.HDBSCANStar(ctx)


@pytest.fixture(scope="module")
def model(pkg, ctx):
    return pkg.HdbscanDataBubbles(ctx)


PRIM_KERNELS = ("prim_block", "prim_coop", "prim_step_total")


def launches(ctx, *names):
    """launches of each named kernel since the last call"""
    return tuple(ctx.kernel_time(k, reset=True)[1] for k in names)


def cand_split(n):
    """knn_lists_device's candidate split S of the generic scan (csrc/knn.hip)"""
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    tiles = -(-n // 256)
    s = max(1, min(-(-cus * 8 // tiles), 64))
    while s > 1 and n // s < 256:
        s -= 1
    return s


def check_graph(what, g, ref):
    va, vb, w = ref
    ga, gb, gw = np.asarray(g.getVerticeA()), np.asarray(g.getVericeB()), np.asarray(g.getEges())
    bad = np.flatnonzero((ga != va) | (gb != vb) | ~((gw == w) | (np.isnan(gw) & np.isnan(w))))
    print(f"{what}: {w.shape[0]} edges, {int((w < 0).sum())} negative, {bad.shape[0]} differ")
    assert np.array_equal(ga, va), (what, "parents", bad[:5], ga[bad[:5]], va[bad[:5]])
    assert np.array_equal(gb, vb), (what, "vertices", bad[:5])
    assert bits_eq(gw, w), (what, "weights", bad[:5], gw[bad[:5]], w[bad[:5]])


# ------------------------------------------------------------------------------ core distances
@pytest.mark.parametrize("metric", METRICS)
@pytest.mark.parametrize("family,n,d,min_pts", M.CORE_CASES, ids=lambda v: str(v))
def test_core_distances_three_semantics(ctx, star, metric, family, n, d, min_pts):
    """calculateCoreDistances under the three semantics and the k-NN lists they are read from, with
    and without the row itself: knn_generic_kernel, knn_merge_generic_kernel (more than one
    candidate chunk from 512 rows on, 11 at 3000) and the cumul_* prefix merge, which has to carry
    a Double.MAX_VALUE list (a NaN row) and negative values across its 256-row chunks"""
    X = M.points(family, n, d)
    if n == 3000:
        assert cand_split(n) == 11
    if n <= 257:
        assert cand_split(n) == 1
    launches(ctx, "knn_generic")
    for sem in M.SEMANTICS:
        want = M.core_case(metric, family, n, d, min_pts, sem)[1]
        got = star.calculateCoreDistances(X, min_pts, metric, sem)
        bad = np.flatnonzero(~((got == want) | (np.isnan(got) & np.isnan(want))))
        assert bits_eq(got, want), (metric, family, n, d, min_pts, sem, bad[:5], got[bad[:5]], want[bad[:5]])
    k = min_pts - 1
    if k == 0:  # HDBSCANStar.java:75-77: zeros, no scan
        assert launches(ctx, "knn_generic") == (0,)
        return
    for excl in (False, True):
        got = star.knn(X, k, metric, exclSelf=excl)
        assert got.shape == (n, k)
        assert bits_eq(got, M.knn_case(metric, family, n, d, k, excl)), (metric, family, n, d, k, excl)
    assert launches(ctx, "knn_generic") == (5,)


@pytest.mark.parametrize("metric", METRICS)
def test_knn_indices_stay_einval_and_the_context_lives(pkg, ctx, star, metric):
    X = M.points("rays", 257, 5)
    with pytest.raises(pkg.HdbError, match="neighbour indices need the euclidean metric") as e:
        star.knn(X, 3, metric, exclSelf=True, withIndices=True)
    assert e.value.code == HDB_EINVAL
    assert bits_eq(star.calculateCoreDistances(X, 4, metric, 2), M.core_case(metric, "rays", 257, 5, 4, 2)[1])


# --------------------------------------------------------------------------------------- Prim
def run_prim(ctx, star, case, metric):
    X, core, ids, ref = case
    launches(ctx, *PRIM_KERNELS)
    before = ctx.get_stat("prim_coop_launches")
    g = star.constructMST(X, core, True, metric, ids)
    return g, launches(ctx, *PRIM_KERNELS), ctx.get_stat("prim_coop_launches") - before


@pytest.mark.parametrize("n,d", M.BLOCK_SHAPES)
@pytest.mark.parametrize("metric", METRICS)
def test_prim_block_classes(ctx, star, metric, n, d):
    """prim_block_kernel<64, 1>, <64, 4>, <256, 4> and <1024, 4> at their borders: negative
    weights (rays) under cosine and Pearson, massive exact ties and zero weights (integer_grid)
    under Manhattan and supremum"""
    case = M.prim_case(metric, M.family_of(metric), n, d, 4, M.PRIM_SEM)
    g, ran, coop4 = run_prim(ctx, star, case, metric)
    assert ran == (1, 0, 0) and coop4 == 0, ran
    check_graph((metric, n, d), g, case[3])


@pytest.mark.parametrize("dm,n,d", M.COOP4_SHAPES)
@pytest.mark.parametrize("metric", M.COOP4_METRICS)
def test_prim_coop4_default_workgroup(ctx, star, metric, dm, n, d):
    """prim_coop4_kernel<1024, DM>: nearly every tree weight of rays is negative under cosine and
    Pearson, and the order-preserving key has to rank them below zero and below +inf"""
    case = M.prim_case(metric, M.family_of(metric), n, d, 4, M.PRIM_SEM)
    g, ran, coop4 = run_prim(ctx, star, case, metric)
    assert ran[0] == 0 and ran[1] >= 1 and ran[2] == 0 and coop4 == 1, (ran, coop4)
    assert ctx.get_stat("prim_coop_last_bs") == 1024
    check_graph((metric, "DM", dm, n, d), g, case[3])


@pytest.mark.parametrize("metric,n,d,bs", [("cosine", 1100, 8, 128), ("pearson", 4500, 3, 256)])
def test_prim_coop4_smallest_workgroup(ctx, star, metric, n, d, bs):
    """prim_coop_bs 0: the smallest workgroup that keeps the Prim within 32 workgroups"""
    case = M.prim_case(metric, "rays", n, d, 4, M.PRIM_SEM)
    with options(ctx, prim_coop_bs=0):
        g, ran, coop4 = run_prim(ctx, star, case, metric)
    assert ran[0] == 0 and ran[1] >= 1 and ran[2] == 0 and coop4 == 1, (ran, coop4)
    assert ctx.get_stat("prim_coop_last_bs") == bs
    check_graph((metric, n, d, "bs", bs), g, case[3])


@pytest.mark.parametrize("family", ["zero_row7", "zero_row_last"])
def test_prim_coop4_nan_row(ctx, star, family):
    """a row whose every distance is NaN keeps Double.MAX_VALUE and parent 0 and is attached last
    but for ties; as the start vertex (row n - 1) it makes every first-step weight NaN"""
    n, d = M.BAD_ROW_SHAPE
    case = M.prim_case("cosine", family, n, d, 4, M.BAD_ROW_SEM)
    g, ran, coop4 = run_prim(ctx, star, case, "cosine")
    assert ran[0] == 0 and ran[1] >= 1 and ran[2] == 0 and coop4 == 1, (ran, coop4)
    check_graph(("cosine", family), g, case[3])


@pytest.mark.parametrize("coop,want", [(1, (0, 1, 0)), (0, (0, 0, 1))])
def test_prim_counter_barrier_and_stepwise_kernels(ctx, star, coop, want):
    """4500 x 3 cosine rays without the register kernel: prim_coop_kernel, prim_step_kernel"""
    case = M.prim_case("cosine", "rays", 4500, 3, 4, M.PRIM_SEM)
    with options(ctx, prim_coop=coop, prim_coop_slots=0):
        g, ran, coop4 = run_prim(ctx, star, case, "cosine")
    assert ran == want and coop4 == 0, (ran, coop4)
    check_graph(("cosine", 4500, 3, "prim_coop", coop), g, case[3])


def test_prim_coop_kernel_above_16_dimensions(ctx, star):
    n, d = M.COOP_ANY_D
    case = M.prim_case("cosine", "rays", n, d, 4, M.PRIM_SEM)
    g, ran, coop4 = run_prim(ctx, star, case, "cosine")
    assert ran == (0, 1, 0) and coop4 == 0, (ran, coop4)
    check_graph(("cosine", n, d), g, case[3])


# ------------------------------------------------------------------------------- batched leaf
@pytest.mark.parametrize("metric", M.LEAF_METRICS)
def test_batched_leaf(pkg, ctx, metric):
    """FirstStep.leaf over eight partitions: leaf_core_kernel's cumulative cores, the 64 x 1 and
    256 x 4 block Prims, and prim_coop4_kernel from inside a batch (1100 x 8, row offset 442)"""
    X, ids, off, ref = M.leaf_case(metric)
    launches(ctx, "leaf_core", *PRIM_KERNELS)
    before = ctx.get_stat("prim_coop_launches")
    core, g = pkg.FirstStep(1.0, 4096, 4, metric, ctx=ctx).leaf(X, ids, off)
    ran = launches(ctx, "leaf_core", *PRIM_KERNELS)
    assert ran[0] == 1 and ran[1] == 2 and ran[2] >= 1 and ran[3] == 0, ran
    assert ctx.get_stat("prim_coop_launches") - before == 1
    va, vb, w = g.getVerticeA(), g.getVericeB(), g.getEges()
    eo = 0
    for p, (a, b) in enumerate(zip(off[:-1], off[1:])):
        rc, (ra, rb, rw) = ref[p]
        ne = 2 * int(b - a) - 1
        assert bits_eq(core[a:b], rc), (metric, p, "core")
        assert np.array_equal(va[eo:eo + ne], ra) and np.array_equal(vb[eo:eo + ne], rb), (metric, p)
        assert bits_eq(w[eo:eo + ne], rw), (metric, p)
        eo += ne
    assert eo == w.shape[0]


# ------------------------------------------------------------------------------------ bubbles
@pytest.mark.parametrize("split", [1, 0])
@pytest.mark.parametrize("metric,family,n,d", M.BUBBLE_CASES)
def test_bubble_cores(ctx, model, metric, family, n, d, split):
    """K5 on singleton bubbles: minPts 4 takes the chunked scan with its replay at 1100 bubbles
    unless bubble_knn_split is 0, minPts 8 and 300 bubbles the plain scan"""
    rep = M.points(family, n, d)
    nB, eB, nnB = M.singletons(n)
    for mp in (4, 8):
        launches(ctx, "bubble_knn")
        before = ctx.get_stat("bubble_knn_replay_overflows")
        with options(ctx, bubble_knn_split=split):
            core = model.calculateCoreDistancesBubbles(rep, nB, eB, nnB, mp, metric)
        grew = ctx.get_stat("bubble_knn_replay_overflows") - before
        assert launches(ctx, "bubble_knn") == (1,)
        if not split or n < 512 or mp == 8:
            assert grew == 0  # a single chunk: no replay
        assert bits_eq(core, M.bubble_core_case(metric, family, n, d, mp)), (metric, family, n, d, mp, split)


@pytest.mark.parametrize("metric,family,n,d", M.BUBBLE_CASES)
def test_bubble_prim(ctx, model, metric, family, n, d):
    """constructMSTBubbles on the oracle's cores: the block kernel at 300 bubbles, prim_coop4_kernel
    at 1100 x 8"""
    rep = M.points(family, n, d)
    nB, eB, nnB = M.singletons(n)
    core = M.bubble_core_case(metric, family, n, d, 4)
    launches(ctx, *PRIM_KERNELS)
    before = ctx.get_stat("prim_coop_launches")
    g = model.constructMSTBubbles(rep, nB, eB, nnB, np.arange(n, dtype=np.int32), core, True, metric)
    ran, coop4 = launches(ctx, *PRIM_KERNELS), ctx.get_stat("prim_coop_launches") - before
    if n == 300:
        assert ran == (1, 0, 0) and coop4 == 0, ran
    else:
        assert ran[0] == 0 and ran[1] >= 1 and ran[2] == 0 and coop4 == 1, (ran, coop4)
    check_graph((metric, family, n, d), g, M.bubble_prim_case(metric, family, n, d))


@pytest.mark.parametrize("metric,family,n,d", M.BUBBLE_CASES)
def test_local_model(pkg, ctx, model, metric, family, n, d):
    """labels, the quicksorted MST and the inter-cluster edges at minPts 4, minClSize 4; where the
    reference throws "Cluster cannot have less than 0 points" the device raises the same code"""
    rep = M.points(family, n, d)
    info = np.zeros((n, 3))
    info[:, 2] = 1.0
    ref = M.local_model_case(metric, family, n, d)
    launches(ctx, "bubble_knn", *PRIM_KERNELS)
    if isinstance(ref, int):
        with pytest.raises(pkg.HdbError) as e:
            model.localModel(rep, info, 4, 4, metric)
        assert e.value.code == ref, (metric, family, n, d, e.value.code)
    else:
        labels, mst, inter = model.localModel(rep, info, 4, 4, metric)
        assert np.array_equal(labels, ref["labels"]), (metric, family, n, d)
        check_graph((metric, family, n, d, "mst"), mst, ref["mst"])
        assert np.array_equal(inter[0], ref["inter"][0]) and np.array_equal(inter[1], ref["inter"][1])
        assert bits_eq(inter[2], ref["inter"][2]), (metric, family, n, d, "inter")
    ran = launches(ctx, "bubble_knn", *PRIM_KERNELS)
    assert ran[0] == 1 and ran[3] == 0 and (ran[1] == 1) != (ran[2] >= 1), ran
    assert (ran[2] >= 1) == (n == 1100), ran


# ----------------------------------------------------------------------------------- exactMST
@pytest.mark.parametrize("metric", METRICS)
def test_exact_mst_ties_the_core_scan_to_k2g(pkg, ctx, star, metric):
    """one call: the cumulative cores of the generic scan, then K2g's tree over them"""
    n = 1500
    X, core, ref = metric_case(metric, "rays", 5, n)
    launches(ctx, "knn_generic", "boruvka_gen_scan")
    got_core, g = star.exactMST(X, 4, metric, pkg.CORE_INCL_SELF_CUMULATIVE)
    ran = launches(ctx, "knn_generic", "boruvka_gen_scan")
    assert ran[0] == 1 and ran[1] >= 1, ran
    assert bits_eq(got_core, core), metric
    va, vb, w = g.getVerticeA(), g.getVericeB(), g.getEges()
    assert spanning_tree(va[:n - 1], vb[:n - 1], n)
    got, want = edge_set(va[:n - 1], vb[:n - 1], w[:n - 1]), edge_set(*ref)
    assert got == want, (metric, len(got - want), sorted(got - want)[:3], sorted(want - got)[:3])
    assert np.all(w[1:n - 1] >= w[:n - 2]), metric  # ascending numerically, negative weights first
    assert np.array_equal(va[n - 1:], np.arange(n)) and np.array_equal(vb[n - 1:], np.arange(n))
    assert bits_eq(w[n - 1:], core), metric
