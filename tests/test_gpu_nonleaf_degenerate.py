"""The recursive-sampling half of MR-HDBSCAN* -- nearest sample (K3: nearest_sq / nearest_generic
+ nearest_merge; K3g: nng_home + nng_search), bubble statistics (K4: both fold kernels, the slice
partials and their combine, both variants), bubble k-NN (K5, chunked and plain), the bubble Prims
and the local model -- on the inputs of tests/nonleaf_inputs.py, where its arguments are thinnest:
K3g's pruning guard r^2 (1 + 2^-48) when r^2 underflows, is subnormal, is 0 or overflows; box
bounds whose span overflows; NaN and infinite points and samples; samples that tie at unrelated
list positions; statistics whose variance term 2 n SS - 2 LS^2 is rounding noise, overflows or is
NaN; CF's n (n - 1) as a wrapping Java int; bubbles of extent 0, infinite extent or non-finite rep.

Everything is compared with the CPU oracle bit for bit (NaN equals NaN; integer outputs with
array_equal); the one exception is the tolerance the suite already has for CF's nnDist (a
real-exponent pow, 1e-9 relative, finite entries only).  The bubbles come from the oracle's own
nearest-sample result, never from the device's.  The nearest-sample cases assert through the
nearest_grouped launch count which of K3g and the plain scan ran.

No family is excluded from any check: the oracle produces every reference (the slowest, the
subnormal family's nearest-sample scan, takes about 2.5 s on one CPU core).  Items that need a
bubble model (cores, Prim, local model) run on the families that make at least 8 bubbles, as
specified: same, two_values and tiny collapse to one or two bubbles and are covered by the
statistics checks and by the singleton-bubble cooperative-Prim cases."""
import numpy as np
import pytest
import torch

import nonleaf_inputs as N
from path_helpers import bits_eq, options

pytestmark = pytest.mark.gpu

DBL_MAX = np.finfo(np.float64).max
MODEL_FAMILIES = N.MODEL_FAMILIES
EREF_NEGATIVE_CLUSTER = -12
NEGATIVE_CLUSTER = ["lattice3", "lattice2", "line1", "line_in_8d", "offset", "subnormal", "max_range"]


@pytest.fixture(scope="module")
def ctx(pkg):
    c = pkg.Context(0)  # private: no option set here can leak into another module's context
    c.use_torch_stream()
    c.set_timing(True)  # launch counts
    return c


def k3g_launches(ctx):
    return ctx.kernel_time("nearest_grouped", reset=True)[1]


def check_nearest(pkg, ctx, what, X, S, r_idx, r_dist, grouped, want, metric=None, xk=None, sk=None):
    k3g_launches(ctx)
    with options(ctx, nearest_grouped=grouped):
        idx, dist = pkg.nearest_sample(X, S, metric, xk, sk, ctx=ctx, with_dist=True)
    ran = k3g_launches(ctx)
    bad = np.flatnonzero((idx != r_idx) | ~((dist == r_dist) | (np.isnan(dist) & np.isnan(r_dist))))
    print(f"{what}: n={X.shape[0]} m={S.shape[0]} d={X.shape[1]} grouped={grouped} K3g launches {ran}, "
          f"no candidate {(r_dist == DBL_MAX).sum()}, differing rows {bad.shape[0]}")
    assert ran == want, what
    assert np.array_equal(idx, r_idx), (what, bad[:5], idx[bad[:5]], r_idx[bad[:5]], dist[bad[:5]], r_dist[bad[:5]])
    assert bits_eq(dist, r_dist), (what, bad[:5], dist[bad[:5]], r_dist[bad[:5]])


# ----------------------------------------------------------------------------- nearest sample
@pytest.mark.parametrize("grouped", [1, 0])
@pytest.mark.parametrize("name,variant", N.NEAREST_CASES, ids=lambda v: str(v))
def test_nearest_euclidean_both_paths(pkg, ctx, name, variant, grouped):
    """8,230 rows of every family against X[::7] and its variants: K3g (one launch when the option
    is on, every sample is finite and d is one of 2, 3, 4, 8, 16 -- not line1, not lattice2's
    3,080 rows, not a sample list with a non-finite row) and the plain scan give the oracle's first
    minimum and its distance; a point without a candidate gets index 0 and Double.MAX_VALUE"""
    X, S, r_idx, r_dist = N.nearest_case(name, variant)
    want = N.k3g_runs(X, S, grouped)
    if name in ("line1", "lattice2") or not grouped or (variant == "forced" and not np.isfinite(S).all()):
        assert want == 0
    elif np.isfinite(S).all():
        assert want == 1
    if variant == "dup":  # every sample twice: the lower list position wins
        assert (r_idx < S.shape[0] // 2).all()
    check_nearest(pkg, ctx, (name, variant), X, S, r_idx, r_dist, grouped, want)


@pytest.mark.parametrize("grouped", [1, 0])
@pytest.mark.parametrize("name", N.KEYED)
def test_nearest_keyed_both_paths(pkg, ctx, name, grouped):
    """a key without samples, a key of 20 samples (one group), a key whose 170-odd samples are one
    row (every split of its tree ties), uneven keys otherwise"""
    X, S, xk, sk, r_idx, r_dist = N.keyed_case(name)
    assert (r_dist[xk == 0] == DBL_MAX).all() and (r_idx[xk == 0] == 0).all()
    check_nearest(pkg, ctx, (name, "keyed"), X, S, r_idx, r_dist, grouped, N.k3g_runs(X, S, grouped), xk=xk, sk=sk)


@pytest.mark.parametrize("name", N.NONLEAF_FAMILIES)
def test_nearest_below_the_k3g_thresholds(pkg, ctx, name):
    """the families at their native 1,500 to 3,080 rows: the plain scan, one sample split"""
    X, S, r_idx, r_dist = N.nearest_case(name, "base", None)
    assert X.shape[0] < 8192 and S.shape[0] < 1024
    check_nearest(pkg, ctx, (name, "native"), X, S, r_idx, r_dist, 1, 0)


@pytest.mark.parametrize("grouped", [1, 0])
@pytest.mark.parametrize("d", [8, 16])
def test_nearest_group_boxes_in_global_memory(pkg, ctx, d, grouped):
    """16,448 samples: 514 groups at d = 8, 257 at d = 16, 65,792 bytes of boxes -- more than the
    64 KiB nng_search_kernel stages in LDS, so it reads them from global memory (the host passes
    no dynamic LDS).  No other test against the oracle has more than 16,384 samples."""
    X, S, r_idx, r_dist = N.global_box_case(d)
    check_nearest(pkg, ctx, ("global boxes", d), X, S, r_idx, r_dist, grouped, grouped)


@pytest.mark.parametrize("metric", N.METRICS)
@pytest.mark.parametrize("name", N.METRIC_FAMILIES)
def test_nearest_other_metrics(pkg, ctx, name, metric):
    """nearest_generic_kernel where cosine and Pearson are NaN (tiny, huge: no row has a candidate),
    and the supremum of a NaN row, which is finite"""
    X, S, r_idx, r_dist = N.metric_case(name, metric)
    if name in ("tiny", "huge") and metric in ("cosine", "pearson"):
        assert (r_dist == DBL_MAX).all() and (r_idx == 0).all()
    if name == "nan_rows" and metric == "supremum":
        assert np.isfinite(r_dist).all() and (r_dist < DBL_MAX).all()
    check_nearest(pkg, ctx, (name, metric), X, S, r_idx, r_dist, 1, 0, metric=metric)


# -------------------------------------------------------------------------- bubble statistics
def check_stats(what, got, ref, cf):
    ls, ss, rep, info = got
    for k, a in (("ls", ls), ("ss", ss), ("rep", rep)):
        assert bits_eq(a, ref[k]), (what, k)
    r = ref["info"]
    assert bits_eq(info[:, 0], r[:, 0]), (what, "extent", np.flatnonzero(info[:, 0] != r[:, 0])[:5])
    assert np.array_equal(info[:, 2], r[:, 2]), (what, "n")
    if not cf:
        assert bits_eq(info[:, 1], r[:, 1]), (what, "nnDist")
        return
    fin = np.isfinite(r[:, 1])
    assert np.array_equal(np.isfinite(info[:, 1]), fin), (what, "nnDist finite pattern")
    assert bits_eq(info[~fin, 1], r[~fin, 1]), (what, "nnDist NaN/inf pattern")
    np.testing.assert_allclose(info[fin, 1], r[fin, 1], rtol=1e-9, atol=0)  # real-exponent pow (test_bubble_stats_cf)


@pytest.mark.parametrize("fold_dim", [1, 0])
@pytest.mark.parametrize("variant", ["combine", "cf"])
@pytest.mark.parametrize("name", N.NONLEAF_FAMILIES)
def test_bubble_stats_both_variants_both_folds(pkg, ctx, name, variant, fold_dim):
    """the sign of 2 n SS - 2 LS^2 decides the extent: exactly 0 on identical rows and lattices,
    negative rounding noise on offset, NaN where SS overflows or a member is non-finite"""
    X, bo, nb = N.bubbles_of(name)
    ref = N.stats_case(name, variant)
    with options(ctx, bubble_fold_dim=fold_dim):
        got = pkg.bubble_stats(X, bo, nb, pkg.BUBBLE_CF if variant == "cf" else pkg.BUBBLE_COMBINESTEP, ctx=ctx)
    e = ref["info"][:, 0]
    print(f"{name} {variant} fold_dim={fold_dim}: {nb} bubbles, largest {int(ref['info'][:, 2].max())}, "
          f"extent 0 x{(e == 0).sum()}, NaN x{np.isnan(e).sum()}, inf x{np.isinf(e).sum()}")
    check_stats((name, variant, fold_dim), got, ref, variant == "cf")


def partials_combine(pkg, ctx, X, bo, nb, cuts):
    """hdb_bubble_partials over all slices, then hdb_bubble_combine"""
    A = pkg._capi
    n, d = X.shape
    S = len(cuts) - 1
    Xd, bd = torch.from_numpy(np.array(X)).cuda(), torch.from_numpy(np.array(bo)).cuda()
    pl = torch.empty(S * nb * d, dtype=torch.float64, device="cuda")
    pq, pn = torch.empty_like(pl), torch.empty(S * nb, dtype=torch.float64, device="cuda")
    lc = np.asarray(cuts, np.int64)
    A.check(A.lib().hdb_bubble_partials(ctx.h, Xd.data_ptr(), n, d, bd.data_ptr(), nb, lc.ctypes.data, S,
                                        pl.data_ptr(), pq.data_ptr(), pn.data_ptr()), "partials")
    out = [torch.empty((nb, d), dtype=torch.float64, device="cuda") for _ in range(3)]
    info = torch.empty((nb, 3), dtype=torch.float64, device="cuda")
    A.check(A.lib().hdb_bubble_combine(ctx.h, pl.data_ptr(), pq.data_ptr(), pn.data_ptr(), S, nb, d,
                                       *(o.data_ptr() for o in out), info.data_ptr()), "combine")
    return tuple(o.cpu().numpy() for o in out) + (info.cpu().numpy(),)


@pytest.mark.parametrize("name", N.NONLEAF_FAMILIES)
def test_bubble_slices_vs_oracle(pkg, ctx, name):
    """CombineStep over [0, a, a, b, n] (an empty slice) equals the oracle's sliced fold; over one
    slice it equals hdb_bubble_stats and the oracle's sequential fold"""
    X, bo, nb = N.bubbles_of(name)
    n = X.shape[0]
    check_stats((name, "sliced"), partials_combine(pkg, ctx, X, bo, nb, N.slice_cuts(n)),
                N.stats_case(name, "combine", True), False)
    one = partials_combine(pkg, ctx, X, bo, nb, [0, n])
    check_stats((name, "one slice"), one, N.stats_case(name, "combine"), False)
    whole = pkg.bubble_stats(X, bo, nb, ctx=ctx)
    for a, b in zip(one, whole):
        assert bits_eq(a, b), name


@pytest.mark.parametrize("fold_dim", [1, 0])
def test_bubble_cf_java_int_wraparound(pkg, ctx, fold_dim):
    """CF divides by n * (n - 1) computed as a Java int: exact at 46,341 members, wrapped to a
    negative value at 46,342 (sqrt of a negative sum: NaN), to 0 at 65,536 (NaN again)"""
    X, bo, comb, cf = N.wrap_case()
    assert np.array_equal(comb["info"][:, 2], N.WRAP_SIZES)
    assert np.array_equal(np.isnan(cf["info"][:, 0]), [False, True, True, False])
    assert np.isfinite(comb["info"][:, 0]).all()
    with options(ctx, bubble_fold_dim=fold_dim):
        check_stats("wrap combine", pkg.bubble_stats(X, bo, 4, pkg.BUBBLE_COMBINESTEP, ctx=ctx), comb, False)
        check_stats("wrap cf", pkg.bubble_stats(X, bo, 4, pkg.BUBBLE_CF, ctx=ctx), cf, True)


# -------------------------------------------------------------------------------- bubble model
def model_inputs(name):
    st = N.stats_case(name, "combine")
    assert st["rep"].shape[0] >= 8
    return (st["rep"],) + N.split_info(st["info"])


@pytest.mark.parametrize("split", [1, 0])
@pytest.mark.parametrize("name", MODEL_FAMILIES)
def test_bubble_cores_on_degenerate_statistics(pkg, ctx, name, split):
    """K5 on bubbles of extent 0, nnDist 0, infinite extent and NaN rep: minPts 4 takes the chunked
    scan with its replay (4 chunks at 1,176 bubbles) unless bubble_knn_split is 0, minPts 8 the
    plain scan"""
    rep, nB, eB, nnB = model_inputs(name)
    model = pkg.HdbscanDataBubbles(ctx)
    for mp in (4, 8):
        before = ctx.get_stat("bubble_knn_replay_overflows")
        with options(ctx, bubble_knn_split=split):
            core = model.calculateCoreDistancesBubbles(rep, nB, eB, nnB, mp)
        grew = ctx.get_stat("bubble_knn_replay_overflows") - before
        print(f"{name} minPts {mp} split {split}: {rep.shape[0]} bubbles, replay overflows +{grew}")
        if not split:
            assert grew == 0
        assert bits_eq(core, N.bubble_core_case(name, mp)), (name, mp, split)


def check_graph(what, g, ref):
    va, vb, w = ref
    assert np.array_equal(g.getVerticeA(), va) and np.array_equal(g.getVericeB(), vb), what
    assert bits_eq(g.getEges(), w), what


@pytest.mark.parametrize("name", MODEL_FAMILIES)
def test_bubble_prim_block_kernel(pkg, ctx, name):
    """b <= 4096: the block Prim on the oracle's cores, self edges included (prim_coop 0 where
    d >= 8 and b > 1024 would take the cooperative kernel, and that kernel too)"""
    rep, nB, eB, nnB = model_inputs(name)
    b, d = rep.shape
    assert b <= 4096
    ids = np.arange(b, dtype=np.int32)
    core, ref = N.bubble_core_case(name, 4), N.bubble_prim_case(name)
    model = pkg.HdbscanDataBubbles(ctx)
    wide = d >= 8 and b > 1024
    before = ctx.get_stat("prim_coop_launches")
    with options(ctx, prim_coop=0 if wide else 1):
        check_graph((name, "block"), model.constructMSTBubbles(rep, nB, eB, nnB, ids, core, True), ref)
    assert ctx.get_stat("prim_coop_launches") == before
    if wide:
        check_graph((name, "coop"), model.constructMSTBubbles(rep, nB, eB, nnB, ids, core, True), ref)
        assert ctx.get_stat("prim_coop_launches") == before + 1


@pytest.mark.parametrize("slots", [4, 0])
@pytest.mark.parametrize("name", N.COOP_BUBBLES)
def test_bubble_prim_cooperative_kernels(pkg, ctx, name, slots):
    """4,100 singleton bubbles: the register kernel (prim_coop_slots 4, one counted launch) and the
    counter-barrier kernel (0)"""
    rep, nB, eB, nnB, core, va, vb, w = N.coop_case(name)
    ids = np.arange(rep.shape[0], dtype=np.int32)
    before = ctx.get_stat("prim_coop_launches")
    with options(ctx, prim_coop_slots=slots):
        g = pkg.HdbscanDataBubbles(ctx).constructMSTBubbles(rep, nB, eB, nnB, ids, core, True)
    assert ctx.get_stat("prim_coop_launches") - before == (1 if slots == 4 else 0)
    check_graph((name, slots), g, (va, vb, w))


def local_model_call(A, ctx, rep, info, core):
    b, d = rep.shape
    ne = 2 * b - 1
    lab = np.zeros(b, np.int32)
    mva, mvb, mw = np.zeros(ne, np.int32), np.zeros(ne, np.int32), np.zeros(ne)
    iva, ivb, iw = np.zeros(ne, np.int32), np.zeros(ne, np.int32), np.zeros(ne)
    nic = np.zeros(1, np.int64)
    tail = (A.ptr(lab), A.ptr(mva), A.ptr(mvb), A.ptr(mw), A.ptr(iva), A.ptr(ivb), A.ptr(iw), A.ptr(nic))
    if core is None:
        rc = A.lib().hdb_local_model(ctx.h, A.ptr(rep), A.ptr(info), b, d, 4, 4, 0, *tail)
    else:
        rc = A.lib().hdb_local_model_cores(ctx.h, A.ptr(rep), A.ptr(info), b, d, 4, 4, 0, A.ptr(core), *tail)
    k = int(nic[0])
    return rc, dict(labels=lab, mst=(mva, mvb, mw), inter=(iva[:k], ivb[:k], iw[:k]))


@pytest.mark.parametrize("name", MODEL_FAMILIES)
def test_local_model_vs_oracle(pkg, ctx, name):
    """labels, the quicksorted MST and the inter-cluster edges at minPts 4, minClSize 4; where the
    reference throws "Cluster cannot have less than 0 points" the product raises the same code;
    hdb_local_model_cores on the oracle's cores gives the same"""
    st = N.stats_case(name, "combine")
    rep, info = np.array(st["rep"]), np.array(st["info"])
    core = np.array(N.bubble_core_case(name, 4))
    ref = N.local_model_case(name)
    assert (ref == EREF_NEGATIVE_CLUSTER) == (name in NEGATIVE_CLUSTER), (name, ref)
    A = pkg._capi
    for what, c in (("hdb_local_model", None), ("hdb_local_model_cores", core)):
        rc, got = local_model_call(A, ctx, rep, info, c)
        if isinstance(ref, int):
            assert rc == ref, (name, what, rc)
            with pytest.raises(pkg.IllegalStateException):
                A.check(rc, what)
            continue
        assert rc == 0, (name, what, rc)
        assert np.array_equal(got["labels"], ref["labels"]), (name, what)
        for k in ("mst", "inter"):
            assert np.array_equal(got[k][0], ref[k][0]) and np.array_equal(got[k][1], ref[k][1]), (name, what, k)
            assert bits_eq(got[k][2], ref[k][2]), (name, what, k)
