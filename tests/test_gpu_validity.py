"""hdb_validity_index (csrc/validity.hip, csrc/validity.cpp) against tests/validity_reference.py, the
plain restatement of its contract (include/hdbmi.h).  Every comparison is bit-exact: the contract
fixes every operation, so there is no tolerance.

Parity: the five metrics, d = 2 (Euclidean trees of large clusters through K2b), 5 (one dimension
chunk) and 24 (several), rounded blobs (ties, duplicates) and rays (negative cosine / Pearson
values), n = 65 and 1,500, three labellings each: the generating labels with about 10 % noise,
uniformly random labels, and the library's own flat labels of the fit.  One labelling built by hand
holds clusters of 1,100 (three sum blocks, the Boruvka route), 513, 512, 65, 64, 3, 2 and 1 members
and an empty label; disjoint clusters of these sizes need 2,260 rows, so it runs on 2,300.
Invariance: forced split counts, the small-cluster bound, host against device pointers, one context
across shapes.  Edges: empty inputs, degenerate clusters, overflow of t^d, non-finite rows, bad
labels, every nullable output left out."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

from metric_kruskal import FAMILIES
from path_helpers import bits_eq
import validity_reference as V

pytestmark = pytest.mark.gpu

METRICS = ("euclidean", "cosine", "pearson", "manhattan", "supremum")
F64 = ("validity", "sparseness", "separation", "core")
I32 = ("nearest_cluster", "size", "internal")
K_GEN = 6
HAND_SIZES = (1100, 513, 512, 65, 64, 3, 2, 1)


@pytest.fixture(scope="module")
def ctx(pkg):
    return pkg.Context(0)


def host(x):
    return x.cpu().numpy() if torch.is_tensor(x) else np.asarray(x)


def as_dict(v):
    out = {k: host(getattr(v, k)) for k in F64 + I32}
    out["index"] = v.index
    return out


def same(got, ref, where=None):
    assert np.float64(got["index"]).view(np.uint64) == np.float64(ref["index"]).view(np.uint64), \
        (where, "index", got["index"], ref["index"])
    for k in F64:
        assert bits_eq(got[k], ref[k]), (where, k, got[k], ref[k])
    for k in I32:
        assert np.array_equal(got[k], ref[k]), (where, k, got[k], ref[k])


def run(pkg, ctx, X, labels, K, metric="euclidean", **kw):
    return as_dict(pkg.validity_index(X, np.asarray(labels, np.int32), metric, K, ctx=ctx, **kw))


@functools.lru_cache(maxsize=None)
def case(family, d, n, metric):
    """(X, its oracle distance matrix), once per process"""
    X = np.ascontiguousarray(FAMILIES[family](n, d), np.float64)
    D = V.dist_matrix(X, metric)
    X.setflags(write=False)
    D.setflags(write=False)
    return X, D


def hand_labels(n, seed=5):
    """clusters of HAND_SIZES members under labels 1..8 (label 9 stays empty), the rest noise, the rows
    dealt at random so that member order is not row order"""
    lab = np.zeros(n, np.int32)
    perm = np.random.default_rng(seed).permutation(n)
    o = 0
    for c, s in enumerate(HAND_SIZES):
        lab[perm[o:o + s]] = c + 1
        o += s
    return lab


@functools.lru_cache(maxsize=None)
def hand_case(metric, d):
    n = 2300
    X, D = case("rounded_blobs", d, n, metric)
    lab = hand_labels(n)
    ref = V.validity_reference(X, lab, 9, metric, D=D)
    return X, lab, ref


# ------------------------------------------------------------------------------------ parity
@pytest.mark.parametrize("n", [65, 1500])
@pytest.mark.parametrize("family", ["rounded_blobs", "rays"])
@pytest.mark.parametrize("d", [2, 5, 24])
@pytest.mark.parametrize("metric", METRICS)
def test_parity_with_the_reference(pkg, ctx, oracle, metric, d, family, n):
    X, D = case(family, d, n, metric)
    labellings = {
        "generating": (V.with_noise(V.generating_labels(family, n, d), 0.1, n + d), K_GEN),
        "random": (V.random_labels(n, K_GEN, n + d), K_GEN),
    }
    try:
        core, g = pkg.HDBSCANStar(ctx).exactMST(X, 4, metric, pkg.CORE_EXCL_SELF, selfEdges=True)
        flat, kf = pkg.flat_labels(g.getVerticeA(), g.getVericeB(), g.getEges(), n, 4 if n < 100 else 10, ctx=ctx)
        labellings["flat"] = (host(flat), kf)
    except pkg.HdbError as e:
        # a row without variance (Pearson at d = 2) or without norm (cosine) has only NaN distances:
        # the fit reports it and there are no flat labels; the other labellings meet the same row below
        assert "non-finite input" in str(e) and metric in ("pearson", "cosine"), e
    for name, (lab, K) in labellings.items():
        try:
            ref = V.validity_reference(X, lab, K, metric, D=D)
        except ValueError as e:  # the Kruskal reference: such a row in a cluster leaves no spanning tree
            assert "do not span" in str(e), e
            with pytest.raises(pkg.HdbError, match=r"validity: cluster \d+: .*non-finite input") as err:
                run(pkg, ctx, X, lab, K, metric)
            assert err.value.code == -1
            continue
        same(run(pkg, ctx, X, lab, K, metric), ref, (name, K))


@pytest.mark.parametrize("metric,d", [("euclidean", 2), ("manhattan", 5)])
def test_parity_on_the_hand_built_labelling(pkg, ctx, oracle, metric, d):
    X, lab, ref = hand_case(metric, d)
    assert ref["size"].tolist() == list(HAND_SIZES) + [0]
    same(run(pkg, ctx, X, lab, 9, metric), ref)


# -------------------------------------------------------------------------------- invariance
@pytest.mark.parametrize("splits", [1, 2, 7, 64])
def test_forced_splits_change_no_bit(pkg, ctx, oracle, splits):
    X, lab, ref = hand_case("manhattan", 5)
    same(run(pkg, ctx, X, lab, 9, "manhattan", splits=splits), ref, splits)
    assert ctx.get_stat("validity_last_splits") == splits == ctx.get_stat("validity_last_core_splits")
    run(pkg, ctx, X, lab, 9, "manhattan")
    assert ctx.get_stat("validity_last_splits") >= 1


@pytest.mark.parametrize("small_max", [0, 2, 1024])
@pytest.mark.parametrize("metric,d", [("euclidean", 2), ("manhattan", 5)])
def test_small_cluster_bound_changes_no_bit(pkg, ctx, oracle, metric, d, small_max):
    X, lab, ref = hand_case(metric, d)
    ctx.set_timing(True)
    try:
        ctx.kernel_time("validity_mst_small")
        same(run(pkg, ctx, X, lab, 9, metric, small_max=small_max), ref, small_max)
        launches = ctx.kernel_time("validity_mst_small")[1]
    finally:
        ctx.set_timing(False)
    assert launches == (0 if small_max == 0 else 1)


def test_host_and_device_pointers_agree(pkg, ctx, oracle):
    X, lab, ref = hand_case("manhattan", 5)
    v = pkg.validity_index(torch.from_numpy(np.array(X)).cuda(), torch.from_numpy(lab).cuda(), "manhattan", 9, ctx=ctx)
    assert torch.is_tensor(v.core) and v.core.is_cuda and v.validity.is_cuda and v.internal.is_cuda
    same(as_dict(v), ref)
    # n_clusters from labels.max(): label 9 is empty, so K = 8
    v8 = as_dict(pkg.validity_index(torch.from_numpy(np.array(X)).cuda(), torch.from_numpy(lab).cuda(), "manhattan"))
    assert v8["size"].shape == (8,) and v8["index"] == ref["index"] and bits_eq(v8["validity"], ref["validity"][:8])


def test_one_context_across_shapes(pkg, oracle):
    own = pkg.Context(0)  # arenas start empty: small, large, small again
    Xs, Ds = case("rounded_blobs", 5, 65, "manhattan")
    ls = V.with_noise(V.generating_labels("rounded_blobs", 65, 5), 0.1, 70)
    rs = V.validity_reference(Xs, ls, K_GEN, "manhattan", D=Ds)
    X, lab, ref = hand_case("manhattan", 5)
    same(run(pkg, own, Xs, ls, K_GEN, "manhattan"), rs, "small")
    same(run(pkg, own, X, lab, 9, "manhattan"), ref, "large")
    same(run(pkg, own, Xs, ls, K_GEN, "manhattan"), rs, "small again")


# ------------------------------------------------------------------------------------- edges
def test_empty_inputs(pkg, ctx):
    r = run(pkg, ctx, np.zeros((0, 3)), np.zeros(0, np.int32), 0)
    assert r["index"] == 0.0 and r["core"].shape == (0,) and r["validity"].shape == (0,)
    r = run(pkg, ctx, np.zeros((0, 3)), np.zeros(0, np.int32), 2)
    assert r["index"] == 0.0 and r["size"].tolist() == [0, 0] and np.all(np.isposinf(r["separation"]))
    X = np.random.default_rng(0).normal(size=(40, 3))
    for K in (0, 3):  # all labels 0
        r = run(pkg, ctx, X, np.zeros(40, np.int32), K)
        same(r, V.validity_reference(X, np.zeros(40, np.int32), K))
        assert r["index"] == 0.0 and not r["internal"].any() and not r["core"].any()


def test_one_cluster(pkg, ctx, oracle):
    X = np.round(np.random.default_rng(1).normal(size=(70, 3)), 1)
    lab = np.ones(70, np.int32)
    lab[::9] = 0
    r = run(pkg, ctx, X, lab, 1)
    same(r, V.validity_reference(X, lab, 1))
    assert r["index"] == 0.0 and np.isposinf(r["separation"][0]) and r["nearest_cluster"][0] == 0 and r["sparseness"][0] > 0


def test_identical_rows(pkg, ctx, oracle):
    row = np.array([1.5, -0.5, 2.0, 0.25])  # with a variance and a norm: Pearson and cosine are defined
    X = np.concatenate([np.tile(row, (30, 1)), np.random.default_rng(2).normal(10.0, 1.0, size=(30, 4))])
    lab = np.repeat(np.array([1, 2], np.int32), 30)
    for metric in METRICS:
        r = run(pkg, ctx, X, lab, 2, metric)
        same(r, V.validity_reference(X, lab, 2, metric), metric)
        if metric in ("euclidean", "manhattan", "supremum"):  # the distance of a row to itself is exactly 0
            assert not r["core"][:30].any() and r["sparseness"][0] == 0.0


def test_power_overflow(pkg, ctx, oracle):
    """200 x 128 rows scaled by 1e-4: t = 1 / dist is about 1e3, t^128 overflows: the cores are 0.0
    as computed"""
    X = np.random.default_rng(3).normal(size=(200, 128)) * 1e-4
    lab = np.repeat(np.array([1, 2], np.int32), 100)
    r = run(pkg, ctx, X, lab, 2)
    same(r, V.validity_reference(X, lab, 2))
    assert not r["core"].any()


def test_non_finite_rows(pkg, ctx, oracle):
    X = np.array(np.round(np.random.default_rng(4).normal(size=(90, 3)), 1))
    lab = V.random_labels(90, 3, 9)
    lab[17] = 0
    X[17, 1] = np.nan
    same(run(pkg, ctx, X, lab, 3), V.validity_reference(X, lab, 3), "NaN in a noise row")
    bad = X.copy()
    noisy = lab.copy()
    row = int(np.flatnonzero(lab > 0)[40])
    bad[row, 2] = np.inf
    bad[int(np.flatnonzero(lab > 0)[60]), 0] = np.nan
    with pytest.raises(pkg.HdbError, match=r"non-finite input \(first: row %d\)" % row) as e:
        run(pkg, ctx, bad, noisy, 3)
    assert e.value.code == -1
    same(run(pkg, ctx, X, lab, 3), V.validity_reference(X, lab, 3), "the call after the error")


@pytest.mark.parametrize("value", [4, -1])
def test_label_out_of_range(pkg, ctx, value):
    X = np.random.default_rng(5).normal(size=(50, 2))
    lab = V.random_labels(50, 3, 1)
    lab[31] = value
    lab[44] = value
    with pytest.raises(pkg.HdbError, match=r"first: row 31\)") as e:
        run(pkg, ctx, X, lab, 3)
    assert e.value.code == -1
    lab[31] = lab[44] = 1
    assert run(pkg, ctx, X, lab, 3)["size"].sum() == np.count_nonzero(lab)


OUTPUTS = ("validity", "sparseness", "separation", "nearest_cluster", "size", "core", "internal")


@pytest.mark.parametrize("left_out", OUTPUTS)
def test_each_output_may_be_null(pkg, ctx, oracle, left_out):
    A = pkg._capi
    X, D = case("rounded_blobs", 5, 65, "euclidean")
    lab = V.with_noise(V.generating_labels("rounded_blobs", 65, 5), 0.1, 70)
    ref = V.validity_reference(X, lab, K_GEN, "euclidean", D=D)
    bufs = {k: np.full(65 if k in ("core", "internal") else K_GEN, -7, np.float64 if k in F64 else np.int32)
            for k in OUTPUTS}
    index = C.c_double(-7.0)
    Xa, la = A.Arr(X, np.float64), A.Arr(lab, np.int32)
    A.call("hdb_validity_index", ctx.h, Xa.p, 65, 5, la.p, K_GEN, 0, C.byref(index),
           *[None if k == left_out else A.ptr(bufs[k]) for k in OUTPUTS])
    assert index.value == ref["index"]
    for k in OUTPUTS:
        if k == left_out:
            assert np.all(bufs[k] == -7)
        elif k in F64:
            assert bits_eq(bufs[k], ref[k]), k
        else:
            assert np.array_equal(bufs[k], ref[k]), k
