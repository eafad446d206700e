"""The whole MR-HDBSCAN* loop on the device under every metric and at minPts other than 4: the
product driver against the oracle's restatement of the same loop on the cases of
tests/driver_cases.py (what each case is made of is asserted on the CPU, test_driver_cases.py).

test_gpu_driver.py, test_gpu_c1.py, test_gpu_mr_scaled.py and test_gpu_sharded.py pin the loop at
Euclidean, minPts = minClSize = 4 only, and the one cosine run there never gets past level 0.  Here
the keyed nearest sample runs with several keys under all five metrics and at d without a fast
instantiation, levels with several big subsets run bubble slices, the model pool, induction,
deferred leaves and the merge under Manhattan, supremum, cosine and Pearson, minPts 2, 8, 9, 16, 17
and 32 fill the k-NN list capacities 1, 7, 15 and 31, minClSize differs from minPts, the local
model raises the reference's exception inside the loop, and the merged list is not a tree.
On the separated blobs of most cases no row lies nearer to another subset's sample than to its
own, so a scan without the key filter would pass them; the OVERLAP cases and grid7 are the runs
that fail without it (driver_cases.filter_rows, asserted on the CPU).

Everything is compared bit for bit: levels, bubble labels, induced keys, model errors, the leaf of
every point, the merged edges (weights with bits_eq), the flat labels.  The launch counts of the
run's context say which nearest-sample scan ran."""
import numpy as np
import pytest

import driver_cases as D
from path_helpers import bits_eq
from test_gpu_driver import check

pytestmark = pytest.mark.gpu

HDB_EINVAL = -1  # include/hdbmi.h
SCANS = ("nearest_grouped", "nearest_sq", "nearest_generic")
FAST_DIMS = (1, 2, 3, 4, 5, 6, 8, 16)  # nearest.hip: the Euclidean scan's instantiations


@pytest.fixture(scope="module")
def ctx(pkg):
    c = pkg.Context(0)  # private: the launch counts are this module's
    c.use_torch_stream()
    c.set_timing(True)
    return c


def device_run(pkg, ctx, name, over=(), **driver_kw):
    """(the driver's result, nearest-sample launches by scan); over: oracle keywords overridden"""
    kw = D.keywords(name, **dict(over))
    star = pkg.MRHDBSCANStar(minPts=kw["min_pts"], minClSize=kw["min_cl_size"], processing_units=kw["processing_units"],
                             k=kw["k"], samples_per_subset=kw.get("samples_per_subset"),
                             all_inter_edges=kw.get("all_inter_edges", True), distanceFunction=kw["metric"],
                             bubble_slices=kw["bubble_slices"], ctx=ctx, **driver_kw)
    for k in SCANS:
        ctx.kernel_time(k, reset=True)
    got = star.run(np.array(D.input_of(D.CASES[name][0])))
    return got, {k: ctx.kernel_time(k, reset=True)[1] for k in SCANS}


def check_bits(ref, got):
    check(ref, got)
    assert bits_eq(got["edges"][2].cpu().numpy(), ref["edges"][2])


def check_scans(name, ref, ran):
    """one keyed nearest-sample call per level that has a big subset: the generic scan under a
    non-Euclidean metric and at d = 7, 12, 24, the fast one otherwise; never K3g (n <= 4000)"""
    kw = D.keywords(name)
    d = D.input_of(D.CASES[name][0]).shape[1]
    levels = sum(1 for L in ref["levels"] if L["big"])
    generic = kw["metric"] != "euclidean" or d not in FAST_DIMS
    assert ran == {"nearest_grouped": 0, "nearest_sq": 0 if generic else levels,
                   "nearest_generic": levels if generic else 0}, (name, ran, levels)
    return generic


@pytest.mark.parametrize("name", [n for n in D.DEVICE_CASES if n not in D.FLAT_ERRORS])
def test_driver_matches_oracle_under_every_metric(pkg, ctx, name):
    ref, err = D.oracle_run(name)
    assert err is None
    got, ran = device_run(pkg, ctx, name)
    print(f"{name}: iterations {got['iterations']}, big {[len(L['big']) for L in got['levels']]}, launches {ran}")
    check_bits(ref, got)
    assert ("labels" in got) == ("labels" in ref)
    generic = check_scans(name, ref, ran)
    if name in D.RECURSING or name in D.ANGULAR:
        d = D.input_of(D.CASES[name][0]).shape[1]
        assert generic == (D.keywords(name)["metric"] != "euclidean" or d in (7, 12, 24))
        assert ran["nearest_generic" if generic else "nearest_sq"] >= 5


@pytest.mark.parametrize("name", list(D.FLAT_ERRORS))
def test_driver_on_a_merged_list_that_is_no_tree(pkg, ctx, name):
    """the oracle's flat labels raise ValueError, the device's HDB_EINVAL; without flat labels the
    run equals the oracle's flat=False run"""
    ref, err = D.oracle_run(name)
    assert err is not None and D.FLAT_ERRORS[name] in err and "labels" not in ref
    with pytest.raises(pkg.HdbError) as ei:
        device_run(pkg, ctx, name, flat_labels=True)
    assert ei.value.code == HDB_EINVAL
    got, ran = device_run(pkg, ctx, name, flat_labels=False)
    assert "labels" not in got
    check_bits(ref, got)
    check_scans(name, ref, ran)


@pytest.fixture(scope="module")
def default_runs(pkg, ctx):
    """the default device run of a variant case, once per module, as host arrays"""
    cache = {}

    def get(name):
        if name not in cache:
            cache[name] = device_run(pkg, ctx, name)[0]
        return cache[name]
    return get


def same_run(a, b):
    assert a["iterations"] == b["iterations"] and len(a["levels"]) == len(b["levels"])
    for x, y in zip(a["levels"], b["levels"]):
        assert x["leaves"] == y["leaves"] and x["big"] == y["big"] and x["new_keys"] == y["new_keys"]
        assert x.get("model_errors") == y.get("model_errors")
        assert x["labels"].keys() == y["labels"].keys()
        for k in y["labels"]:
            assert np.array_equal(x["labels"][k], y["labels"][k]), k
    assert np.array_equal(a["leaf_of"].cpu().numpy(), b["leaf_of"].cpu().numpy())
    for x, y in zip(a["edges"][:2], b["edges"][:2]):
        assert np.array_equal(x.cpu().numpy(), y.cpu().numpy())
    assert bits_eq(a["edges"][2].cpu().numpy(), b["edges"][2].cpu().numpy())
    assert a["n_clusters"] == b["n_clusters"] and np.array_equal(a["labels"].cpu().numpy(), b["labels"].cpu().numpy())


@pytest.mark.parametrize("variant", [dict(defer_leaves=False), dict(cores_first=True), dict(model_threads=1),
                                     dict(exact_prim_leaves=True)], ids=lambda v: "-".join(v))
@pytest.mark.parametrize("name", D.VARIANT_CASES)
def test_driver_variants_change_nothing(pkg, ctx, default_runs, name, variant):
    """per-level leaf batches, cores before Prims, no model pool, exact Prim leaves: the default
    run's result, which is the oracle's"""
    got, ran = device_run(pkg, ctx, name, **variant)
    same_run(got, default_runs(name))
    check_bits(D.oracle_run(name)[0], got)
    check_scans(name, D.oracle_run(name)[0], ran)


@pytest.mark.parametrize("name", D.VARIANT_CASES)
def test_driver_one_bubble_slice(pkg, ctx, name):
    """bubble_slices = 1 (one sequential fold, hdb_bubble_stats instead of partials + combine)
    against the oracle run with 1"""
    ref, err = D.oracle_run(name, bubble_slices=1)
    assert err is None
    got, ran = device_run(pkg, ctx, name, over=(("bubble_slices", 1),))
    check_bits(ref, got)
    check_scans(name, ref, ran)


@pytest.mark.parametrize("name", D.BORUVKA_CASES)
def test_driver_leaves_through_the_exact_mst(pkg, ctx, name):
    """prim_leaf_max = 64 with boruvka_any_leaves: every leaf above 64 points goes to hdb_exact_mst
    (K2g at d = 5 under an angular metric and at d = 7).  Exact weights; the topology may differ
    from the reference Prim's on ties only, so levels, bubble labels, the leaf of every point, the
    sorted weights (the merged list is sorted: multiset equality) and the flat labels are compared,
    as test_gpu_c1.py does for its default driver"""
    ref, err = D.oracle_run(name)
    assert err is None
    assert max(max(L["leaves"].values(), default=0) for L in ref["levels"]) > 64
    got, ran = device_run(pkg, ctx, name, prim_leaf_max=64, boruvka_any_leaves=True)
    check_scans(name, ref, ran)
    assert got["iterations"] == ref["iterations"]
    for a, b in zip(got["levels"], ref["levels"]):
        assert a["leaves"] == b["leaves"] and a["big"] == b["big"] and a["new_keys"] == b["new_keys"]
        assert a.get("model_errors") == b.get("model_errors")
        for k in b["labels"]:
            assert np.array_equal(a["labels"][k], b["labels"][k]), k
    assert np.array_equal(got["leaf_of"].cpu().numpy(), ref["leaf_of"])
    va, vb, w = (x.cpu().numpy() for x in got["edges"])
    assert np.array_equal(w, ref["edges"][2])
    n = ref["leaf_of"].shape[0]
    assert int((va == vb).sum()) == n and np.array_equal(np.sort(va[va == vb]), np.arange(n))
    assert got["n_clusters"] == ref["n_clusters"]
    assert np.array_equal(got["labels"].cpu().numpy(), ref["labels"])
