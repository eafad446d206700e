"""Host-only checks of tests/driver_cases.py: every case still does on the CPU oracle what it is in
the device matrix (test_gpu_driver_matrix.py) for.  A family that stops recursing, stops raising
or starts forming a tree fails here, without a device.

STRUCTURES are the oracle's results as measured: (iterations, big subsets per level, leaves per
level, [(level, key, code)] of the local-model exceptions, edges, negative / zero /
Double.MAX_VALUE weights, distinct weights, the flat labels' ValueError or None)."""
import numpy as np
import pytest

import driver_cases as D

FIELDS = ("iterations", "big", "leaves", "model_errors", "edges", "negative", "zero", "max", "distinct", "flat_error")
STRUCTURES = {
    "d5r-euclidean-4": (8, [1, 2, 2, 2, 2, 2, 1, 0], [0, 0, 1, 1, 1, 1, 2, 1], [], 5999, 0, 2986, 0, 2134, None),
    "d5r-euclidean-2": (8, [1, 2, 2, 2, 2, 2, 1, 0], [0, 0, 1, 1, 1, 1, 2, 1], [], 5999, 0, 3000, 0, 2134, None),
    "d5r-manhattan-4": (7, [1, 2, 2, 2, 2, 2, 0], [0, 0, 1, 1, 1, 1, 2], [], 5999, 0, 2988, 0, 467, None),
    "d5r-supremum-2": (7, [1, 2, 2, 2, 2, 2, 0], [0, 0, 1, 1, 1, 1, 2], [], 5999, 0, 3000, 0, 70, None),
    "d7-euclidean-4": (8, [1, 2, 2, 2, 2, 4, 2, 0], [0, 0, 1, 1, 1, 0, 3, 2], [], 7999, 0, 3984, 0, 3999, None),
    "d7-supremum-4": (8, [1, 2, 2, 2, 2, 4, 2, 0], [0, 0, 1, 1, 1, 0, 3, 2], [], 7999, 0, 3984, 0, 4000, None),
    "d7r-manhattan-8": (9, [1, 2, 2, 2, 2, 2, 4, 1, 0], [0, 0, 1, 1, 1, 1, 0, 4, 1], [], 7999, 0, 3946, 0, 822, None),
    "d7r-euclidean-8": (8, [1, 2, 2, 2, 2, 4, 2, 0], [0, 0, 1, 1, 1, 0, 3, 2], [], 7999, 0, 3952, 0, 2758, None),
    "d7r-supremum-8": (8, [1, 2, 2, 2, 2, 4, 2, 0], [0, 0, 1, 1, 1, 0, 3, 2], [], 7999, 0, 3952, 0, 98, None),
    "d12-manhattan-first-edge": (8, [1, 2, 2, 2, 4, 2, 2, 0], [0, 0, 1, 1, 0, 3, 1, 2], [], 7999, 0, 3984, 0, 4001,
                                 None),
    "d24-supremum-4": (7, [1, 1, 2, 1, 2, 1, 0], [0, 1, 0, 3, 0, 2, 2], [], 7999, 0, 3984, 0, 4002, None),
    "ang5-cosine-4": (7, [1, 2, 2, 2, 2, 2, 0], [0, 0, 1, 1, 1, 1, 2], [], 5999, 0, 2988, 0, 3002, None),
    "ang5-cosine-8": (7, [1, 2, 2, 2, 2, 2, 0], [0, 0, 1, 1, 1, 1, 2], [], 5999, 0, 2964, 0, 3004, None),
    "ang5-pearson-4": (6, [1, 2, 2, 4, 2, 0], [0, 0, 1, 0, 3, 2], [], 5999, 0, 2988, 0, 2999, None),
    "ang5-pearson-8": (6, [1, 2, 2, 4, 2, 0], [0, 0, 1, 0, 3, 2], [], 5999, 0, 2964, 0, 3015, None),
    "ang7-cosine-2": (7, [1, 2, 2, 4, 4, 2, 0], [0, 0, 1, 0, 2, 3, 2], [], 7999, 0, 4000, 0, 4000, None),
    "ang7-cosine-4": (7, [1, 2, 2, 4, 4, 2, 0], [0, 0, 1, 0, 2, 3, 2], [], 7999, 0, 3984, 0, 4003, None),
    "ang7-pearson-2": (7, [1, 2, 4, 4, 2, 2, 0], [0, 0, 0, 2, 3, 1, 2], [], 7999, 0, 4000, 0, 4000, None),
    "ang7-pearson-4": (7, [1, 2, 4, 4, 2, 2, 0], [0, 0, 0, 2, 3, 1, 2], [], 7999, 0, 3984, 0, 4000, None),
    "ang2-cosine-4": (5, [1, 2, 2, 2, 0], [0, 0, 1, 1, 2], [], 4999, 0, 2492, 0, 2501, None),
    "ang2-pearson-4": (3, [1, 2, 0], [0, 0, 2], [], 4999, 4998, 0, 0, 3, None),
    "ang5_x1-cosine-4": (2, [1, 0], [0, 1], [], 5999, 0, 2998, 0, 3000, None),
    "ang5_x1-pearson-4": (2, [1, 0], [0, 1], [], 5999, 0, 2998, 0, 3000, None),
    "ang7_x1-cosine-4": (2, [1, 0], [0, 1], [], 7999, 0, 3998, 0, 4000, None),
    "ang7_x1-pearson-4": (2, [1, 0], [0, 1], [], 7999, 0, 3998, 0, 4000, None),
    "ang2_x1-cosine-4": (2, [1, 0], [0, 1], [], 4999, 0, 2498, 0, 2500, None),
    "ang2_x1-pearson-4": (2, [1, 0], [0, 1], [], 4999, 4998, 0, 0, 3, None),
    "ang5_x1-cosine-8": (2, [1, 0], [0, 1], [], 5999, 0, 2994, 0, 3000, None),
    "ang5_x1-pearson-8": (2, [1, 0], [0, 1], [], 5999, 0, 2994, 0, 3001, None),
    "ang7_x1-cosine-2": (2, [1, 0], [0, 1], [], 7999, 0, 4000, 0, 4000, None),
    "ang7_x1-pearson-2": (2, [1, 0], [0, 1], [], 7999, 0, 4000, 0, 4000, None),
    "d7-euclidean-9-5": (4, [1, 2, 2, 0], [0, 0, 1, 2], [(2, 5, -12)], 7999, 0, 3979, 0, 4005, None),
    "d5r-manhattan-2": (6, [1, 2, 2, 2, 2, 0], [0, 0, 1, 1, 1, 2], [(4, 10, -12)], 5999, 0, 3000, 0, 467, None),
    "d7r-manhattan-16-10": (3, [1, 2, 0], [0, 0, 2], [(1, 2, -12)], 7999, 0, 3972, 0, 818, None),
    "skin3k-euclidean-32-4": (2, [1, 0], [0, 1], [(0, 0, -12)], 5999, 0, 5293, 0, 28, None),
    "skin3k-euclidean-17-4": (2, [1, 0], [0, 1], [(0, 0, -12)], 5999, 0, 5297, 0, 28, None),
    "grid7-euclidean-4": (5, [1, 2, 2, 4, 0], [0, 0, 1, 0, 4], [], 6017, 0, 3081, 0, 45, "not a spanning tree"),
    "n2-euclidean-4": (1, [0], [1], [], 3, 0, 0, 2, 2, "not a spanning tree"),
    "ang5_zero-cosine-4": (7, [1, 2, 2, 2, 2, 2, 0], [0, 0, 1, 1, 1, 1, 2], [], 5999, 0, 3047, 4, 2940,
                           "the edges contain a cycle"),
    "ang5_zero-pearson-4": (5, [1, 2, 2, 2, 0], [0, 0, 1, 1, 2], [], 5999, 0, 3052, 3, 2939,
                            "the edges contain a cycle"),
    "ang5_dup-cosine-4": (7, [1, 2, 2, 2, 2, 2, 0], [0, 0, 1, 1, 1, 1, 2], [], 5999, 0, 3048, 0, 2942, None),
    "tiny1-euclidean-4": (1, [0], [1], [], 1, 0, 0, 1, 1, None),
    "tiny1-cosine-4": (1, [0], [1], [], 1, 0, 0, 1, 1, None),
    "tiny5-euclidean-4": (1, [0], [1], [], 9, 0, 3, 0, 5, None),
    "tiny5-cosine-4": (1, [0], [1], [], 9, 0, 3, 0, 5, None),
    "tiny50-euclidean-4": (1, [0], [1], [], 99, 0, 48, 0, 51, None),
    "tiny50-cosine-4": (1, [0], [1], [], 99, 0, 48, 0, 51, None),
    "tiny51-euclidean-4": (1, [0], [1], [], 101, 0, 49, 0, 51, None),
    "tiny51-cosine-4": (1, [0], [1], [], 101, 0, 49, 0, 52, None),
    "ov7-euclidean-8": (6, [1, 2, 4, 2, 1, 0], [0, 0, 0, 3, 2, 1], [], 6009, 0, 2964, 0, 3026, "not a spanning tree"),
    "ov7-manhattan-4": (5, [1, 2, 4, 2, 0], [0, 0, 0, 3, 2], [], 6007, 0, 2990, 0, 3011, "not a spanning tree"),
    "ov7-supremum-4": (4, [1, 2, 2, 0], [0, 0, 1, 2], [], 6001, 0, 2994, 0, 3002, "not a spanning tree"),
    "ovang7-cosine-4": (4, [1, 2, 4, 0], [0, 0, 0, 4], [], 5999, 0, 2992, 0, 3000, None),
    "ovang7-cosine-8": (6, [1, 2, 4, 4, 1, 0], [0, 0, 0, 2, 4, 1], [], 6016, 0, 2958, 0, 3035,
                        "not a spanning tree"),
    "ovang7-pearson-4": (4, [1, 2, 4, 0], [0, 0, 0, 4], [], 5999, 0, 2992, 0, 3000, None),
    "ovang5-cosine-8": (3, [1, 2, 0], [0, 0, 2], [], 5999, 0, 2988, 0, 3007, None),
}
# driver_cases.filter_rows of the cases where it is not 0 at every level: per level, the rows that a
# scan without the key filter would hand to another subset
FILTER_ROWS = {
    "grid7-euclidean-4": [0, 2, 7, 39],
    "ov7-euclidean-8": [0, 0, 12, 40, 0],
    "ov7-manhattan-4": [0, 1, 4, 22],
    "ov7-supremum-4": [0, 5, 0],
    "ovang7-cosine-4": [0, 0, 2],
    "ovang7-cosine-8": [0, 0, 2, 66, 0],
    "ovang7-pearson-4": [0, 0, 1],
    "ovang5-cosine-8": [0, 15],
}


def test_every_case_has_a_literal():
    assert list(STRUCTURES) == list(D.CASES)
    assert set(D.VARIANT_CASES + D.BORUVKA_CASES) <= set(D.DEVICE_CASES)
    for name in D.CASES:
        assert D.input_of(D.CASES[name][0]).shape[0] <= 4000 and not D.input_of(D.CASES[name][0]).flags.writeable


@pytest.mark.parametrize("name", list(D.CASES))
def test_structure_is_the_measured_one(oracle, name):
    assert D.structure(name) == dict(zip(FIELDS, STRUCTURES[name]))


@pytest.mark.parametrize("name", list(D.RECURSING) + list(D.ANGULAR) + ["ang2-cosine-4"])
def test_recursing_cases_recurse(oracle, name):
    """at least 5 iterations and a level with at least 2 big subsets: the keyed nearest sample gets
    several keys, and bubble slices, model pool, induction, deferred leaves and merge all run"""
    s = D.structure(name)
    assert D.recurses(s) and not s["model_errors"], s
    assert s["edges"] == 2 * D.input_of(D.CASES[name][0]).shape[0] - 1
    if D.keywords(name).get("all_inter_edges", True):
        assert s["flat_error"] is None and "labels" in D.oracle_run(name)[0]
    else:
        assert "labels" not in D.oracle_run(name)[0]  # Main.java's first edge only: no flat labels


def test_recursing_cases_cover_the_metrics_dims_and_list_buckets():
    kws = [D.keywords(n) for n in list(D.RECURSING) + list(D.ANGULAR)]
    assert {k["metric"] for k in kws} == {"euclidean", "manhattan", "supremum", "cosine", "pearson"}
    assert {D.input_of(D.CASES[n][0]).shape[1] for n in D.RECURSING} == {5, 7, 12, 24}
    # k-NN list capacities (the power of two holding minPts - 1 entries, less one): 1, 3, 7 recurse;
    # 15 and 31 come with the exception cases below
    assert {k["min_pts"] for k in kws} == {2, 4, 8}
    assert {D.keywords(n)["min_pts"] for n in D.ERRORS} == {2, 9, 16, 17, 32}
    assert any(D.keywords(n)["min_pts"] != D.keywords(n)["min_cl_size"] for n in D.ERRORS)


@pytest.mark.parametrize("name", list(D.UNSCALED))
def test_angular_inputs_in_their_natural_scale_do_not_recurse(oracle, name):
    """the reason test_driver_cosine_forced_leaf_above_4096 never gets past level 0: the same rows
    as ANGULAR / ANG2 without the factor 1e-2 give one cluster at level 0 and one forced leaf"""
    s = D.structure(name)
    assert (s["iterations"], s["big"], s["leaves"], s["model_errors"]) == (2, [1, 0], [0, 1], [])
    scaled = name.replace("_x1", "")
    assert np.array_equal(D.input_of(D.CASES[scaled][0]), 1e-2 * D.input_of(D.CASES[name][0]))
    assert D.structure(scaled)["iterations"] > 2


def test_ang2_pearson_is_all_ties(oracle):
    """d = 2: a Pearson distance is 0, 2 or a few ulps off them, so the first minimum by sample index
    decides almost every row of the keyed scan"""
    s = D.structure("ang2-pearson-4")
    assert (s["edges"], s["negative"], s["distinct"]) == (4999, 4998, 3)
    assert s["iterations"] == 3 and max(s["big"]) == 2


@pytest.mark.parametrize("name", list(D.ERRORS))
def test_error_cases_raise_inside_the_loop(oracle, name):
    s = D.structure(name)
    assert s["model_errors"] == [(lv, key, D.EREF_NEGATIVE_CLUSTER) for lv, key in D.ERRORS[name][1]]
    assert s["flat_error"] is None
    out = D.oracle_run(name)[0]
    for lv, key in D.ERRORS[name][1]:  # D10: one label, then a forced leaf of the same rows one level down
        L = out["levels"][lv]
        assert len(L["new_keys"][key]) == 1 and (L["labels"][key] == 2).all()
        assert out["levels"][lv + 1]["leaves"][L["new_keys"][key][0]] == L["big"][key]
    if name.startswith("skin3k"):  # the whole prefix is one forced leaf whose lists hold 16 / 31 entries: capacity 31
        assert s["leaves"] == [0, 1] and out["levels"][1]["leaves"] == {2: 3000}
        assert 16 <= D.keywords(name)["min_pts"] - 1 <= 31


@pytest.mark.parametrize("name", list(D.NON_TREE))
def test_non_tree_cases_fail_flat_extraction_only(oracle, name):
    out, err = D.oracle_run(name)
    assert err is not None and D.NON_TREE[name][1] in err and "labels" not in out
    va, vb, w = out["edges"]
    n = D.input_of(D.CASES[name][0]).shape[0]
    s = D.structure(name)
    if name.startswith("grid7"):
        assert (s["edges"], int((va != vb).sum()), s["iterations"]) == (6017, 3017, 5) and 3017 > n - 1
    elif name.startswith("n2"):
        assert (s["edges"], s["max"], int((va != vb).sum())) == (3, 2, 0)
    else:  # n - 1 non-self edges that close a cycle: a zero row is at Double.MAX_VALUE from everything
        assert int((va != vb).sum()) == n - 1 and s["max"] >= 3 and D.recurses(s)


def test_duplicated_rows_alone_keep_the_tree(oracle):
    out, err = D.oracle_run("ang5_dup-cosine-4")
    assert err is None and out["n_clusters"] >= 1
    assert np.array_equal(D.input_of("ang5_dup")[100:160], np.tile(D.input_of("ang5")[99], (60, 1)))
    z = D.input_of("ang5_zero")
    assert np.array_equal(np.flatnonzero(~z.any(axis=1)), [7, 1500, 2999])
    keep = np.setdiff1d(np.arange(3000), [7, 1500, 2999])
    assert np.array_equal(z[keep], D.input_of("ang5_dup")[keep])


@pytest.mark.parametrize("name", D.DEVICE_CASES)
def test_which_cases_depend_on_the_key_filter(oracle, name):
    """On separated blobs every row's nearest sample over the whole level already lies in its own
    subset (measured: 0 rows at every level of every RECURSING, ANGULAR and ERRORS case), so those
    runs cannot tell a keyed scan from an unkeyed one.  The OVERLAP cases and grid7 can: under each
    of the five metrics some level has rows that an unkeyed scan would move to another subset."""
    rows = D.filter_rows(name)
    s = D.structure(name)
    assert len(rows) == sum(1 for b in s["big"] if b) and rows[:1] in ([], [0])  # one subset at level 0
    assert rows == FILTER_ROWS.get(name, [0] * len(rows))
    if name in D.OVERLAP:
        assert sum(rows) > 0 and max(s["big"]) >= 2 and D.FLAT_ERRORS.get(name) == D.OVERLAP[name][1]
        assert s["flat_error"] is None or D.OVERLAP[name][1] in s["flat_error"]
        assert (s["flat_error"] is None) == (D.OVERLAP[name][1] is None)


def test_overlap_cases_cover_the_five_metrics():
    assert {D.keywords(n)["metric"] for n in D.OVERLAP} == {"euclidean", "manhattan", "supremum", "cosine", "pearson"}
    assert set(FILTER_ROWS) == set(D.OVERLAP) | {"grid7-euclidean-4"}


@pytest.mark.parametrize("name", list(D.TINY))
def test_tiny_cases_are_one_leaf(oracle, name):
    s = D.structure(name)
    n = D.input_of(D.CASES[name][0]).shape[0]
    assert (s["iterations"], s["big"], s["leaves"], s["edges"]) == (1, [0], [1], 2 * n - 1)
    assert s["flat_error"] is None


def test_variant_oracle_runs_are_cached_apart(oracle):
    a = D.oracle_run("d5r-euclidean-2")[0]
    b = D.oracle_run("d5r-euclidean-2", bubble_slices=1)[0]
    assert a is D.oracle_run("d5r-euclidean-2")[0] and b is not a
    assert b is D.oracle_run("d5r-euclidean-2", bubble_slices=1)[0]
