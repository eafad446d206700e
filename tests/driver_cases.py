"""Named, seeded, read-only runs of the whole MR-HDBSCAN* loop (keyed nearest sample, bubble
partials, local model, induction, leaves, merge, flat labels) under every metric and at minPts
other than 4, with the CPU oracle's result of each (oracle/mr_driver.py over hdb_oracle.c).
test_driver_cases.py asserts on the CPU that every case still does what it is there for;
test_gpu_driver_matrix.py compares the device's loop with these results.  CPU only; nothing here
touches the library.

A case is (input name, oracle keywords); the keywords left out are DEFAULTS.  Families:

  RECURSING   at least 5 iterations and a level with at least 2 big subsets (there the keyed
              nearest sample sees several keys), Euclidean / Manhattan / supremum at d = 5, 7, 12,
              24 (d = 7, 12, 24 have no fast nearest-sample instantiation: the generic scan)
  ANGULAR     cosine / Pearson on inputs scaled by 1e-2.  Bubble extents are Euclidean-sized and
              angular distances are at most 2, so at scale 1 (UNSCALED) the level-0 model returns
              one cluster, the input becomes one forced leaf and nothing after level 0 runs
  ERRORS      the local model raises the reference's own exception inside the loop (D10,
              HDB_EREF_NEGATIVE_CLUSTER): recorded, the subset forced to a leaf
  NON_TREE    the merged list is not a spanning tree: the oracle's flat labels raise ValueError;
              the edge lists are still compared
  TINY        n = 1, 5, 50, 51: one leaf, one iteration
  OVERLAP     blobs that overlap: sibling subsets touch, so some rows lie nearer to a sample of
              another subset than to any of their own.  On the separated blobs of the families
              above no row does (filter_rows is 0 at every level): there a nearest-sample scan that
              ignored the keys would return the same result, and only these cases, grid7 and the
              kernel tests (test_gpu_nearest_keyed_metrics.py) tell the key filter from none
"""
import functools

import numpy as np

from conftest import blobs, load_skin

DEFAULTS = dict(min_pts=4, min_cl_size=4, processing_units=300, k=0.1, bubble_slices=8, metric="euclidean")
JMAX = np.finfo(np.float64).max
EREF_NEGATIVE_CLUSTER = -12


def _ang5_zero():
    X = np.array(input_of("ang5"))
    X[100:160] = X[99]
    X[[7, 1500, 2999]] = 0.0
    return X


def _ang5_dup():
    X = np.array(input_of("ang5"))
    X[100:160] = X[99]
    return X


INPUTS = {
    "d5r": lambda: np.round(blobs(3000, 5, 6, 1, spread=20.0) + 25.0, 1),
    "d7": lambda: blobs(4000, 7, 8, 2, spread=30.0) + 10.0,
    "d7r": lambda: np.round(blobs(4000, 7, 8, 2, spread=30.0), 1),
    "d12": lambda: blobs(4000, 12, 8, 2, spread=30.0),
    "d24": lambda: blobs(4000, 24, 8, 2, spread=30.0),
    "ang5": lambda: 1e-2 * blobs(3000, 5, 6, 1, spread=20.0),
    "ang7": lambda: 1e-2 * np.round(blobs(4000, 7, 8, 2, spread=30.0), 1),
    "ang2": lambda: 1e-2 * blobs(2500, 2, 5, 8, spread=20.0),
    "ang5_x1": lambda: blobs(3000, 5, 6, 1, spread=20.0),
    "ang7_x1": lambda: np.round(blobs(4000, 7, 8, 2, spread=30.0), 1),
    "ang2_x1": lambda: blobs(2500, 2, 5, 8, spread=20.0),
    "skin3k": lambda: load_skin(3000),
    "grid7": lambda: np.round(blobs(3000, 7, 6, 3, spread=4.0)),
    "n2": lambda: blobs(2, 3, 2, 2),
    "ov7": lambda: blobs(3000, 7, 6, 3, spread=4.0),
    "ovang7": lambda: 1e-2 * blobs(3000, 7, 6, 3, spread=4.0),
    "ovang5": lambda: 1e-2 * blobs(3000, 5, 6, 1, spread=3.0),
    "ang5_zero": _ang5_zero,
    "ang5_dup": _ang5_dup,
    "tiny1": lambda: blobs(1, 3, 2, 1),
    "tiny5": lambda: blobs(5, 3, 2, 5),
    "tiny50": lambda: blobs(50, 3, 2, 50),
    "tiny51": lambda: blobs(51, 3, 2, 51),
}


@functools.lru_cache(maxsize=None)
def input_of(name):
    X = np.ascontiguousarray(INPUTS[name](), np.float64)
    X.setflags(write=False)
    return X


def _mp(a, b):
    return dict(min_pts=a, min_cl_size=b)


RECURSING = {
    "d5r-euclidean-4": ("d5r", {}),
    "d5r-euclidean-2": ("d5r", _mp(2, 2)),
    "d5r-manhattan-4": ("d5r", dict(metric="manhattan")),
    "d5r-supremum-2": ("d5r", dict(metric="supremum", **_mp(2, 2))),
    "d7-euclidean-4": ("d7", {}),
    "d7-supremum-4": ("d7", dict(metric="supremum")),
    "d7r-manhattan-8": ("d7r", dict(metric="manhattan", **_mp(8, 8))),
    "d7r-euclidean-8": ("d7r", _mp(8, 8)),
    "d7r-supremum-8": ("d7r", dict(metric="supremum", **_mp(8, 8))),
    "d12-manhattan-first-edge": ("d12", dict(metric="manhattan", all_inter_edges=False)),
    "d24-supremum-4": ("d24", dict(metric="supremum", processing_units=500, samples_per_subset=150, bubble_slices=3)),
}
ANGULAR = {f"{x}-{m}-{p}": (x, dict(metric=m, **_mp(p, p)))
           for x, ps in (("ang5", (4, 8)), ("ang7", (2, 4))) for m in ("cosine", "pearson") for p in ps}
ANG2 = {f"ang2-{m}-4": ("ang2", dict(metric=m)) for m in ("cosine", "pearson")}
UNSCALED = {f"{x}_x1-{m}-{p}": (x + "_x1", dict(metric=m, **_mp(p, p)))
            for x, p in (("ang5", 4), ("ang7", 4), ("ang2", 4), ("ang5", 8), ("ang7", 2)) for m in ("cosine", "pearson")}
# name: (case, [(level, key)] of the recorded exceptions)
ERRORS = {
    "d7-euclidean-9-5": (("d7", _mp(9, 5)), [(2, 5)]),
    "d5r-manhattan-2": (("d5r", dict(metric="manhattan", **_mp(2, 2))), [(4, 10)]),
    "d7r-manhattan-16-10": (("d7r", dict(metric="manhattan", processing_units=400, bubble_slices=3, **_mp(16, 10))),
                            [(1, 2)]),
    "skin3k-euclidean-32-4": (("skin3k", _mp(32, 4)), [(0, 0)]),
    "skin3k-euclidean-17-4": (("skin3k", _mp(17, 4)), [(0, 0)]),
}
# name: (case, the oracle's ValueError)
NON_TREE = {
    "grid7-euclidean-4": (("grid7", {}), "not a spanning tree"),
    "n2-euclidean-4": (("n2", {}), "not a spanning tree"),
    "ang5_zero-cosine-4": (("ang5_zero", dict(metric="cosine")), "the edges contain a cycle"),
    "ang5_zero-pearson-4": (("ang5_zero", dict(metric="pearson")), "the edges contain a cycle"),
}
# name: (case, the oracle's ValueError or None)
OVERLAP = {
    "ov7-euclidean-8": (("ov7", _mp(8, 8)), "not a spanning tree"),
    "ov7-manhattan-4": (("ov7", dict(metric="manhattan")), "not a spanning tree"),
    "ov7-supremum-4": (("ov7", dict(metric="supremum")), "not a spanning tree"),
    "ovang7-cosine-4": (("ovang7", dict(metric="cosine")), None),
    "ovang7-cosine-8": (("ovang7", dict(metric="cosine", **_mp(8, 8))), "not a spanning tree"),
    "ovang7-pearson-4": (("ovang7", dict(metric="pearson")), None),
    "ovang5-cosine-8": (("ovang5", dict(metric="cosine", **_mp(8, 8))), None),
}
DUPLICATES = {"ang5_dup-cosine-4": ("ang5_dup", dict(metric="cosine"))}
TINY = {f"tiny{n}-{m}-4": (f"tiny{n}", dict(metric=m)) for n in (1, 5, 50, 51) for m in ("euclidean", "cosine")}

CASES = {**RECURSING, **ANGULAR, **ANG2, **UNSCALED, **{k: v[0] for k, v in ERRORS.items()},
         **{k: v[0] for k, v in NON_TREE.items()}, **DUPLICATES, **TINY, **{k: v[0] for k, v in OVERLAP.items()}}
# name: the ValueError of the oracle's flat labels
FLAT_ERRORS = {**{k: v[1] for k, v in NON_TREE.items()}, **{k: v[1] for k, v in OVERLAP.items() if v[1]}}
# the device runs: everything but the scale-1 angular inputs, which are on the CPU side only to show
# why they are not enough (one forced leaf, as test_driver_cosine_forced_leaf_above_4096)
DEVICE_CASES = [k for k in CASES if k not in UNSCALED]
# default run + the driver variants that must not change the result
VARIANT_CASES = ["ang5-cosine-4", "d7r-manhattan-8", "d5r-euclidean-2"]
BORUVKA_CASES = ["ang5-cosine-4", "ang5-pearson-4", "d7r-manhattan-8", "d7r-euclidean-8", "d7r-supremum-8"]


def keywords(name, **over):
    """the oracle's keywords of a case (DEFAULTS filled in), with overrides"""
    return {**DEFAULTS, **CASES[name][1], **over}


def recurses(s):
    return s["iterations"] >= 5 and max(s["big"]) >= 2


@functools.lru_cache(maxsize=None)
def _oracle_run(name, over):
    from oracle import mr_driver as M
    from oracle.flat_labels import flat_labels
    X = input_of(CASES[name][0])
    kw = keywords(name, **dict(over))
    out = M.run(X, flat=False, **kw)
    err = None
    if kw.get("all_inter_edges", True):  # what M.run(flat=True) does, kept apart so that a raise keeps the edges
        try:
            out["labels"], out["n_clusters"] = flat_labels(X.shape[0], *out["edges"], kw["min_cl_size"])
            out["labels"].setflags(write=False)
        except ValueError as e:
            err = str(e)
    for a in out["edges"] + (out["leaf_of"],):
        a.setflags(write=False)
    return out, err


def oracle_run(name, **over):
    """(the oracle's run, None), or (its flat=False run, the ValueError's text) where the flat labels
    raise.  Computed once per process; the arrays are read-only."""
    return _oracle_run(name, tuple(sorted(over.items())))


def structure(name):
    """what a case is made of, as plain Python values (the literals of test_driver_cases.py)"""
    out, err = oracle_run(name)
    w = out["edges"][2]
    return dict(iterations=out["iterations"], big=[len(L["big"]) for L in out["levels"]],
                leaves=[len(L["leaves"]) for L in out["levels"]],
                model_errors=[(L["iteration"], k, c) for L in out["levels"]
                              for k, c in sorted(L.get("model_errors", {}).items())],
                edges=int(w.shape[0]), negative=int((w < 0).sum()), zero=int((w == 0).sum()),
                max=int((w == JMAX).sum()), distinct=int(np.unique(w).shape[0]), flat_error=err)


@functools.lru_cache(maxsize=None)
def filter_rows(name):
    """per level that has a big subset: the rows for which a nearest-sample scan over ALL the level's
    samples ends at a sample of another subset (strictly nearer, or as near and earlier in the
    list).  Where every entry is 0 the run does not depend on the key filter.  The subsets are
    replayed from the oracle run's bubble labels and induced keys; rows without a candidate are not
    counted."""
    from oracle import mr_driver as M
    from oracle import oracle as O
    out, _ = oracle_run(name)
    kw = keywords(name)
    X = input_of(CASES[name][0])
    n = X.shape[0]
    key_of = np.zeros(n, np.int64)
    res = []
    for L in out["levels"]:
        if not L["big"]:
            break
        rows_all, s_rows, owner_s, owner_x = [], [], [], []
        new_key = key_of.copy()
        for i, (c, cnt) in enumerate(sorted(L["big"].items())):
            rows = np.flatnonzero(key_of == c)
            assert rows.shape[0] == cnt
            sp = M.sample_ids(cnt, kw["k"], kw.get("samples_per_subset"), 20210101, L["iteration"], c)
            near = O.nearest_sample(X[rows], X[rows[sp]], kw["metric"])[0]
            used = np.unique(near)
            pos = np.full(sp.shape[0], -1)
            pos[used] = np.arange(used.shape[0])
            induced = dict(zip(sorted(set(L["labels"][c].tolist())), L["new_keys"][c]))
            new_key[rows] = np.array([induced[int(x)] for x in L["labels"][c]])[pos[near]]
            rows_all.append(rows)
            s_rows.append(rows[sp])
            owner_s += [i] * sp.shape[0]
            owner_x += [i] * cnt
        for c in L["leaves"]:
            key_of[key_of == c] = -1 - c
        R, S = np.concatenate(rows_all), np.concatenate(s_rows)
        u, du = O.nearest_sample(X[R], X[S], kw["metric"])
        res.append(int(((np.array(owner_s)[u] != np.array(owner_x)) & (du < JMAX)).sum()))
        key_of = np.where(np.isin(np.arange(n), R), new_key, key_of)
    assert np.array_equal(np.where(key_of < 0, -1 - key_of, key_of), out["leaf_of"])  # the replay is the run
    return res
