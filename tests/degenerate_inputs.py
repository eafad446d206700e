"""Inputs on which the exact leaf's three arguments are thinnest -- the box lower bounds, the
strict total edge order (w, s, lo, hi), the Morton quantisation by the bounding-box span --
as named, seeded, read-only arrays: pure ties, zero spans, squared distances that underflow or
overflow, infinite and NaN rows.  Plain numpy, no device.  Rows are shuffled, so the input
order carries no structure; every family has at most about 3,100 rows (an all-pairs Kruskal
stays around a second).  family(name) -> (X, note); family(name, n) regenerates a family at
another size where that is defined."""
import functools

import numpy as np

SPANNING_FINITE = ["lattice3", "lattice2", "line1", "same", "two_values", "constcol", "line_in_8d", "late_dims16",
                   "offset", "tiny", "subnormal"]               # every weight finite
SPANNING_INF = ["huge", "mixed_huge", "max_range", "inf_rows", "inf_pair"]  # some or all weights +inf
NOT_SPANNING = ["nan_row", "nan_rows"]                            # a NaN row: only NaN pairs reach it
SPANNING = SPANNING_FINITE + SPANNING_INF
FAMILIES = SPANNING + NOT_SPANNING
NAN_ROWS = {"nan_row": [700], "nan_rows": [5, 1000, 1990]}


def _grid(shape, n, rng):
    g = np.stack(np.meshgrid(*[np.arange(s, dtype=np.float64) for s in shape], indexing="ij"), -1).reshape(-1, len(shape))
    return g[rng.permutation(g.shape[0])[:n]]


def _unit(n, d, rng):
    return rng.uniform(-1.0, 1.0, size=(n, d))


def _blobs(n, d, rng):
    C = rng.uniform(-50.0, 50.0, size=(5, d))
    return C[rng.integers(0, 5, n)] + rng.normal(0, 1.0, size=(n, d))


def _make(name, n, rng):
    if name == "lattice3":
        n = n or 16 * 16 * 12
        return _grid((16, 16, -(-n // 256)), n, rng), "integer grid, d = 3: one distinct weight, every edge ties in w and s"
    if name == "lattice2":
        return _grid((56, 55), n or 56 * 55, rng), "integer grid, d = 2"
    if name == "line1":
        n = n or 3000
        return rng.permutation(n).astype(np.float64)[:, None], "the integers 0..n-1, d = 1"
    if name == "same":
        return np.tile(np.array([1.5, -2.25, 7.0]), (n or 1500, 1)), "identical rows: every w and s is 0, only the ids decide"
    if name == "two_values":
        n = n or 2000
        X = np.where((np.arange(n) < n // 2)[:, None], np.array([0.25, 3.0]), np.array([10.5, -4.0]))
        return X[rng.permutation(n)], "half the rows are A, half are B"
    if name == "constcol":
        X = _blobs(n or 2500, 3, rng)
        X[:, 1] = 42.0
        return np.round(X, 1), "d = 3, the middle column constant (Morton span 0), rounded to 0.1"
    if name == "line_in_8d":
        X = np.tile(np.arange(8, dtype=np.float64), (n or 2000, 1))
        X[:, 5] = np.round(rng.normal(0, 30.0, n or 2000), 1)
        return X, "d = 8, one varying column"
    if name == "late_dims16":
        X = np.tile(np.arange(16, dtype=np.float64), (n or 2000, 1))
        X[:, 8:] = np.round(_blobs(n or 2000, 8, rng), 1)
        return X, "d = 16, columns 0-7 constant (every Morton key equal), columns 8-15 blobs"
    if name == "offset":
        return 1e9 + _unit(n or 2000, 3, rng) * 1e-6, "1e9 + uniform(-1, 1) * 1e-6: a few ulps of spread"
    if name == "tiny":
        return _unit(n or 2000, 3, rng) * 1e-170, "uniform * 1e-170: every s underflows to 0"
    if name == "subnormal":
        return _unit(n or 2000, 3, rng) * 1e-160, "uniform * 1e-160: s is subnormal (coarse ties)"
    if name == "huge":
        return _unit(n or 2000, 3, rng) * 1e160, "uniform * 1e160: every s overflows to +inf"
    if name == "mixed_huge":
        X = _unit(n or 2000, 3, rng)
        X[rng.choice(X.shape[0], 10, replace=False)] *= 1e200
        return X, "unit rows plus 10 rows * 1e200"
    if name == "max_range":
        X = _unit(n or 2000, 3, rng)
        X[300, 1], X[1500, 1] = 1.7e308, -1.7e308
        return X, "unit rows plus two rows at +-1.7e308 in one coordinate: the box span overflows"
    if name == "inf_rows":
        X = _unit(n or 2000, 3, rng)
        m = X.shape[0]
        X[m // 3] = np.inf
        X[(2 * m) // 3, 2] = -np.inf
        return X, "unit rows, one all-+inf row, one row with a single -inf coordinate: no NaN pair"
    if name == "inf_pair":
        X = _unit(n or 2000, 3, rng)
        X[400, 0] = X[1600, 0] = np.inf
        return X, "two rows with +inf in the same coordinate: their pair is NaN, every other pair of theirs +inf"
    if name in NAN_ROWS:
        X = _blobs(n or 2000, 3, rng)
        for k, r in enumerate(NAN_ROWS[name]):
            X[r, k % 3] = np.nan
        return X, "blobs with NaN coordinates in rows %s" % NAN_ROWS[name]
    raise KeyError(name)


@functools.lru_cache(maxsize=None)
def family(name, n=None):
    X, note = _make(name, n, np.random.default_rng(1000 + FAMILIES.index(name)))
    X = np.ascontiguousarray(X, np.float64)
    assert X.shape[0] <= 3100 or n is not None
    X.setflags(write=False)
    return X, note


# (minPts, core semantics) of the MST cases: the live cumulative cores at 4, EXCL_SELF at 2
MST_SETTINGS = [(2, 2), (4, 0)]


@functools.lru_cache(maxsize=None)
def family_case(name, mp, sem):
    """(X, oracle core distances, kruskal_mst of them), computed once per process"""
    from oracle import oracle as O
    from path_helpers import kruskal_mst
    O.lib()
    X, _ = family(name)
    core = O.core_distances(X, mp, semantics=sem)
    lo, hi, w = kruskal_mst(X, core)
    for a in (core, lo, hi, w):
        a.setflags(write=False)
    return X, core, (lo, hi, w)
