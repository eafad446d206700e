"""Inputs for the k-NN paths of high dimensions (16 < d: K1m, csrc/knn_mfma.hip, and the FP64 scan
knn_generic_kernel, csrc/knn.hip) on which K1m's rounding-error bound is thinnest: whole-data-set
ties, a centring that leaves nothing or almost nothing, rows far below the scale, squared
distances that underflow or overflow, a scale or its square outside the double range (on either
side: +inf, and 0 while distances are still finite), a candidate
order that fills a log with entries a compaction can drop, NaN and infinite rows.  Named, seeded,
read-only arrays; plain numpy, no device.  hd_family(name, d, n=1500) -> X.  n = 1500 pads to
1,536 rows (3 x 512, 12 query groups of 128): more than one workgroup and a ragged tail; ROWS
holds the row count each family is used at.  Rows are shuffled, except in `descending`, whose row
order is the point."""
import functools

import numpy as np

# K1m must run on these and equal the oracle
FINITE = ["same", "two_values", "zeros", "lattice", "one_hot", "last_col", "late_cols", "offset9", "offset15",
          "tiny", "subnormal_s", "below_sc2", "denormal", "huge", "above_sc2", "mixed_huge", "max_range",
          "descending", "wide_range"]
# the FP64 scan answers (include/hdbmi.h)
NONFINITE = ["nan_row", "nan_rows", "inf_rows", "inf_pair"]
FAMILIES = FINITE + NONFINITE
# more candidates tie at or below every row's k-th distance than a log holds, whatever k
ALL_TIE = ["same", "zeros", "two_values"]
SCALES = {"tiny": 1e-170, "subnormal_s": 1e-160, "below_sc2": 1e-156, "denormal": 1e-310, "huge": 1e160,
          "above_sc2": 2e154}
# The dimensions a family runs at: 17 (one column past the exact kernels, DP 32), 33 (DP 64, one
# column alone in the second 32-column chunk) and one of 129 (DP 256, one column past DP 128) or
# 256 (DP 256 full); the O(n^2 d) oracle decides how many families take the larger one.
_AT_256 = {"same", "one_hot", "offset9", "denormal", "mixed_huge", "descending", "late_cols"}
DIMS = {name: [17, 33, 256 if name in _AT_256 else 129] for name in FINITE}
DIMS["last_col"] = [33, 129]  # d mod 32 = 1: the varying column sits alone in its padded chunk
# Subnormal products cost a CPU a microcode assist each (the oracle takes 3.4 s per call at 1,500 x
# 33 on these two, against 0.06 s on normal numbers): they run at 520 rows (1,024 padded: five
# query groups, a ragged tail)
SLOW = ["subnormal_s", "below_sc2"]
ROWS = {name: 520 if name in SLOW else 1500 for name in FAMILIES}
CORE_DIMS = {name: [33, DIMS[name][-1]] for name in FINITE}  # core distances: d = 33 and the large one


def scan_rows(name, d):
    """rows of the FP64-scan cases: the oracle is O(n^2 d), so fewer rows at d = 256 and 257 (still
    three blocks of 256 queries and two candidate chunks; two blocks for the SLOW families)"""
    return ROWS[name] if d <= 33 else (260 if name in SLOW else 700)


NOTES = {
    "same": "every row equal to one row of non-dyadic values: the column mean need not equal the value",
    "two_values": "two distinct rows, each repeated n/2 times",
    "zeros": "the all-zero matrix: max |x - mu| = 0",
    "lattice": "integer grid in the first 3 columns, the others constant",
    "one_hot": "row i = e_(i mod d): every distinct pair at sqrt 2, twins at 0",
    "last_col": "only column d-1 varies (rounded normal * 30), the others constant",
    "late_cols": "the first half of the columns constant, the second half rounded blobs",
    "offset9": "1e9 + uniform * 1e-6: a few ulps of spread",
    "offset15": "1e15 + small integers",
    "tiny": "uniform * 1e-170: every squared distance underflows to 0",
    "subnormal_s": "uniform * 1e-160: squared distances are non-zero subnormals; scale^2 > DBL_MAX",
    "below_sc2": "uniform * 1e-156, just under 2^-512: subnormal squares of eight more digits; scale^2 still > DBL_MAX",
    "denormal": "uniform * 1e-310: subnormal coordinates; the power-of-two scale itself exceeds DBL_MAX",
    "huge": "uniform * 1e160: every squared distance overflows, the lists are all Double.MAX_VALUE",
    "above_sc2": "uniform * 2e154: max |x - mu| above 2^512, scale^2 below DBL_MIN",
    "mixed_huge": "unit rows plus 10 rows * 1e200: the unit rows vanish beside the scale",
    "max_range": "unit rows plus two rows at +-1.7e308 in one column",
    "wide_range": "uniform * 1e150 plus five rows * 1e13 and their negations: max |x - mu| in [2^537, 2^562), where "
                  "scale^2 rounds to 0 while the squared distances among the other rows are finite",
    "descending": "unshuffled; row i = (n - i) u + 1e-3 noise: every row is closer to the last rows than all before it",
    "nan_row": "blobs, one NaN coordinate",
    "nan_rows": "blobs, NaN coordinates in three rows",
    "inf_rows": "unit rows, one all-+inf row, one row with a single -inf coordinate: no NaN pair",
    "inf_pair": "two rows with +inf in the same column: their pair is NaN, every other pair of theirs +inf",
}


def special_rows(name, n):
    """rows holding the NaN or infinite coordinates, placed as tests/degenerate_inputs.py places
    them at n = 2000 (rows 700; 5, 1000, 1990; n/3, 2n/3; 400, 1600), scaled to n"""
    return {"nan_row": [(7 * n) // 20], "nan_rows": [min(5, n - 1), n // 2, n - 1 - n // 200],
            "inf_rows": [n // 3, (2 * n) // 3], "inf_pair": [n // 5, (4 * n) // 5]}[name]


def _unit(n, d, rng):
    return rng.uniform(-1.0, 1.0, size=(n, d))


def _blobs(n, d, rng):
    C = rng.uniform(-50.0, 50.0, size=(5, d))
    return C[rng.integers(0, 5, n)] + rng.normal(0, 1.0, size=(n, d))


def _const_row(d):
    return np.resize(np.array([0.1, -7.3, 2.7, 1e-3, 41.9, -0.3, 1.1]), d)


def _make(name, d, n, rng):
    if name == "same":
        return np.tile(_const_row(d), (n, 1))
    if name == "two_values":
        A, B = _const_row(d), _const_row(d)[::-1] * 1.7 + 0.2
        return np.where((rng.permutation(n) < n // 2)[:, None], A, B)
    if name == "zeros":
        return np.zeros((n, d))
    if name == "lattice":
        s = int(np.ceil(n ** (1.0 / 3.0)))
        g = np.stack(np.meshgrid(*[np.arange(s, dtype=np.float64)] * 3, indexing="ij"), -1).reshape(-1, 3)
        X = np.tile(_const_row(d), (n, 1))
        X[:, :3] = g[rng.permutation(g.shape[0])[:n]]
        return X
    if name == "one_hot":
        X = np.zeros((n, d))
        X[np.arange(n), np.arange(n) % d] = 1.0
        return X[rng.permutation(n)]
    if name == "last_col":
        X = np.tile(np.arange(d, dtype=np.float64), (n, 1))
        X[:, d - 1] = np.round(rng.normal(0, 30.0, n), 1)
        return X
    if name == "late_cols":
        X = np.tile(np.arange(d, dtype=np.float64), (n, 1))
        X[:, d // 2:] = np.round(_blobs(n, d - d // 2, rng), 1)
        return X
    if name == "offset9":
        return 1e9 + _unit(n, d, rng) * 1e-6
    if name == "offset15":
        return 1e15 + rng.integers(-8, 9, size=(n, d)).astype(np.float64)
    if name in SCALES:
        return _unit(n, d, rng) * SCALES[name]
    if name == "mixed_huge":
        X = _unit(n, d, rng)
        X[rng.choice(n, min(10, n), replace=False)] *= 1e200
        return X
    if name == "max_range":
        X = _unit(n, d, rng)
        X[(3 * n) // 20, 1], X[(3 * n) // 4, 1] = 1.7e308, -1.7e308
        return X
    if name == "wide_range":
        X = _unit(n, d, rng) * 1e150
        r = rng.choice(n, 10, replace=False)
        X[r[:5]] *= 1e13
        X[r[5:]] = -X[r[:5]]  # symmetric: the column means stay at the small rows' scale
        return X
    if name == "descending":
        u = rng.normal(size=d)
        u /= np.linalg.norm(u)
        return (n - np.arange(n, dtype=np.float64))[:, None] * u + 1e-3 * rng.normal(size=(n, d))
    rows = special_rows(name, n)
    if name in ("nan_row", "nan_rows"):
        X = _blobs(n, d, rng)
        for k, r in enumerate(rows):
            X[r, (k * 11) % d] = np.nan
        return X
    X = _unit(n, d, rng)
    if name == "inf_rows":
        X[rows[0]] = np.inf
        X[rows[1], d - 1] = -np.inf
        return X
    if name == "inf_pair":
        X[rows[0], 0] = X[rows[1], 0] = np.inf
        return X
    raise KeyError(name)


@functools.lru_cache(maxsize=None)
def hd_family(name, d, n=1500):
    assert d > 16, d
    rng = np.random.default_rng([2000 + FAMILIES.index(name), d, n])
    X = np.ascontiguousarray(_make(name, d, n, rng), np.float64)
    assert X.shape == (n, d)
    X.setflags(write=False)
    return X


def numpy_sq_rows(X, rows):
    """squared distances of the given rows to all rows in the reference's order
    (EuclideanDistance.java:31-33): s = s + t * t over the dimensions, every operation rounded
    once.  Returns (len(rows), n)."""
    Q = X[rows]
    s = np.zeros((Q.shape[0], X.shape[0]))
    with np.errstate(over="ignore", under="ignore", invalid="ignore"):
        for j in range(X.shape[1]):
            t = Q[:, j:j + 1] - X[None, :, j]
            s = s + t * t
    return s


def numpy_knn_rows(X, rows, k, excl_self):
    """the k smallest distances of the given rows, ascending, Double.MAX_VALUE padded: the strict
    '<' insertion into a Double.MAX_VALUE buffer (HDBSCANStar.java:84-97) keeps exactly the values
    below Double.MAX_VALUE (never NaN, never +inf)"""
    jmax = np.finfo(np.float64).max
    with np.errstate(invalid="ignore"):
        dist = np.sqrt(numpy_sq_rows(X, rows))
        dist = np.where(dist < jmax, dist, jmax)  # NaN and +inf: not below the initial value
    if excl_self:
        dist[np.arange(len(rows)), rows] = jmax
    dist = np.concatenate([dist, np.full((len(rows), k), jmax)], axis=1)  # fewer than k candidates: padding
    return np.sort(dist, axis=1)[:, :k]


@functools.lru_cache(maxsize=None)
def hd_lists(name, d, n=None):
    """(X, the oracle's 31-NN lists with self, without self), computed once per process.  The
    k-NN list of a smaller k is the first k columns (the strict insertion keeps the k smallest
    values in ascending order; tests/test_highdim_inputs.py checks the prefix property on the
    oracle itself)."""
    from oracle import oracle as O
    O.lib()
    X = hd_family(name, d, n or ROWS[name])
    out = tuple(O.knn_lists(X, 32, excl_self=e) for e in (False, True))
    for a in out:
        a.setflags(write=False)
    return (X,) + out


@functools.lru_cache(maxsize=None)
def hd_core(name, d, mp, sem, n=None):
    from oracle import oracle as O
    O.lib()
    c = O.core_distances(hd_family(name, d, n or ROWS[name]), mp, semantics=sem)
    c.setflags(write=False)
    return c
