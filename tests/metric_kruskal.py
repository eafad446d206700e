"""The independent Kruskal reference of the exact MST for any metric (K2g, csrc/boruvka_generic.hip),
and the input families its tests share.  CPU only.

kruskal_mst_metric(X, core, metric): the unique minimum spanning tree of the mutual-reachability
graph under the strict total edge order (w, s, lo, hi) of include/hdbmi.h:
  w   the pair's distance, replaced by core_lo, then core_hi, on a strict '>' only
      (HDBSCANStar.java:162-168: a NaN core never raises a weight, a NaN distance stays NaN);
  s   Euclidean: the squared distance summed in dimension order (exactly path_helpers.kruskal_mst,
      which this function returns for that metric); every other metric: the distance itself;
  lo < hi the row indices.  A pair whose w is NaN is not an edge.
Every distance comes from the oracle's orc_distance (oracle.distance's function, bit-exact for the
five metrics), one call per pair -- through a prototype that takes row addresses, so the all-pairs
loop costs about a second at 1,500 rows.  The union-find is path_helpers.kruskal_mst's: the sorted
prefix is consumed in chunks and pairs inside one component are dropped after each chunk."""
import ctypes as C
import functools

import numpy as np

from path_helpers import _pairs, kruskal_mst

METRICS = ("manhattan", "supremum", "cosine", "pearson")


@functools.lru_cache(maxsize=1)
def _orc_distance():
    from oracle import oracle as O
    lib = O.lib()
    return C.CFUNCTYPE(C.c_double, C.c_void_p, C.c_void_p, C.c_int, C.c_int)(("orc_distance", lib)), O.METRICS


def pair_distances(X, metric):
    """oracle.distance(X[i], X[j], metric) for every pair i < j, in np.triu_indices order"""
    X = np.ascontiguousarray(X, np.float64)
    n, d = X.shape
    f, codes = _orc_distance()
    m = codes[metric]
    base, stride = X.ctypes.data, X.strides[0]
    out = np.empty(n * (n - 1) // 2, np.float64)
    k = 0
    for a in range(n - 1):
        pa = base + a * stride
        out[k:k + n - 1 - a] = [f(pa, base + b * stride, d, m) for b in range(a + 1, n)]
        k += n - 1 - a
    return out


def kruskal_mst_metric(X, core, metric="euclidean"):
    """(lo, hi, w) of the n - 1 tree edges in key order; ValueError "do not span: isolated rows
    [...]" (the rows outside the largest component) if the non-NaN pairs do not connect all rows"""
    if metric == "euclidean":
        return kruskal_mst(X, core)
    X = np.ascontiguousarray(X, np.float64)
    core = np.ascontiguousarray(core, np.float64)
    n = X.shape[0]
    i, j = _pairs(n)
    s = pair_distances(X, metric)
    with np.errstate(invalid="ignore"):
        w = s.copy()
        ci, cj = core[i], core[j]
        w = np.where(ci > w, ci, w)  # strict '>': a NaN core is never taken, a NaN w never replaced
        w = np.where(cj > w, cj, w)
    parent = list(range(n))

    def find(x):
        while parent[x] != x:
            parent[x] = parent[parent[x]]
            x = parent[x]
        return x

    out = []
    idx = np.flatnonzero(~np.isnan(w))
    while len(out) < n - 1:
        if idx.shape[0] == 0:
            root = np.fromiter((find(x) for x in range(n)), np.int64, n)
            big = np.bincount(root).argmax()
            raise ValueError("the non-NaN pairs do not span: isolated rows %s" % np.flatnonzero(root != big).tolist())
        take = min(idx.shape[0], 8 * n)
        wi = w[idx]
        sel = wi <= np.partition(wi, take - 1)[take - 1]  # whole tie groups: the rest is strictly heavier
        chunk, idx = idx[sel], idx[~sel]
        chunk = chunk[np.lexsort((j[chunk], i[chunk], s[chunk], w[chunk]))]  # numeric: negatives first, -0.0 == +0.0
        for e, a, b in zip(chunk.tolist(), i[chunk].tolist(), j[chunk].tolist()):
            ra, rb = find(a), find(b)
            if ra != rb:
                parent[rb] = ra
                out.append(e)
                if len(out) == n - 1:
                    break
        root = np.fromiter((find(x) for x in range(n)), np.int64, n)
        idx = idx[root[i[idx]] != root[j[idx]]]
    out = np.asarray(out, np.int64)
    return i[out].astype(np.int32), j[out].astype(np.int32), w[out]


# ------------------------------------------------------------------------------- input families
def rounded_blobs(n, d, seed=0):
    """Gaussian blobs rounded to one decimal: ties in w and in s"""
    rng = np.random.default_rng(4000 + 31 * d + n + seed)
    C_ = rng.uniform(-10.0, 10.0, size=(6, d))
    return np.round(C_[rng.integers(0, 6, n)] + rng.normal(0, 1.0, size=(n, d)), 1)


def rays(n, d):
    """rows k * u, u one of 6 positive directions, k uniform in [0.1, 10]: rows of one direction are
    positive multiples of one another, so their cosine and Pearson distances are 0 or a few ulps
    either side of it (negative ones included) and tie heavily.  No row has zero norm or zero
    variance."""
    rng = np.random.default_rng(5000 + 31 * d + n)
    U = rng.uniform(0.5, 2.0, size=(6, d))
    return U[rng.integers(0, 6, n)] * rng.uniform(0.1, 10.0, size=(n, 1))


def zero_row(n, d, pos=7):
    """rays with row pos (7 unless given) all zeros: its cosine distance to every row is NaN"""
    X = rays(n, d)
    X[pos] = 0.0
    return X


FAMILIES = {"rounded_blobs": rounded_blobs, "rays": rays, "zero_row": zero_row}
SHAPES = [(d, n) for d in (5, 24) for n in (65, 1500)]


@functools.lru_cache(maxsize=None)
def metric_case(metric, family, d, n, min_pts=4):
    """(X, oracle core distances, kruskal_mst_metric of them), computed once per process"""
    from oracle import oracle as O
    X = np.ascontiguousarray(FAMILIES[family](n, d), np.float64)
    core = O.core_distances(X, min_pts, metric=metric)
    lo, hi, w = kruskal_mst_metric(X, core, metric)
    for a in (X, core, lo, hi, w):
        a.setflags(write=False)
    return X, core, (lo, hi, w)
