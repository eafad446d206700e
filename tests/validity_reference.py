"""A plain restatement of the contract of hdb_validity_index (include/hdbmi.h): the DBCV validity
index of a labelling.  CPU only.

Every distance comes from the oracle (metric_kruskal.pair_distances, one orc_distance call per pair),
the per-cluster tree from metric_kruskal.kruskal_mst_metric, the real-exponent power from math.pow
(the host libm the library calls).  The sums are written out in the contract's shape: blocks of
SUM_BLOCK consecutive members, a block's partial from 0.0 in member order, the total from 0.0 over
the block partials in block order.  The loops run over candidate columns; every addition,
multiplication and division is one elementwise IEEE operation over the queries (no numpy ``**`` or
np.power, which may go to a vector library whose last bit differs from libm's)."""
import math

import numpy as np

from metric_kruskal import kruskal_mst_metric, pair_distances

SUM_BLOCK = 512


def dist_matrix(X, metric):
    """the symmetric n x n matrix of oracle distances (diagonal 0, never read)"""
    X = np.ascontiguousarray(X, np.float64)
    n = X.shape[0]
    D = np.zeros((n, n), np.float64)
    if n >= 2:
        iu = np.triu_indices(n, 1)
        v = pair_distances(X, metric)
        D[iu] = v
        D.T[iu] = v
    return D


def powi(t, d):
    """t^d by right-to-left binary exponentiation, elementwise"""
    r, b, e = np.ones_like(t), t.copy(), int(d)
    while e:
        if e & 1:
            r = r * b
        e >>= 1
        if e:
            b = b * b
    return r


def blocked_totals(p, contributes, block=SUM_BLOCK):
    """per query (row) the two-level sum of the contributing p over the candidate columns"""
    nc = p.shape[0]
    total = np.zeros(nc, np.float64)
    for b0 in range(0, nc, block):
        partial = np.zeros(nc, np.float64)
        for j in range(b0, min(b0 + block, nc)):
            partial = np.where(contributes[:, j], partial + p[:, j], partial)
        total = total + partial
    return total


def plain_totals(p, contributes):
    """the same pairs summed left to right in one run (what the contract does NOT do)"""
    return blocked_totals(p, contributes, block=p.shape[0] + 1)


def apts_cores(Dc, d):
    """all-points core distances of one cluster from its members' distance matrix"""
    nc = Dc.shape[0]
    if nc <= 1:
        return np.zeros(nc, np.float64)
    with np.errstate(all="ignore"):
        contributes = (Dc > 0) & ~np.eye(nc, dtype=bool)  # NaN > 0 is False
        p = powi(1.0 / Dc, d)
        total = blocked_totals(p, contributes)
    out = np.zeros(nc, np.float64)
    for i, t in enumerate(total.tolist()):
        if t == 0.0:
            continue
        try:
            out[i] = math.pow(t / float(nc - 1), -1.0 / d)
        except OverflowError:  # libm returns +inf where Python raises
            out[i] = math.inf
    return out


def validity_reference(X, labels, K, metric="euclidean", D=None):
    """dict of index, validity, sparseness, separation, nearest_cluster, size (K each), core, internal
    (n each); D: dist_matrix(X, metric) when the caller shares it between labellings"""
    X = np.ascontiguousarray(X, np.float64)
    labels = np.asarray(labels, np.int64)
    n, d = X.shape
    assert labels.shape == (n,) and (n == 0 or (labels.min() >= 0 and labels.max() <= K))
    if D is None:
        Xl = X.copy()
        Xl[labels == 0] = 0.0  # noise rows are never read as coordinates
        D = dist_matrix(Xl, metric)
    core = np.zeros(n, np.float64)
    internal = np.zeros(n, np.int32)
    size = np.zeros(K, np.int32)
    sparseness = np.zeros(K, np.float64)
    separation = np.full(K, np.inf)
    nearest = np.zeros(K, np.int32)
    validity = np.zeros(K, np.float64)
    members = [np.flatnonzero(labels == c) for c in range(K + 1)]
    for c in range(1, K + 1):
        idx = members[c]
        nc = idx.shape[0]
        size[c - 1] = nc
        if nc == 0:
            continue
        core[idx] = apts_cores(D[np.ix_(idx, idx)], d)
        if nc == 1:
            internal[idx] = 1
            continue
        lo, hi, w = kruskal_mst_metric(X[idx], core[idx], metric)
        deg = np.bincount(np.concatenate([lo, hi]), minlength=nc)
        inner = deg >= 2
        inner_edge = inner[lo] & inner[hi]
        if not inner_edge.any():
            inner[:] = True
            inner_edge[:] = True
        internal[idx] = inner
        sparseness[c - 1] = max(w[inner_edge].tolist())
    for c in range(1, K + 1):
        xs = members[c][internal[members[c]] == 1]
        best_w, best_l = math.inf, 0
        for c2 in range(1, K + 1):
            ys = members[c2][internal[members[c2]] == 1]
            if c2 == c or xs.shape[0] == 0 or ys.shape[0] == 0:
                continue
            with np.errstate(invalid="ignore"):
                W = D[np.ix_(xs, ys)]
                cx, cy = core[xs][:, None], core[ys][None, :]
                W = np.where(cx > W, cx, W)
                W = np.where(cy > W, cy, W)
            W = W[~np.isnan(W)]
            if W.shape[0] == 0:
                continue
            m = float(W.min())
            if best_l == 0 or m < best_w:  # labels ascend: an equal value keeps the smaller label
                best_w, best_l = m, c2
        if best_l:
            separation[c - 1], nearest[c - 1] = best_w, best_l
    index = 0.0
    for c in range(K):
        sep, sp = float(separation[c]), float(sparseness[c])
        mx = sep if sep > sp else sp
        v = 0.0
        if size[c] > 0 and sep != math.inf and mx != 0.0:
            v = (sep - sp) / mx
        validity[c] = v
        index = index + (float(size[c]) / float(n)) * v
    return dict(index=index, validity=validity, sparseness=sparseness, separation=separation,
                nearest_cluster=nearest, size=size, core=core, internal=internal)


# ------------------------------------------------------------------------------- labellings
def generating_labels(family, n, d, seed=0):
    """the blob / direction of every row of metric_kruskal.rounded_blobs(n, d, seed) or rays(n, d),
    1..6: the same generator replayed up to the draw of the assignment"""
    if family == "rounded_blobs":
        rng = np.random.default_rng(4000 + 31 * d + n + seed)
        rng.uniform(-10.0, 10.0, size=(6, d))
    else:
        rng = np.random.default_rng(5000 + 31 * d + n)
        rng.uniform(0.5, 2.0, size=(6, d))
    return (rng.integers(0, 6, n) + 1).astype(np.int32)


def with_noise(labels, share=0.1, seed=1):
    """about `share` of the rows set to 0"""
    rng = np.random.default_rng(seed)
    out = np.array(labels, np.int32)
    out[rng.random(out.shape[0]) < share] = 0
    return out


def random_labels(n, K, seed=2):
    return np.random.default_rng(seed).integers(0, K + 1, n).astype(np.int32)
