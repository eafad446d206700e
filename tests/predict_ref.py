"""The brute-force restatement of out-of-sample prediction (hdb_attach_points and
hdb_predict_labels, include/hdbmi.h).  CPU only.

attach_ref(X, core, Q, min_pts, metric): every pair distance comes from the oracle's orc_distance
(the query row first), one call per pair, as tests/metric_kruskal.py calls it.  A query's list is
built by strict '<' insertion into a Double.MAX_VALUE buffer of K = min_pts - 1 entries; core_q is
its last entry.  w starts as the distance and is replaced by core_q, then by core[j], on a strict
'>' only (a -0.0 core reads as +0.0); nearest is the first row under (w, s, j) among the pairs whose
w is not NaN, s being the squared distance summed in dimension order for Euclidean and the distance
itself otherwise; no such pair gives (-1, Double.MAX_VALUE).

predict_ref(tree, nearest, level, flat_label): the tree walk as a plain loop."""
import bisect

import numpy as np

from metric_kruskal import _orc_distance

JMAX = float(np.finfo(np.float64).max)


def cross_distances(Q, X, metric):
    """oracle.distance(Q[i], X[j], metric) as an (m, n) array"""
    Q, X = np.ascontiguousarray(Q, np.float64), np.ascontiguousarray(X, np.float64)
    (m, d), n = Q.shape, X.shape[0]
    f, codes = _orc_distance()
    c = codes[metric]
    out = np.empty((m, n), np.float64)
    xs = [X.ctypes.data + j * X.strides[0] for j in range(n)]
    for i in range(m):
        qi = Q.ctypes.data + i * Q.strides[0]
        out[i] = [f(qi, xj, d, c) for xj in xs]
    return out


def insert_list(row, K):
    """HDBSCANStar.java:79-97: the K smallest by strict '<' insertion, Double.MAX_VALUE padded"""
    buf = [JMAX] * K
    for x in row.tolist():
        if x < buf[-1]:  # false for NaN and for anything not below MAX_VALUE
            bisect.insort_right(buf, x)
            buf.pop()
    return buf


def attach_ref(X, core, Q, min_pts, metric="euclidean"):
    X, Q = np.ascontiguousarray(X, np.float64), np.ascontiguousarray(Q, np.float64)
    core = np.ascontiguousarray(core, np.float64) + 0.0  # -0.0 + 0.0 == +0.0; NaN stays NaN
    (m, d), n = Q.shape, X.shape[0]
    K = min_pts - 1
    D = cross_distances(Q, X, metric)
    core_q = np.array([insert_list(D[i], K)[K - 1] if K > 0 else 0.0 for i in range(m)], np.float64).reshape(m)
    nearest, level = np.full(m, -1, np.int32), np.full(m, JMAX, np.float64)
    jj = np.arange(n)
    with np.errstate(all="ignore"):
        for i in range(m):
            if metric == "euclidean":
                s = np.zeros(n)
                for k in range(d):
                    t = Q[i, k] - X[:, k]
                    s = s + t * t
            else:
                s = D[i]
            w = D[i].copy()
            w = np.where(core_q[i] > w, core_q[i], w)  # strict '>': a NaN is never taken, a NaN w never replaced
            w = np.where(core > w, core, w)
            ok = np.flatnonzero(~np.isnan(w))
            if ok.shape[0] == 0:
                continue
            best = ok[np.lexsort((jj[ok], s[ok], w[ok]))[0]]  # numeric: negatives first, -0.0 == +0.0
            nearest[i], level[i] = best, w[best]
    return core_q, nearest, level


def predict_ref(tree, nearest, level, flat_label=None):
    """(tree_label, labels, scores) of hdb_predict_labels over a host ClusterTree"""
    parent, birth, death = (np.asarray(getattr(tree, k)) for k in ("parent", "birth", "death"))
    flat = np.asarray(tree.flat_label if flat_label is None else flat_label)
    pc, pl = np.asarray(tree.point_cluster), np.asarray(tree.point_level)
    K = parent.shape[0]
    eps_max = [JMAX, JMAX] + [float(x) for x in death[1:]]  # by tree label; the root: its descendants only
    for c in range(K, 1, -1):
        p = int(parent[c - 1])
        eps_max[p] = min(eps_max[p], eps_max[c])
    m = len(nearest)
    tl, lab, sc = np.zeros(m, np.int32), np.zeros(m, np.int32), np.ones(m, np.float64)
    with np.errstate(all="ignore"):
        for i in range(m):
            y = int(nearest[i])
            if y < 0:
                continue
            e = np.float64(level[i])
            C = int(pc[y])
            while birth[C - 1] <= e:  # NaN for the root: stops
                C = int(parent[C - 1])
            tl[i] = C
            S = C
            while S > 0 and flat[S - 1] == 0:
                S = int(parent[S - 1])
            lab[i] = flat[S - 1] if S > 0 else 0
            eps = max(e, np.float64(pl[y]))
            sc[i] = 0.0 if eps == 0 else np.float64(1.0) - np.float64(eps_max[C]) / eps
    return tl, lab, sc
