"""The plain restatement of soft clustering (hdb_exemplars, hdb_exemplar_distances and
hdb_membership_vectors; the contract is in include/hdbmi.h).  CPU only.

Every distance comes from the oracle's orc_distance through predict_ref.cross_distances (the query
row first, one call per pair).  Leaves, the nearest selected cluster, eps_max and every LCA are
plain Python walks over the parent array: no binary lifting, no depth table.  Every sum over
clusters is a Python loop in ascending flat label over numpy float64 scalars: one IEEE operation
per step, no vectorised reduction."""
import numpy as np

from predict_ref import JMAX, cross_distances

INF = float("inf")
F = np.float64


def tree_arrays(tree, flat_label=None):
    parent, birth, death = (np.asarray(getattr(tree, k)) for k in ("parent", "birth", "death"))
    flat = np.asarray(tree.flat_label if flat_label is None else flat_label)
    return parent, birth, death, flat


def exemplars_ref(tree, flat_label=None, C=None):
    """(ids int32, offsets int64[C + 1]) of hdb_exemplars over a host ClusterTree"""
    parent, _, _, flat = tree_arrays(tree, flat_label)
    pc, pl = np.asarray(tree.point_cluster), np.asarray(tree.point_level)
    K, n = parent.shape[0], pc.shape[0]
    if C is None:
        C = int(flat.max()) if K else 0
    has_child = [False] * (K + 1)
    for c in range(1, K + 1):
        has_child[int(parent[c - 1])] = True
    low = [INF] * (K + 1)
    for x in range(n):
        if pl[x] < low[int(pc[x])]:  # false for NaN
            low[int(pc[x])] = float(pl[x])
    segs = [[] for _ in range(C + 1)]
    for x in range(n):
        c = int(pc[x])
        if has_child[c] or not (pl[x] == low[c]):
            continue
        s = c
        while s > 0 and flat[s - 1] == 0:
            s = int(parent[s - 1])
        f = int(flat[s - 1]) if s > 0 else 0
        if f > 0:
            segs[f].append(x)
    ids = [x for f in range(1, C + 1) for x in segs[f]]
    offsets = np.zeros(C + 1, np.int64)
    for f in range(1, C + 1):
        offsets[f] = offsets[f - 1] + len(segs[f])
    return np.asarray(ids, np.int32).reshape(-1), offsets


def min_by_segment(D, offsets):
    """dmin (m x C) from the distances D (m x E) to the exemplars: the minimum under '<' from +inf
    (a NaN is never taken), a zero stored as +0.0"""
    m, C = D.shape[0], offsets.shape[0] - 1
    out = np.full((m, C), INF)
    for i in range(m):
        row = D[i].tolist()
        for f in range(C):
            best = INF
            for e in range(int(offsets[f]), int(offsets[f + 1])):
                if row[e] < best:
                    best = row[e]
            out[i, f] = 0.0 if best == 0 else best
    return out


def exemplar_distances_ref(X, ids, offsets, Q, metric="euclidean"):
    X, Q = np.ascontiguousarray(X, np.float64), np.ascontiguousarray(Q, np.float64)
    ids = np.asarray(ids, np.int64)
    if ids.shape[0] == 0:
        return np.full((Q.shape[0], offsets.shape[0] - 1), INF)
    return min_by_segment(cross_distances(Q, np.ascontiguousarray(X[ids]), metric), np.asarray(offsets))


def eps_max_ref(parent, death):
    """by tree label (index 0 unused): the subtree minimum of death; the root: its descendants only"""
    K = parent.shape[0]
    em = [JMAX, JMAX] + [float(x) for x in death[1:]]
    for c in range(K, 1, -1):
        p = int(parent[c - 1])
        if p > 0:
            em[p] = min(em[p], em[c])
    return em


def merge_birth_ref(parent, birth, a, c):
    """B(c) for anchor a >= 1: -inf when a is c or below it, else the birth of the child of
    LCA(a, c) on the way to c"""
    anc_a = set()
    x = a
    while x > 0:
        anc_a.add(x)
        x = int(parent[x - 1])
    prev, cur = 0, c
    while cur > 0 and cur not in anc_a:
        prev, cur = cur, int(parent[cur - 1])
    return F(-INF) if prev == 0 else F(birth[prev - 1])


def membership_ref(tree, anchor, level, dmin, flat_label=None, C=None):
    """(vectors m x C, prob, labels) of hdb_membership_vectors over a host ClusterTree"""
    parent, birth, death, flat = tree_arrays(tree, flat_label)
    K = parent.shape[0]
    dmin = np.asarray(dmin, np.float64)
    m = len(anchor)
    if C is None:
        C = dmin.shape[1]
    em = eps_max_ref(parent, death)
    sel = [0] * (C + 1)
    for c in range(K, 0, -1):
        if flat[c - 1] > 0:
            sel[int(flat[c - 1])] = c
    vec, prob, lab = np.zeros((m, C)), np.zeros(m), np.zeros(m, np.int32)
    one, zero = F(1.0), F(0.0)
    with np.errstate(all="ignore"):
        for i in range(m):
            a, l = int(anchor[i]), F(level[i])
            if a == 0:
                continue
            t = []
            for f in range(1, C + 1):
                c = sel[f]
                if c == 0:
                    t.append(zero)
                    continue
                B = merge_birth_ref(parent, birth, a, c)
                M = B if B > l else l
                t.append(one if M == 0 else F(em[c]) / M)
            mx = zero
            for x in t:
                if x > mx:
                    mx = x
            pr = one if one < mx else mx
            d = [F(x) for x in dmin[i]]
            Z = [f for f in range(C) if d[f] <= 0]
            if Z:
                dv = [one / F(len(Z)) if f in Z else zero for f in range(C)]
            else:
                r = [zero if x == INF else one / x for x in d]
                S = zero
                for x in r:
                    S = S + x
                dv = [zero if S == 0 else x / S for x in r]
            p = [dv[f] * t[f] for f in range(C)]
            P = zero
            for x in p:
                P = P + x
            best = zero
            for f in range(C):
                v = zero if P == 0 else pr * (p[f] / P)
                vec[i, f] = v
                if v > best:
                    best, lab[i] = v, f + 1
            prob[i] = pr
    return vec, prob, lab


def new_row_anchors(tree, nearest, level, tree_label):
    """the anchors of new rows from the attach scan and the tree read: (tree_label, max(level,
    point_level[nearest])), anchor 0 where nearest is -1"""
    pl = np.asarray(tree.point_level)
    m = len(nearest)
    anchor, lv = np.zeros(m, np.int32), np.array(level, np.float64)
    for i in range(m):
        y = int(nearest[i])
        if y < 0:
            continue
        anchor[i] = int(tree_label[i])
        if pl[y] > lv[i]:
            lv[i] = pl[y]
    return anchor, lv
