"""Test-side reference for the cluster tree and the level cuts: a plain top-down restatement,
independent of the library's bottom-up algorithms (in the style of glosh_reference.py).

* The spanning tree's edges are removed in descending weight, a tie group (one level; -0.0 and
  0.0 are one level) at once.  When a cluster's component falls apart, a part with >= minClSize
  points is valid: with two or more valid parts the cluster ends and each valid part is born as
  a child at that level; with exactly one the cluster lives on in it; the points of every
  other part become noise: eps(x) = the level, last(x) = the cluster they leave.
* Per cluster: birth (NaN for the root), death (the last level at which points leave it), size
  and smallest member at birth, stability = one term ``count * (1/level - 1/birth)`` per level
  at which points leave, added in descending level (count: every point when the cluster ends,
  else the points of the invalid parts).
* FOSC: children in ascending smallest member; a cluster keeps itself when its stability is >=
  the sum of its children's contributions; the root is never selected; flat labels 1.. by
  ascending smallest member.
* Tree labels: 1 = the root, 2.. by (birth descending, smallest member ascending).
* ``snapshots``: the tree-label array as it stands before each level is processed -- the
  hierarchy row of that level, by brute force; ``cut(eps)`` picks the row that holds while
  every edge of weight <= eps is still present, with no use of the walk rule.

O(levels x n): for n of about 2,000 or less.
"""
import numpy as np


class RefTree:
    pass


def cluster_tree_reference(va, vb, w, n, min_cl_size):
    va, vb = np.asarray(va, np.int64), np.asarray(vb, np.int64)
    w = np.asarray(w, np.float64)
    adj = [set() for _ in range(n)]
    by_level = {}
    for a, b, x in zip(va.tolist(), vb.tolist(), w.tolist()):
        if a == b:
            continue
        adj[a].add(b)
        adj[b].add(a)
        by_level.setdefault(x + 0.0, []).append((a, b))
    eps = np.zeros(n, np.float64)
    last = np.zeros(n, np.int64)
    cluster_of = [0] * n
    parent, birth, death, size, minid = [-1], [np.float64("nan")], [np.float64(0.0)], [n], [0]
    stab = [np.float64(0.0)]
    kids = [[]]
    members = [list(range(n))]
    raw_snaps = []
    one = np.float64(1.0)
    with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
        for level in sorted(by_level, reverse=True):
            raw_snaps.append((level, list(cluster_of)))
            touched = {}
            for a, b in by_level[level]:
                adj[a].discard(b)
                adj[b].discard(a)
                c = cluster_of[a]
                if c >= 0:
                    touched.setdefault(c, []).extend((a, b))
            for c, ends in touched.items():
                seen, parts = set(), []
                for s in ends:
                    if s in seen:
                        continue
                    seen.add(s)
                    part, i = [s], 0
                    while i < len(part):
                        for y in adj[part[i]]:
                            if y not in seen:
                                seen.add(y)
                                part.append(y)
                        i += 1
                    parts.append(part)
                valid = sorted((p for p in parts if len(p) >= min_cl_size), key=min)
                gone = 0
                for p in parts:
                    if len(p) < min_cl_size:
                        gone += len(p)
                        for x in p:
                            eps[x] = level
                            last[x] = c
                            cluster_of[x] = -1
                count = gone if len(valid) == 1 else sum(len(p) for p in parts)
                if count > 0:
                    stab[c] = stab[c] + np.float64(count) * (one / np.float64(level) - one / birth[c])
                    death[c] = np.float64(level)
                if len(valid) >= 2:
                    for p in valid:
                        k = len(parent)
                        parent.append(c)
                        birth.append(np.float64(level))
                        death.append(np.float64(0.0))
                        size.append(len(p))
                        minid.append(min(p))
                        stab.append(np.float64(0.0))
                        kids.append([])
                        members.append(p)
                        kids[c].append(k)
                        for x in p:
                            cluster_of[x] = k
    K = len(parent)
    # FOSC, children before parents (children are numbered after their parents)
    contrib = [np.float64(0.0)] * K
    keep = [False] * K
    for c in range(K - 1, 0, -1):
        prop = np.float64(0.0)
        for k in kids[c]:  # ascending smallest member
            prop = prop + contrib[k]
        if not kids[c] or stab[c] >= prop:
            contrib[c], keep[c] = stab[c], True
        else:
            contrib[c] = prop
    sel, todo = [], list(kids[0])
    while todo:
        c = todo.pop()
        if keep[c]:
            sel.append(c)
        else:
            todo.extend(kids[c])
    sel.sort(key=lambda c: minid[c])
    flat_of = [0] * K
    for i, c in enumerate(sel):
        flat_of[c] = i + 1
    order = [0] + sorted(range(1, K), key=lambda c: (-birth[c], minid[c]))
    lab = [0] * K
    for i, c in enumerate(order):
        lab[c] = i + 1
    t = RefTree()
    t.K = K
    t.parent = np.array([lab[parent[c]] if c else 0 for c in order], np.int32)
    t.birth = np.array([birth[c] for c in order], np.float64)
    t.death = np.array([death[c] for c in order], np.float64)
    t.stability = np.array([stab[c] for c in order], np.float64)
    t.size = np.array([size[c] for c in order], np.int32)
    t.min_id = np.array([minid[c] for c in order], np.int32)
    t.flat_label = np.array([flat_of[c] for c in order], np.int32)
    t.point_cluster = np.array([lab[c] for c in last.tolist()], np.int32)
    t.point_level = eps
    t.n_clusters = len(sel)
    tolab = np.array(lab + [0], np.int32)  # index -1 (noise) -> 0
    t.snapshots = [(lv, tolab[np.asarray(s, np.int64)]) for lv, s in raw_snaps]
    # flat labels: a point belongs to the selected cluster that held it at birth
    flat = np.zeros(n, np.int32)
    for c in sel:
        flat[members[c]] = flat_of[c]
    t.flat = flat

    def cut(e, t=t, n=n):
        for lv, row in t.snapshots:  # descending: the first level <= e is the highest such
            if lv <= e:
                return row
        return np.zeros(n, np.int32)

    t.cut = cut
    return t
