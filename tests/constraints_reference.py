"""Test-side reference for the constraint-aware flat extraction: a top-down restatement of
HDBSCANStar.calculateNumConstraintsSatisfied over label snapshots, independent of the library's
LCA closed form and of ``point_cluster`` (the labels come from the rows too).

* The label rows come from cluster_tree_reference's ``snapshots`` (brute force).  The first call
  is for the root with every label 1.  Then, at every level at which clusters are born, the rule
  is applied to the row that holds AFTER that level (the next snapshot; all noise after the last):
  - a must-link pair whose two labels are equal adds 2 to that cluster when it is new;
  - a cannot-link pair whose labels differ, or whose first label is noise, adds 1 to each
    endpoint's cluster when it is new and not noise; an endpoint that is noise adds 1 to the
    virtual child of the first of the new clusters' parents whose virtual child holds it.  A
    parent's virtual child is every point that left it as noise: the points whose row entry is 0
    now and whose last non-zero label in the rows so far is that parent.
* Propagation and selection as the contract states them: children before parents and in ascending
  tree label, ``prop_sat = virt + sum chosen_sat``, ``prop_stability = 0.0 + ...`` one addition
  per child, a non-root cluster chosen as itself when it is a leaf, or satisfies more, or as many
  with ``stability >= prop_stability``; the topmost self-chosen clusters are selected, numbered
  by ascending (smallest member, tree label).

O(birth levels x (n + m)), vectorised per level: for n of about 2,000 or less.
"""
import numpy as np

from cluster_tree_reference import cluster_tree_reference

MUST_LINK, CANNOT_LINK = 0, 1


def big_tree(n, values, seed):
    """random recursive tree; weights continuous (values None) or from `values` distinct values
    (the generator of the GPU tests, without their torch import)"""
    rng = np.random.default_rng(seed)
    va = (rng.random(n - 1) * np.arange(1, n)).astype(np.int64)
    vb = np.arange(1, n, dtype=np.int64)
    w = rng.random(n - 1) if values is None else rng.integers(0, values, n - 1) / 8.0
    perm = rng.permutation(n)
    return perm[va].astype(np.int32), perm[vb].astype(np.int32), w


def random_constraints(n, m, seed):
    """m pairs of mixed types; a few with a == b"""
    rng = np.random.default_rng(seed)
    ca, cb = rng.integers(0, n, m).astype(np.int32), rng.integers(0, n, m).astype(np.int32)
    same = rng.random(m) < 0.02
    cb[same] = ca[same]
    return ca, cb, (rng.random(m) < 0.5).astype(np.int32)


class RefConstrained:
    pass


def constraints_reference(ref, ca, cb, ctype):
    """ref: the RefTree of cluster_tree_reference (its tree labels are the library's)"""
    ca, cb, ctype = np.asarray(ca, np.int64), np.asarray(cb, np.int64), np.asarray(ctype, np.int64)
    K, n, m = ref.K, ref.point_level.shape[0], ca.shape[0]
    num = np.zeros(K + 1, np.int64)
    virt = np.zeros(K + 1, np.int64)
    ml, cl = ctype == MUST_LINK, ctype == CANNOT_LINK
    assert np.all(ml | cl)
    parent = np.r_[0, ref.parent].astype(np.int64)  # by label
    birth = np.r_[np.nan, ref.birth]

    def apply(row, new, lastlab):
        is_new = np.zeros(K + 1, bool)
        is_new[list(new)] = True
        la, lb = row[ca], row[cb]
        hit = ml & (la == lb) & is_new[la]
        np.add.at(num, la[hit], 2)
        live = cl & ((la != lb) | (la == 0))
        for lab, pts in ((la, ca), (lb, cb)):
            np.add.at(num, lab[live & (lab != 0) & is_new[lab]], 1)
            # the virtual child: the endpoint is noise now, and the cluster it left is splitting here
            parents = np.zeros(K + 1, bool)
            parents[[parent[c] for c in new if parent[c]]] = True
            gone = live & (lab == 0)
            src = lastlab[pts]
            np.add.at(virt, src[gone & parents[src]], 1)

    lastlab = np.zeros(n, np.int64)
    born_row = {}
    rows = [np.asarray(r, np.int64) for _, r in ref.snapshots] + [np.zeros(n, np.int64)]
    levels = [lv for lv, _ in ref.snapshots]
    if K >= 1 and n > 0:
        apply(np.ones(n, np.int64), [1], lastlab)  # the initial call: the root, every label 1
    for i, lv in enumerate(levels):
        nz = rows[i] != 0
        lastlab[nz] = rows[i][nz]
        new = [c for c in range(2, K + 1) if birth[c] == lv]
        if new:
            apply(rows[i + 1], new, lastlab)
            for c in new:
                born_row[c] = i + 1
    # propagation: children before parents (a parent's label is below its children's)
    kids = [[] for _ in range(K + 1)]
    for c in range(2, K + 1):
        kids[parent[c]].append(c)  # ascending label
    stab = np.r_[np.nan, ref.stability]
    psat = np.zeros(K + 1, np.int64)
    pstab = np.zeros(K + 1, np.float64)
    self_ = np.zeros(K + 1, bool)
    chosen = [(0, np.float64(0.0))] * (K + 1)
    for c in range(K, 0, -1):
        ps, pst = (int(virt[c]) if kids[c] else 0), np.float64(0.0)
        for k in kids[c]:
            ps += chosen[k][0]
            pst = pst + chosen[k][1]
        psat[c], pstab[c] = ps, pst
        if c != 1 and (not kids[c] or num[c] > ps or (num[c] == ps and stab[c] >= pst)):
            self_[c] = True
            chosen[c] = (int(num[c]), np.float64(stab[c]))
        else:
            chosen[c] = (ps, pst)
    sel, todo = [], list(kids[1]) if K >= 1 else []
    while todo:
        c = todo.pop()
        if self_[c]:
            sel.append(c)
        else:
            todo.extend(kids[c])
    sel.sort(key=lambda c: (int(ref.min_id[c - 1]), c))
    flat = np.zeros(K + 1, np.int32)
    for i, c in enumerate(sel):
        flat[c] = i + 1
    labels = np.zeros(n, np.int32)
    for c in sel:  # a point belongs to the selected cluster that held it at birth
        labels[rows[born_row[c]] == c] = flat[c]
    out = RefConstrained()
    out.num_sat, out.prop_sat = num[1:].astype(np.int32), psat[1:].astype(np.int32)
    out.prop_stability, out.flat_label = pstab[1:], flat[1:]
    out.labels = labels
    out.n_clusters = len(sel)
    return out
