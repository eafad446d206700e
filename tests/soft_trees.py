"""Hand-built cluster trees, selections and queries for the membership half of soft clustering
(test_soft_trees.py on the host, test_gpu_soft_trees.py on the device).  No fit: the arrays of a
ClusterTree are written down directly, in the shapes a fitted blob tree never has.  CPU only;
nothing here touches the library but the ClusterTree record itself.

Shapes (SHAPES; tree labels, parent[i] in 0..i):
  chain-K    parent[i] = i: depth K.  K at the sizing boundaries of the device's ancestor tables
             (J rows, 2^J >= K): a chain of exactly 2^J clusters sets every bit of a lift
  comb-S     a spine of S clusters with two children each, a leaf and the next spine cluster (the
             condensed shape of the caterpillar): K = 2 S + 1, depth S + 1
  binary-h   complete, h levels: K = 2^h - 1
  star-N     a root with N children
  forest     chain 9, binary 15, two single-cluster roots, chain 17, comb 21 side by side: every
             further root has parent 0 at a label above 1
  random-K-s parent uniform below the label (a random recursive tree), seed s

Births and deaths (levels): a root's birth is NaN, the extra roots of the forest included; the
children of one parent are born at one level, as in a real tree, and that level falls strictly with
the depth; a cluster with children dies where they are born, a leaf at 1/4 .. 4/4 of its birth.
Everything is finite and positive, so with the levels and distances below the restatement has no
NaN (asserted by the tests, never skipped over).

Selections (selection()): "all" (flat_label[i] = i + 1, C = K: nested on purpose, every (anchor,
cluster) pair of the tree), "sampled" (C = 48: the root, label 2, label K and a deepest cluster
among them, flat labels in random order), "multi" (labels carried by two and by three clusters,
ancestor / descendant and unrelated, one label carried by none), "two" (C = 2, for the run of
more queries than one launch has threads).

Queries (queries()): every anchor 0..K at four levels -- its own birth (the birth of its
siblings: M == B ties), 0.0, +inf, and a value strictly between its birth and its parent's -- with
rows of distances from {0.5, 1, 2, 7.25, +inf}, every third row with one to three zeros (+0.0 and
-0.0); then three fixed rows: all +inf, zeros at both ends (the first -0.0), one finite entry.
"""
import functools

import numpy as np

NAN, INF = float("nan"), float("inf")
PALETTE = (0.0, 0.5, 1.0, 2.0, 7.25, INF)
SAMPLED_C = 48


def _freeze(*arrays):
    for a in arrays:
        a.setflags(write=False)
    return arrays


# ---------------------------------------------------------------------------------------- shapes
def chain(K):
    return list(range(K))


def comb(S):
    parent, spine = [0], 1
    for k in range(S):
        first = len(parent) + 1
        parent += [spine, spine]
        spine = first + (k % 2)  # the spine continues through the lower and the higher child in turn
    return parent


def binary(h):
    return [c // 2 for c in range(1, 2 ** h)]


def star(N):
    return [0] + [1] * N


def forest(*trees):
    parent = []
    for t in trees:
        off = len(parent)
        parent += [p + off if p else 0 for p in t]
    return parent


def random_recursive(K, seed):
    rng = np.random.default_rng(seed)
    return [0] + [int(rng.integers(1, c)) for c in range(2, K + 1)]


CHAINS = (1, 2, 3, 4, 5, 8, 9, 16, 17, 64, 65, 1024, 1025)
SHAPES = {"chain-%d" % K: functools.partial(chain, K) for K in CHAINS}
SHAPES.update({"comb-%d" % S: functools.partial(comb, S) for S in (40, 600)})
SHAPES.update({"binary-%d" % h: functools.partial(binary, h) for h in (1, 2, 3, 4, 5, 6, 11)})
SHAPES["star-299"] = functools.partial(star, 299)
SHAPES["forest"] = functools.partial(forest, chain(9), binary(4), chain(1), chain(1), chain(17), comb(10))
SHAPES.update({"random-500-%d" % s: functools.partial(random_recursive, 500, s) for s in (1, 2)})


def table_rows(K):
    """J of csrc/soft.hip: the rows of the ancestor tables"""
    J = 1
    while (1 << J) < K:
        J += 1
    return J


@functools.lru_cache(maxsize=None)
def shape(name):
    """(parent int32, birth, death, depth int64 by tree label with depth[0] = 0), read-only"""
    parent = np.asarray(SHAPES[name](), np.int32)
    K = parent.shape[0]
    depth = np.zeros(K + 1, np.int64)
    has_child = np.zeros(K + 1, bool)
    for c in range(1, K + 1):
        depth[c] = depth[parent[c - 1]] + 1
        has_child[parent[c - 1]] = True
    D = int(depth.max()) if K else 0
    born = lambda p: (D + 1 - depth[p]) * 0.25 + (p % 4) / 32.0  # the level at which p's children are born
    birth, death = np.empty(K), np.empty(K)
    for c in range(1, K + 1):
        p = int(parent[c - 1])
        birth[c - 1] = born(p) if p else NAN
        if has_child[c]:
            death[c - 1] = born(c)
        else:
            death[c - 1] = birth[c - 1] * (1 + c % 4) / 4.0 if p else 0.5 * (1 + c % 4)
    return _freeze(parent, birth, death, depth)


def make_tree(pkg, name, flat, C):
    """a host ClusterTree over the shape: no points, the given selection"""
    parent, birth, death, _ = shape(name)
    K = parent.shape[0]
    z, zi = np.zeros(K), np.zeros(K, np.int32)
    return pkg.ClusterTree(parent, birth, death, z, zi, zi, np.asarray(flat, np.int32), np.zeros(0, np.int32),
                           np.zeros(0), C)


def ancestors(parent, c):
    """c and its ancestors, c first (a plain walk)"""
    out = []
    while c > 0:
        out.append(c)
        c = int(parent[c - 1])
    return out


def related(parent, a, b):
    return a in ancestors(parent, b) or b in ancestors(parent, a)


# ------------------------------------------------------------------------------------ selections
@functools.lru_cache(maxsize=None)
def selection(name, kind):
    """(flat_label int32[K], C, witnesses) -- witnesses: for "multi", the clusters behind each claim"""
    parent, _, _, depth = shape(name)
    K = parent.shape[0]
    deepest = int(np.argmax(depth))
    flat, wit = np.zeros(K, np.int32), {}
    if kind == "all":
        flat[:] = np.arange(1, K + 1)
        C = K
    elif kind == "sampled":
        rng = np.random.default_rng(K + len(name))
        picks = list(dict.fromkeys([1, 2, K, deepest]))
        picks += [int(c) for c in rng.permutation(np.arange(1, K + 1)) if c not in picks][:SAMPLED_C - len(picks)]
        assert len(set(picks)) == SAMPLED_C
        flat[np.array(picks) - 1] = rng.permutation(np.arange(1, SAMPLED_C + 1))
        C = SAMPLED_C
    elif kind == "multi":
        rng = np.random.default_rng(7 * K + len(name))
        path = ancestors(parent, deepest)
        assert len(path) >= 4
        used, kept = set(), {path[-1], deepest, path[-2], path[1]}  # kept: placed by hand below

        def unrelated_to(cs):
            for c in rng.permutation(np.arange(1, K + 1)).tolist():
                if c not in used | kept and not any(related(parent, c, x) for x in cs):
                    return c
            return next(c for c in range(K, 0, -1) if c not in used | kept)  # a chain has no unrelated pair

        def carry(label, cs):
            for c in cs:
                assert c not in used
                used.add(c)
                flat[c - 1] = label
        carry(1, [path[-1], deepest])  # a root and the deepest cluster under it
        wit["nested"] = (1, path[-1], deepest)
        u = unrelated_to([])
        used.add(u)
        v = unrelated_to([u])
        used.discard(u)
        carry(2, [u, v])
        wit["pair"] = (2, u, v)
        # label 3: no cluster
        carry(4, [path[-2], path[1], unrelated_to([path[-2]])])
        wit["three"] = (4,) + tuple(c for c in range(1, K + 1) if flat[c - 1] == 4)
        carry(5, [unrelated_to([])])
        C = 5
    elif kind == "two":  # label 1 on the deepest cluster and on its root's child, label 2 on cluster 12
        path = ancestors(parent, deepest)
        flat[[path[-2] - 1, deepest - 1]] = 1
        flat[11] = 2
        C = 2
    else:
        raise KeyError(kind)
    flat.setflags(write=False)
    return flat, C, wit


# --------------------------------------------------------------------------------------- queries
@functools.lru_cache(maxsize=None)
def anchors_and_levels(name):
    """(anchor int32, level): every anchor 0..K at four levels, then the deepest cluster three times"""
    parent, birth, death, depth = shape(name)
    K = parent.shape[0]
    # a root without children keeps eps_max = Double.MAX_VALUE: only label 1 can be one, and any
    # finite positive level under it overflows (inf / inf further on), so it is asked at 0 and +inf
    bare_root = K >= 1 and not np.any(parent == 1)
    anchor, level = [], []
    between = np.zeros(K + 1)
    for a in range(K + 1):
        if a == 0:
            four = [1.0, 0.0, INF, 0.5]
        elif a == 1 and bare_root:
            four = [0.0, 0.0, INF, INF]
        else:
            p, b = int(parent[a - 1]), float(birth[a - 1])
            if p == 0:  # a root: where its children are born, and half of that
                four = [float(death[a - 1]), 0.0, INF, float(death[a - 1]) * 0.5]
            elif parent[p - 1] == 0:  # a root's child: its own birth is the only one on the path
                four = [b, 0.0, INF, b * 1.5]
            else:
                four = [b, 0.0, INF, (b + float(birth[p - 1])) / 2]
                assert b < four[3] < birth[p - 1]
        between[a] = four[3]
        anchor += [a] * 4
        level += four
    if K:
        z = int(np.argmax(depth))
        anchor += [z] * 3
        level += [float(between[z])] * 3
    return _freeze(np.asarray(anchor, np.int32), np.asarray(level, np.float64))


@functools.lru_cache(maxsize=None)
def queries(name, C, seed=0):
    """(anchor, level, dmin m x C), read-only"""
    anchor, level = anchors_and_levels(name)
    m = anchor.shape[0]
    K = shape(name)[0].shape[0]
    rng = np.random.default_rng(1000 * seed + 31 * m + C)
    dmin = rng.choice(np.array(PALETTE[1:]), (m, C))
    if C:
        for i in range(0, m, 3):
            pos = rng.integers(0, C, 1 + (i // 3) % 3)
            dmin[i, pos] = 0.0
            if i % 2:
                dmin[i, pos[0]] = -0.0
        if K:  # the three fixed rows
            dmin[m - 3] = INF
            dmin[m - 2, 0], dmin[m - 2, C - 1] = -0.0, 0.0  # C == 1: one +0.0
            if C > 2:
                dmin[m - 2, C // 2] = 0.0
            dmin[m - 1] = INF
            dmin[m - 1, C // 2] = 2.0
    return anchor, level, _freeze(dmin)[0]


GRID_CAP = 16384 * 256  # csrc/common.hpp grid_for: at most 16,384 workgroups of 256 threads per launch


def tiled_queries(name, C, m):
    """m queries: the anchors and levels of the shape over and over (their count, odd, divides
    neither the workgroup nor the grid), fresh distances for every row"""
    anchor, level = anchors_and_levels(name)
    idx = np.arange(m) % anchor.shape[0]
    rng = np.random.default_rng(m + C)
    pal = np.array(PALETTE + (-0.0,))
    dmin = pal[rng.integers(1, 6, (m, C))]
    zero = np.flatnonzero(rng.integers(0, 4, m) == 0)
    dmin[zero, rng.integers(0, C, zero.shape[0])] = pal[rng.choice([0, 6], zero.shape[0])]
    return anchor[idx], level[idx], dmin


# ----------------------------------------------------------------------------------------- cases
# (shape, selection, reference): "restatement" = tests/soft_reference.py on every row; "host" = the
# host path of csrc/soft.cpp on every row, which test_soft_trees.py pins to the restatement on these
# very inputs (a sample of the rows where the Python walk over every row takes minutes)
CASES = [("chain-%d" % K, "all", "restatement") for K in CHAINS if K <= 65]
CASES += [("chain-1024", "sampled", "host"), ("chain-1025", "sampled", "host")]
CASES += [("comb-40", "sampled", "restatement"), ("comb-600", "sampled", "host")]
CASES += [("binary-%d" % h, "all", "restatement") for h in (1, 2, 3, 4, 5, 6)]
CASES += [("binary-6", "sampled", "restatement"), ("binary-11", "sampled", "host")]
CASES += [("star-299", "sampled", "restatement")]
CASES += [("forest", "all", "restatement"), ("forest", "sampled", "restatement")]
CASES += [("random-500-1", "sampled", "restatement"), ("random-500-2", "sampled", "restatement")]
CASES += [(s, "multi", "restatement") for s in ("chain-9", "chain-17", "binary-4", "binary-6", "comb-40", "forest",
                                                "random-500-1")]
CASE_IDS = ["%s-%s" % c[:2] for c in CASES]
HOST_SAMPLE = 96  # rows of a "host" case that the CPU test walks in Python


def case_inputs(pkg, case):
    """(host tree, flat, C, anchor, level, dmin) of a CASES entry"""
    name, kind, _ = case
    flat, C, _ = selection(name, kind)
    anchor, level, dmin = queries(name, C)
    return make_tree(pkg, name, flat, C), flat, C, anchor, level, dmin


def sample_rows(m, count=HOST_SAMPLE):
    """a fixed sample of row indices: the first rows, the last ones (the deepest anchors and the
    fixed rows) and a spread in between"""
    if m <= count:
        return np.arange(m)
    rng = np.random.default_rng(m)
    return np.unique(np.r_[np.arange(8), np.arange(m - 24, m), rng.integers(0, m, count - 32)])
