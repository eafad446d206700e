"""Shared, seeded inputs of the hierarchy tests on negative, signed-zero, subnormal and infinite
edge weights (test_hierarchy_weights.py on the host, test_gpu_hierarchy_weights.py on the device).
CPU only; nothing here touches the library.

Weight families (FAMILIES): what an MST can hand to the hierarchy since K2g returns exact cosine
and Pearson trees ("a few ulps below zero") and non-finite rows give +inf edges.
Tree shapes: the random recursive tree under a random relabelling of the older tests (n in SIZES),
a caterpillar (several combs more than 200 clusters deep whose heavy paths meet non-negative,
negative, infinite and NaN stabilities in runs shorter than 8 and longer than 64), and wide nodes
(more than 64 valid children under one parent, negative stabilities among them).
A real tree: the cosine and the Pearson Kruskal MST of rays(1500, 5).

Every builder is cached: a tree and its O(levels x n) references are computed once per process
and shared, read-only, by every test that needs them.
"""
import functools

import numpy as np

from cluster_tree_reference import cluster_tree_reference
from constraints_reference import constraints_reference, random_constraints
from glosh_reference import glosh_reference

INF = float("inf")
FO_CHUNK, FO_SHORT, FO_WIDE = 64, 48, 8  # csrc/flat.hip: the FOSC walker's chunk, lane-path and wide-node limits
SIZES = (2, 9, 300, 1500)
MCS = (2, 5)


def _choice(values):
    return lambda rng, m: rng.choice(np.array(values, np.float64), m)


def _signed_zero(first):
    def draw(rng, m):
        w = rng.choice(np.array([-0.0, 0.0, -1e-16, 1e-16, 0.5]), m)
        zero = np.flatnonzero(w == 0.0)
        if zero.shape[0] == 0:
            zero = np.array([int(rng.integers(0, m))])
        w[zero[0]] = first  # the lowest-index zero edge leads its tie group on the host
        return w
    return draw


FAMILIES = {
    "tiny_normal": lambda rng, m: rng.normal(0.0, 1e-15, m),
    "tiny_mixed": _choice([-3e-16, -2e-16, -1e-16, 1e-16, 2e-16, 0.5]),
    "tiny_mixed_zero": _choice([-3e-16, -2e-16, -1e-16, 1e-16, 2e-16, 0.5, 0.0]),
    "inf_tenth": lambda rng, m: np.where(rng.random(m) < 0.1, INF, rng.integers(0, 4, m).astype(np.float64)),
    "all_inf": lambda rng, m: np.full(m, INF),
    "extremes": _choice([1.7e308, 5e-324, 1e-310, 1.0, INF, -5e-324]),
    "all_negative": lambda rng, m: -rng.integers(1, 5, m).astype(np.float64),
    "signed_zero_first": _signed_zero(-0.0),
    "signed_zero_last": _signed_zero(0.0),
}
SIGNED_ZERO = ("signed_zero_first", "signed_zero_last")
SHAPES = ("caterpillar", "wide")
MSTS = ("cosine", "pearson")
# (name, n or None): every family x size, then the shapes and the real trees, which bring their own weights
CASES = [(f, n) for f in FAMILIES for n in SIZES] + [(s, None) for s in SHAPES + MSTS]


def case_id(case):
    return case[0] if case[1] is None else "%s-%d" % case


def case_mcs(case):
    """the minClSize values a case is run at"""
    return (2, 4) if case[0] == "caterpillar" else (2,) if case[0] == "wide" else MCS


def _freeze(*arrays):
    for a in arrays:
        a.setflags(write=False)
    return arrays


def recursive_tree(rng, n):
    """random recursive tree under a random relabelling (test_outlier_scores.random_tree's shape)"""
    va = np.array([int(rng.integers(0, i)) for i in range(1, n)], np.int64)
    vb = np.arange(1, n, dtype=np.int64)
    perm = rng.permutation(n)
    return perm[va].astype(np.int32), perm[vb].astype(np.int32)


def big_recursive_tree(rng, n):
    """the same shape, vectorised, for the 20,000-point trees"""
    va = (rng.random(n - 1) * np.arange(1, n)).astype(np.int64)
    vb = np.arange(1, n, dtype=np.int64)
    perm = rng.permutation(n)
    return perm[va].astype(np.int32), perm[vb].astype(np.int32)


# ------------------------------------------------------------------------------ the caterpillar
# one (kind, teeth) run list per arm, bottom of the comb first.  A run is shorter than 8 or longer
# than 64 teeth.  "zero" (a +inf stability) and "nan" stick to everything above them on a heavy
# path (inf + x = inf, NaN + x = NaN), so arm 0 has neither, arm 1 no "nan", and the arms that have
# them keep them high; the last two arms are there for their "tie3" alone.  A "tie3" entry makes three spine edges equal: one four-way node on the
# path, whose middle tooth is of the named kind and enters through the multi-way sums alone.
ARMS = [
    [("pos", 100), ("neg", 3), ("pos", 70), ("neg", 66), ("pos", 5), ("neg", 7), ("pos", 80)],
    [("neg", 70), ("pos", 2), ("neg", 1), ("pos", 130), ("zero", 3), ("pos", 66), ("neg", 5)],
    [("pos", 170), ("tie3", "nan"), ("pos", 70), ("neg", 4), ("zero", 2), ("nan", 1), ("pos", 6)],
    [("pos", 90), ("tie3", "neg"), ("pos", 75), ("nan", 2), ("pos", 3), ("neg", 68), ("nan", 70)],
    [("pos", 140), ("tie3", "nan"), ("pos", 90)],
    [("neg", 3), ("pos", 117), ("tie3", "nan"), ("pos", 66), ("zero", 1)],
]
BELOW_ZERO = 30  # spine edges of every arm at or below level zero
STEP = 1.0 / 64.0


def _tooth(rng, kind, birth):
    """three inner weights of a 4-point tooth born at `birth` (a path base - x1 - x2 - x3), by the
    stability they give the tooth at minClSize 2; kinds other than "pos" need a positive birth"""
    if kind != "pos" and not birth > 1e-300:
        kind = "pos"
    if kind == "pos":  # below the birth, same sign: 1/eps - 1/birth > 0 (a zero birth: -inf)
        if birth > 0:
            return birth * rng.uniform(0.1, 0.9, 3)
        return birth * rng.uniform(1.5, 3.0, 3) if birth < 0 else -rng.uniform(0.1, 1.0, 3)
    if kind == "neg":  # eps < 0 < birth
        return -rng.uniform(1e-3, 1.0, 3)
    if kind == "zero":  # 1/0 = +inf
        return np.zeros(3)
    # "nan": {base, x1} and {x2, x3} are born at 1e-310 and end at 5e-324: inf - inf
    return np.array([5e-324, 1e-310, 5e-324])


@functools.lru_cache(maxsize=None)
def caterpillar():
    """(va, vb, w, n): the arms' tops chained by edges of weight 100 (the root splits once, into the arms);
    tooth i of an arm hangs on spine vertex i, spine edge i joins vertices i - 1 and i and its
    weight (i - BELOW_ZERO) * STEP rises with i -- top down, a spine edge splits one tooth off the
    chain below it, the chain is the heavy child, and the levels descend through zero (arm 0 and
    arm 2 hold a spine weight of exactly 0.0)"""
    rng = np.random.default_rng(20260117)
    va, vb, w, tops, n = [], [], [], [], 0
    for a, runs in enumerate(ARMS):
        kinds, ties = [], []
        for kind, count in runs:
            if kind == "tie3":
                ties.append(len(kinds))
                kinds += ["pos", count, "pos"]
            else:
                kinds += [kind] * count
        T = len(kinds)
        level = (np.arange(T) - BELOW_ZERO + (a % 2) * 0.5) * STEP  # odd arms step over zero
        for i in ties:
            level[i + 1] = level[i + 2] = level[i]
        base = n + 4 * np.arange(T)
        for i in range(T):
            # tooth i is born with its spine edge; tooth 0 at the lowest edge, with tooth 1
            inner = _tooth(rng, kinds[i], float(level[max(i, 1)]))
            b = int(base[i])
            va += [b, b + 1, b + 2]
            vb += [b + 1, b + 2, b + 3]
            w += inner.tolist()
            if i:
                va.append(int(base[i - 1]))
                vb.append(b)
                w.append(float(level[i]))
        tops.append(int(base[-1]))
        n += 4 * T
    for a in range(1, len(tops)):
        va.append(tops[a - 1])
        vb.append(tops[a])
        w.append(100.0)
    perm = rng.permutation(n)
    return _freeze(perm[np.array(va)].astype(np.int32), perm[np.array(vb)].astype(np.int32),
                   np.array(w, np.float64)) + (n,)


# -------------------------------------------------------------------------------- the wide nodes
WIDE_BLOCKS = (100, 70, 129, 65, 200)  # children of one parent: more than FO_CHUNK each


@functools.lru_cache(maxsize=None)
def wide():
    """(va, vb, w, n): two-point groups (test_gpu_cluster_tree.pair_groups), chained by weight-1.0
    edges inside a block and by 2.0 between blocks: every block is a parent born at 2.0 whose
    groups are all born at 1.0.  Inner weights: positive, negative (a negative stability: eps < 0
    < birth), now and then zero (+inf); one group per block has three points (the heavy
    child, wherever its smallest member puts it among its siblings)"""
    rng = np.random.default_rng(20260118)
    va, vb, w, n, ends = [], [], [], 0, []
    for size in WIDE_BLOCKS:
        heavy = int(rng.integers(0, size))
        prev = None
        for g in range(size):
            kind = rng.random()
            inner = rng.uniform(0.1, 0.9) if kind < 0.5 else -rng.uniform(0.1, 2.0) if kind < 0.97 else 0.0
            pts = 3 if g == heavy else 2
            for k in range(1, pts):
                va.append(n + k - 1), vb.append(n + k), w.append(inner * (1.0 if k == 1 else 0.5))
            if prev is not None:
                va.append(prev), vb.append(n), w.append(1.0)
            prev = n + pts - 1
            n += pts
        ends.append(prev)
    for a, b in zip(ends, ends[1:]):
        va.append(a), vb.append(b - 1), w.append(2.0)
    perm = rng.permutation(n)
    return _freeze(perm[np.array(va)].astype(np.int32), perm[np.array(vb)].astype(np.int32),
                   np.array(w, np.float64)) + (n,)


# ----------------------------------------------------------------------------------- real trees
@functools.lru_cache(maxsize=None)
def real_mst(metric):
    """(X, core, va, vb, w, n): kruskal_mst_metric of rays(1500, 5) with the oracle's cores"""
    from metric_kruskal import metric_case
    X, core, (lo, hi, w) = metric_case(metric, "rays", 5, 1500)
    return X, core, lo, hi, w, X.shape[0]


@functools.lru_cache(maxsize=None)
def tree_case(case):
    """(va, vb, w, n) of a CASES entry, read-only"""
    name, n = case
    if name == "caterpillar":
        return caterpillar()
    if name == "wide":
        return wide()
    if name in MSTS:
        return real_mst(name)[2:]
    rng = np.random.default_rng(1000 * sorted(FAMILIES).index(name) + n)
    va, vb = recursive_tree(rng, n)
    w = np.ascontiguousarray(FAMILIES[name](rng, n - 1), np.float64)
    return _freeze(va, vb, w) + (n,)


@functools.lru_cache(maxsize=None)
def big_case(family, n=20000):
    rng = np.random.default_rng(77 + sorted(FAMILIES).index(family))
    va, vb = big_recursive_tree(rng, n)
    w = np.ascontiguousarray(FAMILIES[family](rng, n - 1), np.float64)
    return _freeze(va, vb, w) + (n,)


# ----------------------------------------------------------------------------------- references
@functools.lru_cache(maxsize=None)
def ref_tree(case, mcs):
    va, vb, w, n = tree_case(case)
    return cluster_tree_reference(va, vb, w, n, mcs)


@functools.lru_cache(maxsize=None)
def ref_glosh(case, mcs):
    va, vb, w, n = tree_case(case)
    return _freeze(*glosh_reference(va, vb, w, n, mcs))


def constraints_of(case, mcs):
    n = tree_case(case)[3]
    return random_constraints(n, min(4 * n, 700), 13 * n + mcs)


@functools.lru_cache(maxsize=None)
def ref_constrained(case, mcs):
    return constraints_reference(ref_tree(case, mcs), *constraints_of(case, mcs))


def cut_levels(w):
    """every distinct weight, +-inf, +-0.0, +-1e-17 and the midpoints between neighbouring levels"""
    lv = np.unique(np.asarray(w, np.float64) + 0.0)
    with np.errstate(over="ignore", invalid="ignore"):
        mids = lv[:-1] / 2 + lv[1:] / 2
    out = np.r_[lv, mids[~np.isnan(mids)], INF, -INF, 0.0, -0.0, 1e-17, -1e-17]
    return out


def case_levels(case):
    """the cut and attach levels of a case: every one up to 1,500 points, beyond that (the caterpillar)
    every seventh and the special values"""
    va, vb, w, n = tree_case(case)
    lv = cut_levels(w)
    return lv if n <= 1500 else np.r_[lv[:-6:7], lv[-6:]]


def ref_cuts(ref, levels):
    """the reference's rows at `levels`: the snapshot of the highest processed level <= eps (brute
    force, no walk rule), all noise below the lowest -- RefTree.cut, with a bisection"""
    n = ref.point_level.shape[0]
    desc = np.array([lv for lv, _ in ref.snapshots], np.float64)  # descending
    rows = np.zeros((len(levels), n), np.int32)
    asc = desc[::-1]
    for i, e in enumerate(np.asarray(levels, np.float64).tolist()):
        k = int(np.searchsorted(asc, e, side="right"))  # levels <= e
        if k > 0:
            rows[i] = ref.snapshots[len(desc) - k][1]
    return rows


def queries_of(case, mcs, m=1500):
    """(nearest, level): training rows (and -1) attached at the cut levels"""
    va, vb, w, n = tree_case(case)
    rng = np.random.default_rng(31 * n + mcs)
    lv = case_levels(case)
    return rng.integers(-1, n, m).astype(np.int32), np.ascontiguousarray(lv[rng.integers(0, lv.shape[0], m)])


# ------------------------------------------------------------------- what a tree holds (host)
def _odd(x):
    """negative, -0.0 or NaN: what the FOSC walker's add-and-max fast path must not meet"""
    x = np.asarray(x, np.float64)
    return np.isnan(x) | np.signbit(x)


def tree_stats(t):
    """counts over a host cluster tree (a ClusterTree or a RefTree): negative and NaN stabilities,
    +inf births, the depth, the largest child count, and what the device's FOSC walk (fo_walk) meets
    on the paths a wave walks (longer than FO_SHORT records, or through a node with more than FO_WIDE
    children).  general: a negative, -0.0 or NaN stability or child contribution on such a path --
    the walker leaves its add-and-max fast path.  A model of its 64-record chunks (from the path's
    bottom; a multi-way node ends a segment) counts the segments of 8 or more records in chunks whose
    staged values are all >= +0: fast where the running value entering the segment is >= +0 too,
    guarded where it is not (the general path inside a clean chunk), both: the chunks that hold a
    fast and a guarded segment (the switch in the middle of a chunk).  Heavy child: the most points, as on the device (ties
    there go by an internal id; here by label)"""
    parent, stab, size = np.asarray(t.parent), np.asarray(t.stability, np.float64), np.asarray(t.size)
    K = parent.shape[0]
    kids = [[] for _ in range(K + 1)]
    for c in range(2, K + 1):
        kids[parent[c - 1]].append(c)
    depth = np.zeros(K + 1, np.int64)
    for c in range(2, K + 1):
        depth[c] = depth[parent[c - 1]] + 1
    contrib = np.zeros(K + 1)
    with np.errstate(all="ignore"):
        for c in range(K, 1, -1):
            prop = np.float64(0.0)
            for k in sorted(kids[c], key=lambda k: t.min_id[k - 1]):
                prop = prop + contrib[k]
            contrib[c] = stab[c - 1] if not kids[c] or stab[c - 1] >= prop else prop
    general, fast, guarded, both = False, 0, 0, 0
    tops = [1] if K else []
    while tops:
        c = tops.pop()
        root_path = c == 1  # the root's own record is never evaluated
        wide_node, odd, recs = False, False, []  # recs: (stability, staged light value, multi-way, contribution)
        while True:
            odd |= c != 1 and bool(_odd(stab[c - 1]))
            if not kids[c]:
                recs.append((stab[c - 1], 0.0, False, contrib[c]))
                break
            h = max(kids[c], key=lambda k: (size[k - 1], k))
            light = [k for k in kids[c] if k != h]
            tops += light
            wide_node |= len(kids[c]) > FO_WIDE
            odd |= c != 1 and bool(_odd(contrib[light]).any())
            recs.append((stab[c - 1], contrib[light[0]] if len(kids[c]) == 2 else 0.0, len(kids[c]) > 2, contrib[c]))
            c = h
        if not (len(recs) > FO_SHORT or wide_node):
            continue  # a lane's path: fo_node, one rule
        general |= odd
        up = recs[:0:-1] if root_path else recs[::-1]  # bottom first
        for lo in range(0, len(up), FO_CHUNK):  # the walker's chunks, from the path's bottom
            chunk = up[lo:lo + FO_CHUNK]
            clean = not any(bool(_odd(st)) or bool(_odd(lv)) for st, lv, _, _ in chunk)
            i = 1 if lo == 0 else 0
            before = fast, guarded
            while i < len(chunk):
                e = next((q for q in range(i, len(chunk)) if chunk[q][2]), len(chunk))
                acc = chunk[i - 1][3] if i else up[lo - 1][3]  # the running value where the segment starts
                if clean and e - i >= 8:
                    fast += not bool(_odd(acc))
                    guarded += bool(_odd(acc))
                i = e + 1
            both += fast > before[0] and guarded > before[1]
    s = stab[1:]
    return dict(negative=int((s < 0).sum()), nan=int(np.isnan(s).sum()), inf_birth=int(np.isinf(t.birth[1:]).sum()),
                depth=int(depth.max()) if K else 0, widest=max((len(k) for k in kids), default=0), general=general,
                fast=fast, guarded=guarded, both=both)
