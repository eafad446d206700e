"""Inputs and CPU references of the point and bubble kernels under the four non-Euclidean metrics
(tests/test_gpu_metrics.py): the generic k-NN scan with its merge and the cumulative epilogue
(csrc/knn.hip), every Prim kernel (csrc/prim.hip), the batched leaf, and the bubble k-NN, bubble
Prim and local model (csrc/bubbles.hip, csrc/local_model.cpp).  Plain numpy and the CPU oracle, no
device; every reference is computed once per process and handed out read-only.

Families (n rows, d columns):
  rays, rounded_blobs   metric_kruskal's: rows that are positive multiples of one another (cosine and
                        Pearson distances a few ulps either side of 0, negative ones included, and
                        heavy ties); blobs rounded to one decimal
  zero_row7 / _last     rays with row 7 / row n - 1 all zeros: cosine is NaN against it
  const_row7 / _last    rays with that row constant: Pearson is NaN against it (cosine is not).
                        Row n - 1 is Prim's start vertex, so every first-step weight is NaN there
  scaled_up / _down     rounded_blobs times 1e160 / 1e-170: cosine and Pearson overflow in the norm
                        products (1 or NaN) / underflow to 0 / 0; Manhattan and supremum stay finite
  integer_grid          coordinates in {0, 1, 2, 3} with an eighth of the rows repeated: massive
                        exact ties and zero distances under Manhattan and supremum (and all-zero
                        rows, NaN under cosine)
  same, constcol, inf_rows   degenerate_inputs' families through nonleaf_inputs.nl_family (d = 3)

prim_reference(): a plain-Python transcription of HDBSCANStar.constructMST (HDBSCANStar.java:124-205)
over the oracle's pairwise distances, which pins oracle.prim_mst where weights are negative or tie.
oracle/java_transcription.py and tests/path_helpers.py hold no point Prim (the former has the
bubble Prim with its own Euclidean distance only), so this one is new."""
import functools

import numpy as np

from metric_kruskal import METRICS, pair_distances, rays, rounded_blobs, zero_row
from nonleaf_inputs import nl_family, ro

SEMANTICS = (0, 1, 2)  # CORE_INCL_SELF_CUMULATIVE, CORE_INCL_SELF, CORE_EXCL_SELF
DBL_MAX = float(np.finfo(np.float64).max)
ANGULAR = ("cosine", "pearson")


def const_row(n, d, pos):
    """rays with row pos constant: zero variance, so its Pearson distance to every row is NaN"""
    X = rays(n, d)
    X[pos] = 1.25
    return X


def scaled(n, d, factor):
    return rounded_blobs(n, d) * factor


def integer_grid(n, d):
    """coordinates in {0, 1, 2, 3}; rows [n / 2, n / 2 + n / 8) repeat rows [0, n / 8)"""
    X = np.random.default_rng(6000 + 31 * d + n).integers(0, 4, size=(n, d)).astype(np.float64)
    k = n // 8
    X[n // 2:n // 2 + k] = X[:k]
    return X


FAMILIES = {
    "rays": rays, "rounded_blobs": rounded_blobs, "integer_grid": integer_grid,
    "zero_row7": lambda n, d: zero_row(n, d, 7), "zero_row_last": lambda n, d: zero_row(n, d, n - 1),
    "const_row7": lambda n, d: const_row(n, d, 7), "const_row_last": lambda n, d: const_row(n, d, n - 1),
    "scaled_up": lambda n, d: scaled(n, d, 1e160), "scaled_down": lambda n, d: scaled(n, d, 1e-170),
    "same": lambda n, d: nl_family("same", n), "constcol": lambda n, d: nl_family("constcol", n),
    "inf_rows": lambda n, d: nl_family("inf_rows", n),
}
NL_DIM = 3  # the d of the nl_family entries


@functools.lru_cache(maxsize=None)
def points(family, n, d):
    X = np.ascontiguousarray(FAMILIES[family](n, d), np.float64)
    assert X.shape == (n, NL_DIM if family in ("same", "constcol", "inf_rows") else d), (family, X.shape)
    return ro(np.array(X))


def family_of(metric):
    """the family of the Prim cases: negative weights for the angular metrics, ties for the others"""
    return "rays" if metric in ANGULAR else "integer_grid"


# ------------------------------------------------------------------------------ core distances
@functools.lru_cache(maxsize=None)
def core_case(metric, family, n, d, min_pts, sem):
    """(X, oracle.core_distances)"""
    from oracle import oracle as O
    X = points(family, n, d)
    return X, ro(O.core_distances(X, min_pts, metric=metric, semantics=sem))


@functools.lru_cache(maxsize=None)
def knn_case(metric, family, n, d, k, excl):
    """oracle.knn_lists: n x k, ascending, Double.MAX_VALUE padded"""
    from oracle import oracle as O
    return ro(O.knn_lists(points(family, n, d), k + 1, metric=metric, excl_self=bool(excl)))


# (family, n, d, minPts) of the core-distance cases; each runs under the four metrics and the three
# semantics.  n around one 256-query tile and below minPts; 3000 rows: the candidate split is 11,
# so the merge of partial lists runs; one minPts per list bucket (1 | 3 | 7 | 15 | 31 entries)
def _core_cases():
    out = []
    for n in (1, 2, 3, 5, 255, 257, 1025):
        out += [("rays", n, 5, 4), ("integer_grid", n, 5, 4)]
    for d in (5, 24):
        out += [("rays", 3000, d, 4), ("integer_grid", 3000, d, 4)]
    out += [("zero_row7", 3000, 5, 4), ("const_row_last", 3000, 24, 4)]
    out += [("rays", 1025, 5, mp) for mp in (1, 2, 8, 16, 32)]
    out += [(f, 1025, 5, 4) for f in ("zero_row7", "zero_row_last", "const_row7", "const_row_last", "scaled_up",
                                      "scaled_down", "rounded_blobs")]
    out += [(f, 1025, NL_DIM, 4) for f in ("same", "constcol", "inf_rows")]
    return out


CORE_CASES = _core_cases()


# --------------------------------------------------------------------------------------- Prim
def prim_reference(n, pair_d, core, ids, self_edges=True):
    """HDBSCANStar.constructMST (HDBSCANStar.java:124-205) in plain Python floats.  pair_d: the
    distance of every pair i < j in np.triu_indices order.  Select on '<=' (:177), update on '<'
    (:170), the parent of a vertex that was never updated is 0 (a new int[]).  Returns
    (va, vb, w) as lists: n - 1 tree edges, then the n self edges."""
    D = [[0.0] * n for _ in range(n)]
    k = 0
    pd = [float(x) for x in pair_d]
    for a in range(n - 1):
        for b in range(a + 1, n):
            D[a][b] = D[b][a] = pd[k]
            k += 1
    core = [float(c) for c in core]
    ids = [int(i) for i in ids]
    attached = [False] * n
    near = [0] * (n - 1)
    dist = [DBL_MAX] * (n - 1)
    cur = n - 1
    attached[cur] = True
    num = 1
    while num < n:
        best_pt, best_d = -1, DBL_MAX
        row, cc = D[cur], core[cur]
        for nb in range(n):
            if nb == cur or attached[nb]:
                continue
            mrd = row[nb]
            if cc > mrd:
                mrd = cc
            if core[nb] > mrd:
                mrd = core[nb]
            if mrd < dist[nb]:
                dist[nb] = mrd
                near[nb] = ids[cur]
            if dist[nb] <= best_d:
                best_d = dist[nb]
                best_pt = nb
        attached[best_pt] = True
        num += 1
        cur = best_pt
    other = ids[:n - 1]
    if self_edges:
        near, other, dist = near + ids, other + ids, dist + core
    return near, other, dist


def prim_ids(n):
    return ro(np.arange(n, dtype=np.int32) * 3 + 1)


@functools.lru_cache(maxsize=None)
def prim_case(metric, family, n, d, min_pts=4, sem=0):
    """(X, oracle cores, ids = 3 i + 1, oracle.prim_mst with self edges)"""
    from oracle import oracle as O
    X, core = core_case(metric, family, n, d, min_pts, sem)
    ids = prim_ids(n)
    return X, core, ids, ro(*O.prim_mst(X, core, ids, metric=metric, self_edges=True))


def tree_weights(case):
    n = case[0].shape[0]
    return case[3][2][:n - 1]


# the block kernel's four classes (64 x 1, 64 x 4, 256 x 4, 1024 x 4 vertices) and their borders
BLOCK_SHAPES = [(n, 5) for n in (1, 2, 3, 64, 65, 256, 257, 1024, 1025)] + [(4096, 3)]
# prim_coop4_kernel<BS, DM>: (DM, n, d); 1024 < n <= 4096 reaches it only for 8 <= d <= 16
COOP4_SHAPES = [(4, 4500, 3), (8, 1025, 8), (8, 1100, 8), (16, 1100, 16)]
COOP4_METRICS = ("cosine", "pearson", "manhattan")
COOP_ANY_D = (4500, 24)  # d > 16: prim_coop_kernel by default
# every (metric, n, d) whose tree must be mostly negative (test_metric_inputs.py)
NEGATIVE_PRIM_SHAPES = sorted({(n, d) for _, n, d in COOP4_SHAPES} | {COOP_ANY_D})
# core semantics of the Prim cases: the cumulative cores except where a NaN row needs EXCL_SELF
PRIM_SEM = 0
BAD_ROW_SEM = 2
BAD_ROW_SHAPE = (1100, 8)


# ------------------------------------------------------------------------------- batched leaf
LEAF_SIZES = [50, 49, 1, 2, 37, 3, 300, 1100]
LEAF_D = 8
LEAF_METRICS = ("cosine", "manhattan")


@functools.lru_cache(maxsize=None)
def leaf_case(metric, min_pts=4):
    """(X, ids, offsets, [(core, (va, vb, w)) per partition]) of oracle.first_step_leaf"""
    from oracle import oracle as O
    off = np.concatenate([[0], np.cumsum(LEAF_SIZES)]).astype(np.int64)
    n = int(off[-1])
    X = points("rays", n, LEAF_D)
    ids = ro(np.random.default_rng(77).permutation(n).astype(np.int32) * 2 + 5)
    ref = []
    for a, b in zip(off[:-1], off[1:]):
        core, (va, vb, w) = O.first_step_leaf(np.array(X[a:b]), ids[a:b], min_pts, metric)
        ref.append((ro(core), ro(va, vb, w)))
    return X, ids, ro(off), ref


# ------------------------------------------------------------------------------------ bubbles
BUBBLE_FAMILIES = ("rays", "rounded_blobs")
BUBBLE_SHAPES = [(300, 5), (1100, 8)]
BUBBLE_CASES = [(m, f, n, d) for m in METRICS for f in BUBBLE_FAMILIES for n, d in BUBBLE_SHAPES]


def singletons(b):
    """CombineStep's one-member bubbles: (nB, eB, nnB) = (1, 0, 0)"""
    return ro(np.ones(b, np.int32), np.zeros(b), np.zeros(b))


@functools.lru_cache(maxsize=None)
def bubble_core_case(metric, family, n, d, min_pts):
    from oracle import oracle as O
    return ro(O.bubble_core_distances(points(family, n, d), *singletons(n), min_pts, metric))


@functools.lru_cache(maxsize=None)
def bubble_prim_case(metric, family, n, d):
    """oracle.bubble_prim_mst on the oracle's cores at minPts 4, ids 0..n-1, self edges"""
    from oracle import oracle as O
    _, eB, nnB = singletons(n)
    return ro(*O.bubble_prim_mst(points(family, n, d), eB, nnB, bubble_core_case(metric, family, n, d, 4),
                                 metric=metric))


@functools.lru_cache(maxsize=None)
def local_model_case(metric, family, n, d):
    """the oracle's local model at minPts 4, minClSize 4, or the error code it raises"""
    from oracle import oracle as O
    info = np.zeros((n, 3))
    info[:, 2] = 1.0  # (extent, nnDist, n)
    try:
        r = O.local_model(points(family, n, d), info, 4, 4, metric)
    except O.OracleError as e:
        return e.code
    ro(r["labels"], *r["mst"], *r["inter"])
    return r
