"""Mirror of the reference's ``distance`` and ``hdbscanstar`` packages over libhdbmi.

Same class/method names and argument meaning as the Java (源代码/distance/*.java,
源代码/hdbscanstar/HDBSCANStar.java, UndirectedGraph.java); the bodies call the C-ABI.
Arrays may be numpy (host) or torch tensors (host or HIP device); results come back on the
side the input lives on.
"""
from __future__ import annotations

import numpy as np

from . import _capi as A


# --------------------------------------------------------------- distance
class DistanceCalculator:
    """distance/DistanceCalculator.java:9-21."""

    name = ""

    def getName(self) -> str:  # DistanceCalculator.java:20
        return self.name

    def computeDistance(self, attributesOne, attributesTwo) -> float:  # :17
        a = np.asarray(attributesOne, np.float64).reshape(1, -1)
        b = np.asarray(attributesTwo, np.float64).reshape(1, -1)
        return float(distance_rows(a, b, self)[0])

    @property
    def metric(self) -> int:
        return A.METRIC[self.getName()]


class EuclideanDistance(DistanceCalculator):
    name = "euclidean"  # EuclideanDistance.java:28-41


class CosineSimilarity(DistanceCalculator):
    name = "cosine"  # CosineSimilarity.java:28-45


class PearsonCorrelation(DistanceCalculator):
    name = "pearson"  # PearsonCorrelation.java:28-56


class ManhattanDistance(DistanceCalculator):
    name = "manhattan"  # ManhattanDistance.java:28-41


class SupremumDistance(DistanceCalculator):
    name = "supremum"  # SupremumDistance.java:28-43


def metric_of(distanceFunction) -> int:
    if distanceFunction is None:
        return 0
    if isinstance(distanceFunction, str):
        return A.METRIC[distanceFunction]
    if isinstance(distanceFunction, int):
        return distanceFunction
    return A.METRIC[distanceFunction.getName()]


def distance_rows(a, b, distanceFunction=None, ctx=None):
    aa, bb = A.Arr(a, np.float64), A.Arr(b, np.float64)
    n, d = aa.obj.shape
    out = A.new_like(aa, (n,), np.float64)
    c = A.context_for(ctx, aa)
    A.call("hdb_distance_rows", c.h, aa.p, bb.p, n, d, metric_of(distanceFunction), A.ptr(out))
    return out


# ---------------------------------------------------------- UndirectedGraph
class UndirectedGraph:
    """hdbscanstar/UndirectedGraph.java: parallel edge arrays (+ adjacency on demand)."""

    def __init__(self, verticesA, verticesB, edgeWeights, numVertices: int | None = None):
        self.verticesA = verticesA
        self.verticesB = verticesB
        self.edgeWeights = edgeWeights
        self.numVertices = numVertices

    def _host(self):
        def h(x, dt):
            if A.is_torch(x):
                return np.ascontiguousarray(x.detach().cpu().numpy(), dtype=dt)
            return np.ascontiguousarray(x, dtype=dt)
        return h(self.verticesA, np.int32), h(self.verticesB, np.int32), h(self.edgeWeights, np.float64)

    def quicksortByEdgeWeight(self):
        """UndirectedGraph.java:93-124 (pivot = startIndex quirk), in place on host copies."""
        a, b, w = self._host()
        A.call("hdb_quicksort_edges", A.ptr(a), A.ptr(b), A.ptr(w), w.shape[0], what="quicksortByEdgeWeight")
        self.verticesA, self.verticesB, self.edgeWeights = a, b, w

    def getNumVertices(self):
        return self.numVertices

    def getNumEdges(self):
        return int(self.edgeWeights.shape[0])

    def getFirstVertexAtIndex(self, i):
        return int(self.verticesA[i])

    def getSecondVertexAtIndex(self, i):
        return int(self.verticesB[i])

    def getEdgeWeightAtIndex(self, i):
        return float(self.edgeWeights[i])

    def getVerticeA(self):
        return self.verticesA

    def getVericeB(self):  # sic, UndirectedGraph.java:259
        return self.verticesB

    def getEges(self):  # sic, UndirectedGraph.java:263
        return self.edgeWeights


# --------------------------------------------------------------- HDBSCANStar
class HDBSCANStar:
    """hdbscanstar/HDBSCANStar.java -- the hot-path entry points."""

    def __init__(self, ctx: A.Context | None = None):
        self.ctx = ctx

    def calculateCoreDistances(self, dataSet, k: int, distanceFunction=None,
                               semantics: int = A.CORE_INCL_SELF_CUMULATIVE):
        """HDBSCANStar.java:71-106 (live: the k-NN buffer is never reset between points).
        semantics selects the reference's other variants (CORE_INCL_SELF:
        CoreDistanceMapper.java:71-109, CORE_EXCL_SELF: CreateLocalMST.java:138-185)."""
        X = A.Arr(dataSet, np.float64)
        n, d = X.obj.shape
        core = A.new_like(X, (n,), np.float64)
        c = A.context_for(self.ctx, X)
        A.call("hdb_core_distances", c.h, X.p, n, d, k, metric_of(distanceFunction), semantics, A.ptr(core),
               what="calculateCoreDistances")
        return core

    def constructMST(self, dataSet, coreDistances, selfEdges: bool, distanceFunction=None, indices=None,
                     totalLength=None) -> UndirectedGraph:
        """HDBSCANStar.java:124-205 -- exact reference Prim (totalLength unused, as in Java)."""
        X = A.Arr(dataSet, np.float64)
        n, d = X.obj.shape
        core = A.Arr(coreDistances, np.float64)
        ids = A.Arr(indices, np.int32) if indices is not None else None
        ne = (n - 1) + (n if selfEdges else 0)
        va, vb, w = A.new_edges(X, ne)
        c = A.context_for(self.ctx, X)
        A.call("hdb_prim_mst", c.h, X.p, n, d, core.p, ids.p if ids else None, metric_of(distanceFunction),
               int(bool(selfEdges)), A.ptr(va), A.ptr(vb), A.ptr(w), what="constructMST")
        return UndirectedGraph(va, vb, w)

    def constructLocalMST(self, dataSet, indices, coreDistances, selfEdges: bool, distanceFunction=None,
                          node: int = 0):
        """CreateLocalMST.constructMST (partition/mappers/CreateLocalMST.java:187-292): the
        reference Prim plus its MinimumSpanningTree record fields -- returns (va, vb, w, fake1,
        fake2, node) with fake1 = nearestneighborsID (:242), fake2 = otherVertexIndicesID
        (:266), node (:285); format with formats.format_local_mst (CreateLocalMST.java:110-123)."""
        g = self.constructMST(dataSet, coreDistances, selfEdges, distanceFunction, indices)
        va, vb, w = g.getVerticeA(), g.getVericeB(), g.getEges()
        n = A.Arr(dataSet, np.float64).obj.shape[0]
        ids = A.Arr(indices, np.int32) if indices is not None else None
        a, b, ww = A.Arr(va, np.int32), A.Arr(vb, np.int32), A.Arr(w, np.float64)
        ne = a.obj.shape[0]
        f1, f2, nd = (A.new_like(a, (ne,), np.int32) for _ in range(3))
        c = A.context_for(self.ctx, a)
        A.call("hdb_local_mst_ids", c.h, ids.p if ids else None, n, a.p, b.p, ww.p, ne, int(node), A.ptr(f1),
               A.ptr(f2), A.ptr(nd))
        return va, vb, w, f1, f2, nd

    def constructMSTBoruvka(self, dataSet, coreDistances, selfEdges: bool, distanceFunction=None) -> UndirectedGraph:
        """Large-graph MST: same sorted weights as constructMST, the unique tree under the strict
        edge order (w, s, min id, max id) of include/hdbmi.h; edges sorted by (w, min id, max id),
        then the self edges.  Every distanceFunction and every d: K2b's index for Euclidean
        d in {1, 2, 3, 4, 8, 16}, K2g's tiled all-pairs scan for everything else (cosine and
        Pearson weights can be a few ulps below zero and come back as computed)."""
        X = A.Arr(dataSet, np.float64)
        n, d = X.obj.shape
        core = A.Arr(coreDistances, np.float64)
        ne = (n - 1) + (n if selfEdges else 0)
        va, vb, w = A.new_edges(X, ne)
        c = A.context_for(self.ctx, X)
        A.call("hdb_mst_boruvka", c.h, X.p, n, d, core.p, metric_of(distanceFunction), int(bool(selfEdges)),
               A.ptr(va), A.ptr(vb), A.ptr(w), what="constructMSTBoruvka")
        return UndirectedGraph(va, vb, w)

    def exactMST(self, dataSet, k: int, distanceFunction=None, semantics: int = A.CORE_EXCL_SELF,
                 selfEdges: bool = True, merged: bool = False):
        """FirstStep's leaf branch on one large partition (FirstStep.java:104-108):
        calculateCoreDistances + the exact MRD MST (constructMSTBoruvka's weights and edge
        order) in one call -- sharing one spatial index for K2b's shapes, calculateCoreDistances
        followed by K2g for every other distanceFunction and d.  Returns (core, UndirectedGraph).
        merged: the edges in the reducers' merge order (UnionFindReducer.java:19-69 +
        SortMST.java:9-17) -- what sort_edges_desc returns for the plain list -- without the
        re-sort (HDB_EDGES_MERGED)."""
        X = A.Arr(dataSet, np.float64)
        n, d = X.obj.shape
        ne = (n - 1) + (n if selfEdges else 0)
        core = A.new_like(X, (n,), np.float64)
        va, vb, w = A.new_edges(X, ne)
        c = A.context_for(self.ctx, X)
        flags = (A.EDGES_SELF if selfEdges else 0) | (A.EDGES_MERGED if merged else 0)
        A.call("hdb_exact_mst", c.h, X.p, n, d, k, metric_of(distanceFunction), semantics, flags, A.ptr(core),
               A.ptr(va), A.ptr(vb), A.ptr(w), what="exactMST")
        return core, UndirectedGraph(va, vb, w)

    def knn(self, dataSet, k: int, distanceFunction=None, exclSelf: bool = False, withIndices: bool = False):
        """Per-row k smallest distances (ascending, Double.MAX_VALUE padded) [+ indices]."""
        X = A.Arr(dataSet, np.float64)
        n, d = X.obj.shape
        dist = A.new_like(X, (n, k), np.float64)
        idx = A.new_like(X, (n, k), np.int32) if withIndices else None
        c = A.context_for(self.ctx, X)
        A.call("hdb_knn", c.h, X.p, n, d, k, metric_of(distanceFunction), int(exclSelf), A.ptr(dist), A.ptr(idx),
               what="knn")
        return (dist, idx) if withIndices else dist

    def attachPoints(self, dataSet, coreDistances, queries, k: int, distanceFunction=None, attach_splits: int = 0):
        """The attach scan of out-of-sample prediction (hdb_attach_points): for every row of
        ``queries`` its core distance against ``dataSet`` (the k - 1 nearest training rows, the
        CORE_EXCL_SELF value of the query as one more row), the training row it reaches through
        its cheapest mutual-reachability edge under the strict order (w, s, j) and that weight.
        ``coreDistances`` are the training rows' core distances as the fit computed them.
        Returns (core_q, nearest, level); a query without a candidate has nearest -1 and level
        Double.MAX_VALUE.  Each array may be host or device memory; results live where
        ``queries`` does.  ``attach_splits`` > 0 forces the number of candidate columns the scan
        merges (hdb_attach_points_splits; no bit of the result depends on it)."""
        X, core, Q = A.Arr(dataSet, np.float64), A.Arr(coreDistances, np.float64), A.Arr(queries, np.float64)
        n, d = X.obj.shape
        m = Q.obj.shape[0]
        if Q.obj.ndim != 2 or Q.obj.shape[1] != d:
            raise ValueError("queries must be m x d with the training rows' d")
        if core.obj.shape[0] != n:
            raise ValueError("coreDistances must have one entry per training row")
        core_q, level = A.new_like(Q, (m,), np.float64), A.new_like(Q, (m,), np.float64)
        nearest = A.new_like(Q, (m,), np.int32)
        c = A.context_for(self.ctx, Q, X, core)
        A.call("hdb_attach_points_splits", c.h, X.p, n, d, core.p, Q.p, m, k, metric_of(distanceFunction),
               int(attach_splits), A.ptr(core_q), A.ptr(nearest), A.ptr(level), what="attachPoints")
        return core_q, nearest, level

    def exemplarDistances(self, dataSet, ids, offsets, queries, distanceFunction=None, splits: int = 0):
        """The exemplar-distance scan of soft clustering (hdb_exemplar_distances): ``dmin`` (m x C)
        with dmin[i][f - 1] = the smallest distance from row i of ``queries`` (the query row first)
        to the rows ``dataSet[ids[e]]`` of segment f, offsets[f - 1] <= e < offsets[f]; +inf for an
        empty segment, a NaN distance is no candidate.  ``ids`` / ``offsets`` as exemplars returns
        them, or any arrays of that form (ids in 0..n-1, offsets ascending from 0 to len(ids)).  Each
        array may be host or device memory; the result lives where ``queries`` does.  ``splits`` > 0
        forces the number of candidate columns the scan merges (no bit of the result depends on it).
        Memory: the output is m * C doubles; scratch beyond it is the gathered and packed exemplar
        rows, the packed queries and splits * m * C partial minima -- chunk ``queries`` when that is
        too much."""
        X, Q = A.Arr(dataSet, np.float64), A.Arr(queries, np.float64)
        ia, oa = A.Arr(ids, np.int32), A.Arr(offsets, np.int64)
        n, d = X.obj.shape
        m = Q.obj.shape[0]
        if Q.obj.ndim != 2 or Q.obj.shape[1] != d:
            raise ValueError("queries must be m x d with the training rows' d")
        if oa.obj.ndim != 1 or oa.obj.shape[0] < 1 or ia.obj.ndim != 1:
            raise ValueError("offsets needs C + 1 entries, ids one per exemplar")
        C = int(oa.obj.shape[0]) - 1
        dmin = A.new_like(Q, (m, C), np.float64)
        c = A.context_for(self.ctx, Q, X, ia, oa)
        A.call("hdb_exemplar_distances_splits", c.h, X.p, n, d, ia.p, int(ia.obj.shape[0]), oa.p, C, Q.p, m,
               metric_of(distanceFunction), int(splits), A.ptr(dmin), what="exemplarDistances")
        return dmin


def flat_labels(va, vb, w, n: int, minClSize: int, ctx=None):
    """Global HDBSCAN* flat partition over a merged MST (the reference's
    Main.java:351-408 never completes it): HDBSCANStar.java:208-625 semantics, canonical tie
    rules.  Returns (labels[n] with 1..K by smallest member id and 0 = noise, K).
    Device tensors, or any arrays with a ctx, run the device algorithm (K6, csrc/flat.hip);
    host arrays without a ctx run the host algorithm (csrc/flat.cpp) with no device."""
    a, b, ww = A.Arr(va, np.int32), A.Arr(vb, np.int32), A.Arr(w, np.float64)
    labels = A.new_like(a, (n,), np.int32)
    k = np.zeros(1, np.int64)
    c = A.context_for(ctx, a, host_ok=True)
    A.call("hdb_flat_labels", c.h if c else None, a.p, b.p, ww.p, ww.obj.shape[0], n, minClSize, A.ptr(labels),
           A.ptr(k), what="flat_labels")
    return labels, int(k[0])


def outlier_scores(va, vb, w, n: int, minClSize: int, ctx=None, with_labels: bool = False):
    """GLOSH outlier scores over the merged MST's hierarchy (HDBSCANStar.propagateTree :505-540,
    calculateOutlierScores :653-686; the hierarchy and tie rules of flat_labels).  Returns
    (scores[n], noise_level[n]), or (scores, noise_level, labels, K) with with_labels -- labels
    and scores then come from the one hierarchy the call builds.

    noise_level[x] = eps(x), the level at which x becomes noise; scores[x] = 0 when eps(x) == 0,
    else 1 - eps_max(last(x)) / eps(x), with eps_max the lowest death level among the cluster x
    leaves from and its descendants.  For the root cluster only its descendants count, and a root
    that never splits into two valid children keeps Java's initial Double.MAX_VALUE
    (Cluster.java:57,99-105): points leaving such a root get the reference's huge negative (or
    -inf) scores, not a clamped value.  Device and host selection as in flat_labels."""
    a, b, ww = A.Arr(va, np.int32), A.Arr(vb, np.int32), A.Arr(w, np.float64)
    scores = A.new_like(a, (n,), np.float64)
    noise = A.new_like(a, (n,), np.float64)
    labels = A.new_like(a, (n,), np.int32) if with_labels else None
    k = np.zeros(1, np.int64)
    c = A.context_for(ctx, a, host_ok=True)
    A.call("hdb_flat_outlier_scores", c.h if c else None, a.p, b.p, ww.p, ww.obj.shape[0], n, minClSize, A.ptr(scores),
           A.ptr(noise), A.ptr(labels), A.ptr(k) if with_labels else None, what="outlier_scores")
    return (scores, noise, labels, int(k[0])) if with_labels else (scores, noise)


def outlier_ranking(scores, core):
    """The order calculateOutlierScores writes the points in: ascending (score, core distance,
    id) under OutlierScore.compareTo's > / < comparisons (OutlierScore.java:36-50), so -0.0
    ties 0.0.  Defined for non-NaN scores.  Returns the permutation (int64, host)."""
    def host(x):
        if A.is_torch(x):
            x = x.detach().cpu().numpy()
        return np.ascontiguousarray(x, dtype=np.float64) + 0.0  # -0.0 + 0.0 == +0.0: one key per value
    s, c = host(scores), host(core)
    return np.lexsort((np.arange(s.shape[0]), c, s)).astype(np.int64)


class ClusterTree:
    """The condensed cluster tree of hdb_flat_cluster_tree.  Entry i of a per-cluster array
    describes TREE LABEL i + 1 (1 = the root; 0 = noise / no parent): ``parent``, ``birth`` (NaN
    for the root), ``death``, ``stability`` (NaN for the root), ``size``, ``min_id``,
    ``flat_label`` (1..n_clusters when FOSC selected the cluster, else 0).  Per point:
    ``point_cluster`` (the tree label the point leaves as noise from) and ``point_level`` (the
    level at which it leaves, the noise level of outlier_scores).  Arrays are numpy arrays or
    torch tensors, as the edges given to cluster_tree were."""

    FIELDS = ("parent", "birth", "death", "stability", "size", "min_id", "flat_label", "point_cluster", "point_level")

    def __init__(self, parent, birth, death, stability, size, min_id, flat_label, point_cluster, point_level,
                 n_clusters):
        self.parent, self.birth, self.death, self.stability = parent, birth, death, stability
        self.size, self.min_id, self.flat_label = size, min_id, flat_label
        self.point_cluster, self.point_level = point_cluster, point_level
        self.n_clusters = int(n_clusters)

    @property
    def n_tree(self) -> int:
        return int(self.parent.shape[0])

    @property
    def n(self) -> int:
        return int(self.point_cluster.shape[0])

    def host(self) -> "ClusterTree":
        """The same record with numpy arrays."""
        f = [getattr(self, k) for k in self.FIELDS]
        return ClusterTree(*[x.detach().cpu().numpy() if A.is_torch(x) else np.asarray(x) for x in f], self.n_clusters)

    def _t(self, name):
        import torch
        x = getattr(self, name)
        return x if A.is_torch(x) else torch.from_numpy(np.ascontiguousarray(x))

    def _back(self, t):
        return t if A.is_torch(self.parent) else t.numpy()

    def flat_labels(self):
        """The flat partition of flat_labels, re-derived from the tree: flat_label of the nearest
        selected cluster on the path from a point's last cluster to the root (pointer doubling
        over the K clusters, one gather per point)."""
        import torch
        near, up, pc = self._t("flat_label").clone(), self._t("parent").to(torch.int64), self._t("point_cluster")
        for _ in range(max(1, self.n_tree).bit_length()):
            has = up > 0
            idx = (up - 1).clamp(min=0)
            near = torch.where((near == 0) & has, near[idx], near)
            up = torch.where(has, up[idx], up)
        if self.n == 0:
            return self._back(pc.clone())
        return self._back(near[pc.to(torch.int64) - 1])

    def outlier_scores(self):
        """The GLOSH scores of outlier_scores, re-derived from the tree (bit-identical): eps_max is
        the subtree minimum of ``death`` (for the root: its descendants only, Double.MAX_VALUE
        when it has none), score = 0 where point_level is 0, else 1 - eps_max / point_level."""
        import torch
        K = self.n_tree
        em = self._t("death").clone()
        par = self._t("parent").to(torch.int64)
        if K:
            em[0] = em[1:].min() if K > 1 else A.JMAX
        up = torch.where(par <= 1, torch.zeros_like(par), par)  # nothing propagates into the root
        while bool((up > 0).any()):
            live = up > 0
            em.scatter_reduce_(0, up[live] - 1, em[live], "amin")
            up = torch.where(live, up[(up - 1).clamp(min=0)], up)
        eps = self._t("point_level")
        if self.n == 0:
            return self._back(eps.clone())
        e = em[self._t("point_cluster").to(torch.int64) - 1]
        return self._back(torch.where(eps == 0, torch.zeros_like(eps), 1.0 - e / eps))


def cluster_tree_bound(n: int, minClSize: int) -> int:
    """hdb_cluster_tree_bound: max(1, 2 * (n // minClSize) - 1) clusters at most (0 for n <= 0)."""
    return int(A.lib().hdb_cluster_tree_bound(int(n), int(minClSize)))


def cluster_tree(va, vb, w, n: int, minClSize: int, ctx=None) -> ClusterTree:
    """The condensed cluster tree of the hierarchy flat_labels builds (HDBSCANStar.
    computeHierarchyAndClusterTree :208-474; include/hdbmi.h hdb_flat_cluster_tree, DESIGN.md
    "cluster tree"): a ClusterTree whose per-cluster arrays are sized with the bound and trimmed
    to the K clusters found.  Tensors in give tensors out; device and host selection as in
    flat_labels."""
    a, b, ww = A.Arr(va, np.int32), A.Arr(vb, np.int32), A.Arr(w, np.float64)
    cap = max(cluster_tree_bound(n, max(int(minClSize), 2)), 1)
    i32 = [A.new_like(a, (cap,), np.int32) for _ in range(4)]
    f64 = [A.new_like(a, (cap,), np.float64) for _ in range(3)]
    pc, pl = A.new_like(a, (n,), np.int32), A.new_like(a, (n,), np.float64)
    kt, k = np.zeros(1, np.int64), np.zeros(1, np.int64)
    c = A.context_for(ctx, a, host_ok=True)
    A.call("hdb_flat_cluster_tree", c.h if c else None, a.p, b.p, ww.p, ww.obj.shape[0], n, minClSize, cap, A.ptr(kt),
           A.ptr(i32[0]), A.ptr(f64[0]), A.ptr(f64[1]), A.ptr(f64[2]), A.ptr(i32[1]), A.ptr(i32[2]), A.ptr(i32[3]),
           A.ptr(pc), A.ptr(pl), A.ptr(k), what="cluster_tree")
    K = int(kt[0])
    return ClusterTree(i32[0][:K], f64[0][:K], f64[1][:K], f64[2][:K], i32[1][:K], i32[2][:K], i32[3][:K], pc, pl,
                       int(k[0]))


def labels_at_levels(tree: ClusterTree, levels, ctx=None):
    """Hierarchy rows at arbitrary levels (hdb_labels_at_levels): an (L, n) int32 array whose row
    l holds the tree labels while every edge of weight <= levels[l] is still present (0 = noise).
    Levels in any order, duplicates and +-inf allowed; NaN raises.  The tree's arrays and the
    levels may each be host or device memory; the result lives where the tree's points do."""
    par, bi = A.Arr(tree.parent, np.int32), A.Arr(tree.birth, np.float64)
    pc, pl = A.Arr(tree.point_cluster, np.int32), A.Arr(tree.point_level, np.float64)
    lv = A.Arr(levels if A.is_torch(levels) else np.atleast_1d(np.asarray(levels, dtype=np.float64)), np.float64)
    L, n, K = int(lv.obj.shape[0]), int(pc.obj.shape[0]), int(par.obj.shape[0])
    out = A.new_like(pc, (L, n), np.int32)
    c = A.context_for(ctx, pc, par, lv, host_ok=True)
    A.call("hdb_labels_at_levels", c.h if c else None, par.p, bi.p, K, pc.p, pl.p, n, lv.p, L, A.ptr(out),
           what="labels_at_levels")
    return out


def predict_labels(tree: ClusterTree, nearest, level, flat_label=None, ctx=None):
    """hdb_predict_labels: queries attached to training point nearest[i] at level[i] read their
    tree label (the walk of labels_at_levels from the point's last cluster, without its noise
    rule), their flat label (``flat_label`` per cluster: the tree's own by default, or the one
    constrained_flat_labels returns) and their GLOSH score at max(level, point_level[nearest]).
    nearest -1: (0, 0, 1.0).  Returns (tree_labels, labels, scores) where ``nearest`` lives; host
    arrays without a ctx run on the host with no device."""
    par, bi, de = A.Arr(tree.parent, np.int32), A.Arr(tree.birth, np.float64), A.Arr(tree.death, np.float64)
    fl = A.Arr(tree.flat_label if flat_label is None else flat_label, np.int32)
    pc, pl = A.Arr(tree.point_cluster, np.int32), A.Arr(tree.point_level, np.float64)
    nr, lv = A.Arr(nearest, np.int32), A.Arr(level, np.float64)
    K, n, m = int(par.obj.shape[0]), int(pc.obj.shape[0]), int(nr.obj.shape[0])
    if fl.obj.shape[0] != K or lv.obj.shape[0] != m:
        raise ValueError("flat_label needs one entry per cluster, level one per query")
    tl, lab = A.new_like(nr, (m,), np.int32), A.new_like(nr, (m,), np.int32)
    sc = A.new_like(nr, (m,), np.float64)
    c = A.context_for(ctx, nr, lv, pc, par, fl, host_ok=True)
    A.call("hdb_predict_labels", c.h if c else None, par.p, bi.p, de.p, fl.p, K, pc.p, pl.p, n, nr.p, lv.p, m,
           A.ptr(tl), A.ptr(lab), A.ptr(sc), what="predict_labels")
    return tl, lab, sc


class Prediction:
    """The result of approximate_predict, one entry per query: ``labels`` (flat; 0 = noise),
    ``tree_labels``, ``nearest`` (the training row attached to, -1 = none), ``level`` (the
    mutual-reachability weight of that edge), ``core`` (the query's core distance) and ``scores``
    (GLOSH)."""

    def __init__(self, labels, tree_labels, nearest, level, core, scores):
        self.labels, self.tree_labels, self.nearest = labels, tree_labels, nearest
        self.level, self.core, self.scores = level, core, scores


def approximate_predict(tree: ClusterTree, X, core, Q, minPts: int, distanceFunction=None, flat_label=None,
                        ctx=None) -> Prediction:
    """fit, then predict: classifies rows that were not in the fit without refitting.  Each row
    of Q is attached to the fitted hierarchy through its cheapest mutual-reachability edge into
    the training rows X (HDBSCANStar.attachPoints; ``core`` = their core distances, e.g. from
    exactMST) and reads the cluster at that level out of ``tree`` (predict_labels).  Tensors in
    give tensors out; the results live where Q does."""
    core_q, nearest, level = HDBSCANStar(ctx).attachPoints(X, core, Q, minPts, distanceFunction)
    tl, lab, sc = predict_labels(tree, nearest, level, flat_label, ctx=ctx)
    return Prediction(lab, tl, nearest, level, core_q, sc)


def _selection(tree: ClusterTree, flat_label):
    """(flat_label array, C): the tree's own selection, or the given one with C = its maximum"""
    if flat_label is None:
        return tree.flat_label, tree.n_clusters
    fl = A.Arr(flat_label, np.int32)
    return fl.obj, (max(int(fl.obj.max()), 0) if fl.obj.shape[0] else 0)


def exemplars(tree: ClusterTree, flat_label=None, ctx=None):
    """The exemplars of the selected clusters (hdb_exemplars): the points that leave a leaf of the
    cluster tree at the leaf's smallest point level, each under the flat label of the nearest
    selected cluster above its leaf (``flat_label`` per cluster: the tree's own by default, or the
    one constrained_flat_labels returns).  Returns (ids, offsets): int32 point ids ordered by (flat
    label, id) and int64 offsets with the ids of flat label f at offsets[f - 1]:offsets[f].  The
    arrays live where the tree's points do; host arrays without a ctx need no device."""
    fl_obj, C = _selection(tree, flat_label)
    par, fl = A.Arr(tree.parent, np.int32), A.Arr(fl_obj, np.int32)
    pc, pl = A.Arr(tree.point_cluster, np.int32), A.Arr(tree.point_level, np.float64)
    K, n = int(par.obj.shape[0]), int(pc.obj.shape[0])
    if fl.obj.shape[0] != K:
        raise ValueError("flat_label needs one entry per cluster")
    ids, offsets = A.new_like(pc, (n,), np.int32), A.new_like(pc, (C + 1,), np.int64)
    E = np.zeros(1, np.int64)
    c = A.context_for(ctx, pc, par, fl, host_ok=True)
    A.call("hdb_exemplars", c.h if c else None, par.p, fl.p, K, C, pc.p, pl.p, n, A.ptr(ids), A.ptr(offsets), A.ptr(E),
           what="exemplars")
    return ids[:int(E[0])], offsets


class Membership:
    """The result of membership_vectors, one row per query: ``vectors`` (m x C; entry f - 1 is the
    membership in flat label f, the row sums to ``prob`` or is zero), ``prob`` (how strongly the
    query belongs to any cluster), ``labels`` (the flat label of the row's first maximum, 0 for a
    zero row) and ``dist`` (m x C, the distance to each cluster's nearest exemplar)."""

    def __init__(self, vectors, prob, labels, dist):
        self.vectors, self.prob, self.labels, self.dist = vectors, prob, labels, dist


def membership_vectors(tree: ClusterTree, X, Q=None, core=None, minPts=None, distanceFunction=None, flat_label=None,
                       ctx=None) -> Membership:
    """Soft clustering (hdb_exemplars, hdb_exemplar_distances, hdb_membership_vectors; the
    contract is in include/hdbmi.h): how strongly each row belongs to each selected cluster of the
    fitted ``tree`` over the training rows X.  With ``Q`` None the rows are the training rows, each
    anchored at its own (point_cluster, point_level); otherwise the rows of Q, attached through
    approximate_predict (``core`` = the training rows' core distances and ``minPts`` as there).
    Tensors in give tensors out; the results live where the queries do.  The distance scan needs a
    device.  Memory: ``dist`` and ``vectors`` are m x C doubles each -- chunk the queries when that
    is too much."""
    ids, offsets = exemplars(tree, flat_label, ctx=ctx)
    if Q is None:
        queries, anchor, level = X, tree.point_cluster, tree.point_level
    else:
        if core is None or minPts is None:
            raise ValueError("new rows need the training rows' core distances and minPts")
        queries = Q
        pred = approximate_predict(tree, X, core, Q, minPts, distanceFunction, flat_label, ctx=ctx)
        anchor = pred.tree_labels
        if A.is_torch(pred.level):
            import torch
            pl = tree._t("point_level").to(pred.level.device)[pred.nearest.to(torch.int64).clamp(min=0)]
            level = torch.where(pl > pred.level, pl, pred.level)
        else:
            pl = np.asarray(tree.host().point_level)[np.maximum(pred.nearest, 0)] if tree.n else pred.level
            level = np.where(pl > pred.level, pl, pred.level)
    dist = HDBSCANStar(ctx).exemplarDistances(X, ids, offsets, queries, distanceFunction)
    return membership_rows(tree, anchor, level, dist, flat_label, ctx=ctx)


def membership_rows(tree: ClusterTree, anchor, level, dist, flat_label=None, ctx=None) -> Membership:
    """hdb_membership_vectors on its own: the membership of queries given as anchor clusters (tree
    labels, 0 = none), levels and their rows of exemplar distances (m x C).  Results live where
    ``dist`` does; host arrays without a ctx run on the host with no device."""
    fl_obj, C = _selection(tree, flat_label)
    par, bi, de = A.Arr(tree.parent, np.int32), A.Arr(tree.birth, np.float64), A.Arr(tree.death, np.float64)
    fl, an, lv, dm = A.Arr(fl_obj, np.int32), A.Arr(anchor, np.int32), A.Arr(level, np.float64), A.Arr(dist, np.float64)
    K, m = int(par.obj.shape[0]), int(an.obj.shape[0])
    if lv.obj.shape[0] != m or tuple(dm.obj.shape) != (m, C):
        raise ValueError("one anchor, one level and one row of C distances per query")
    vec = A.new_like(dm, (m, C), np.float64)
    prob, lab = A.new_like(dm, (m,), np.float64), A.new_like(dm, (m,), np.int32)
    c = A.context_for(ctx, dm, an, lv, par, fl, host_ok=True)
    A.call("hdb_membership_vectors", c.h if c else None, par.p, bi.p, de.p, fl.p, K, C, an.p, lv.p, dm.p, m, A.ptr(vec),
           A.ptr(prob), A.ptr(lab), what="membership_vectors")
    return Membership(vec, prob, lab, dist)


class Validity:
    """The result of validity_index: ``index`` (the DBCV index, a float in [-1, 1]); per cluster
    (entry c - 1 = label c) ``validity``, ``sparseness``, ``separation``, ``nearest_cluster`` (0:
    none) and ``size``; per row ``core`` (the all-points core distance, 0 for noise) and
    ``internal`` (1: an internal node of its cluster's tree)."""

    def __init__(self, index, validity, sparseness, separation, nearest_cluster, size, core, internal):
        self.index, self.validity, self.sparseness, self.separation = index, validity, sparseness, separation
        self.nearest_cluster, self.size, self.core, self.internal = nearest_cluster, size, core, internal


def validity_index(X, labels, distanceFunction=None, n_clusters=None, ctx=None, splits: int = 0,
                   small_max: int | None = None) -> Validity:
    """How good a labelling is: the DBCV validity index (Moulavi et al., SDM 2014) of ``labels``
    (0 = noise, 1..n_clusters; n_clusters defaults to labels.max()) over the rows of X, under any
    of the five metrics (hdb_validity_index; the contract is in include/hdbmi.h).  Higher is
    better; compare the results of a sweep over minPts, minClSize, the metric or a level cut by
    it.  numpy arrays or torch device tensors; the arrays of the result live where X does.
    ``splits`` > 0 forces the candidate-column count of both scans and ``small_max`` the size up to
    which clusters share the one Prim launch (0: every cluster through Boruvka); no bit of the
    result depends on either."""
    Xa, la = A.Arr(X, np.float64), A.Arr(labels, np.int32)
    if Xa.obj.ndim != 2 or la.obj.shape[0] != Xa.obj.shape[0]:
        raise ValueError("X must be n x d and labels must have one entry per row")
    n, d = Xa.obj.shape
    K = int(n_clusters) if n_clusters is not None else (int(la.obj.max()) if n else 0)
    K = max(K, 0)
    val, spa, sep = (A.new_like(Xa, (K,), np.float64) for _ in range(3))
    near, size = A.new_like(Xa, (K,), np.int32), A.new_like(Xa, (K,), np.int32)
    core, internal = A.new_like(Xa, (n,), np.float64), A.new_like(Xa, (n,), np.int32)
    index = A.C.c_double()
    c = A.context_for(ctx, Xa, la)
    A.call("hdb_validity_index_route", c.h, Xa.p, n, d, la.p, K, metric_of(distanceFunction), int(splits),
           1024 if small_max is None else int(small_max), A.C.byref(index), A.ptr(val), A.ptr(spa), A.ptr(sep),
           A.ptr(near), A.ptr(size), A.ptr(core), A.ptr(internal), what="validity_index")
    return Validity(index.value, val, spa, sep, near, size, core, internal)


MUST_LINK, CANNOT_LINK = 0, 1  # HDB_CONSTRAINT_*


class ConstrainedLabels:
    """The result of constrained_flat_labels: ``labels`` (n; 1..n_clusters, 0 = noise),
    ``n_clusters``, and per cluster (entry i = tree label i + 1) ``flat_label``, ``num_sat``
    (numConstraintsSatisfied), ``prop_sat`` and ``prop_stability`` (the propagated values);
    ``m`` constraints, ``satisfied_fraction`` = 0.5 * prop_sat[root] / m as the reference prints
    it (NaN for m == 0, Java's 0.0 / 0)."""

    def __init__(self, labels, n_clusters, flat_label, num_sat, prop_sat, prop_stability, m):
        self.labels, self.n_clusters, self.flat_label = labels, int(n_clusters), flat_label
        self.num_sat, self.prop_sat, self.prop_stability, self.m = num_sat, prop_sat, prop_stability, int(m)

    @property
    def satisfied_fraction(self) -> float:
        if self.m == 0 or self.prop_sat.shape[0] == 0:
            return float("nan")
        return 0.5 * int(self.prop_sat[0]) / self.m


def constrained_flat_labels(tree: ClusterTree, ca, cb, ctype, ctx=None) -> ConstrainedLabels:
    """Semi-supervised flat extraction (hdb_constrained_flat_labels; DESIGN.md "Constrained flat
    labels"): the FOSC selection of the tree under must-link (ctype 0) and cannot-link (ctype 1)
    pairs of point ids -- a cluster that satisfies more constraints than its descendants is kept,
    stability breaks ties.  Without constraints the result equals tree.flat_label /
    tree.flat_labels().  The tree's arrays and the constraints may each be host or device memory;
    tensors in give tensors out (the results live where the tree's arrays do)."""
    par, st, mi = A.Arr(tree.parent, np.int32), A.Arr(tree.stability, np.float64), A.Arr(tree.min_id, np.int32)
    pc = A.Arr(tree.point_cluster, np.int32)
    a, b, t = A.Arr(ca, np.int32), A.Arr(cb, np.int32), A.Arr(ctype, np.int32)
    K, n, m = int(par.obj.shape[0]), int(pc.obj.shape[0]), int(a.obj.shape[0])
    if b.obj.shape[0] != m or t.obj.shape[0] != m:
        raise ValueError("ca, cb and ctype must have one entry per constraint")
    num, prop, flat = (A.new_like(par, (K,), np.int32) for _ in range(3))
    pst = A.new_like(par, (K,), np.float64)
    labels = A.new_like(pc, (n,), np.int32)
    k = np.zeros(1, np.int64)
    c = A.context_for(ctx, pc, par, st, mi, a, b, t, host_ok=True)
    A.call("hdb_constrained_flat_labels", c.h if c else None, par.p, st.p, mi.p, K, pc.p, n, a.p, b.p, t.p, m,
           A.ptr(num), A.ptr(prop), A.ptr(pst), A.ptr(flat), A.ptr(labels), A.ptr(k), what="constrained_flat_labels")
    return ConstrainedLabels(labels, int(k[0]), flat, num, prop, pst, m)
