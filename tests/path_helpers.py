"""Shared helpers of the tests that switch runtime options (test_gpu_paths.py and the rows added
to the older files): an option scope that always restores the defaults, and the independent
Kruskal reference for the exact-leaf MST."""
import contextlib
import functools

import numpy as np

# hdb_ctx's defaults (csrc/common.hpp): every name hdb_ctx_set_option accepts
DEFAULTS = {
    "knn_fp32_screen": 1, "knn_tree": 1, "knn_tree_min_n": 8192, "knn_mfma": 1, "knn_mfma_min_n": 2048,
    "knn_mfma_single": 1, "knn_mfma_prune": 1, "nearest_grouped": 1,
    "boruvka_seed": 1, "leaf_seed_k": -1, "leaf_list_rounds": 2, "boruvka_knn_seed": 1, "boruvka_wave_pts": 64,
    "boruvka_early_pts": 0, "boruvka_early_rounds": 5, "boruvka_adj_seed": 1, "bor_xcd_chunks": 8,
    "k1t_xcd_chunks": 8, "trav_pop_test": 0,
    "prim_coop": 1, "prim_coop_plain": 1, "prim_coop_xcd": 1, "prim_coop_bs": 1024, "prim_coop_plain_spin_log2": 20,
    "prim_coop_slots": 4, "bubble_fold_dim": 1, "bubble_knn_split": 1,
    "flat_link_variant": 1, "flat_root_variant": 3, "flat_relabel": 1, "flat_block_log": 10, "flat_mid_log": 12,
    "flat_deep_depth": 64, "flat_deep_root": 3, "flat_deep_link": 1,
    "ssort": 1, "ssort_cap": 0, "count_evals": 0,
}


@contextlib.contextmanager
def options(ctx, **kw):
    """set the options for the block, back to the library defaults after it (also on an error)"""
    for k in kw:
        assert k in DEFAULTS, k
    try:
        for k, v in kw.items():
            ctx.set_option(k, v)
        yield
    finally:
        for k in kw:
            ctx.set_option(k, DEFAULTS[k])


def bits_eq(a, b):
    """bit equality of two float64 arrays (NaNs compare equal to NaNs)"""
    a, b = np.ascontiguousarray(a, np.float64), np.ascontiguousarray(b, np.float64)
    if a.shape != b.shape:
        return False
    na, nb = np.isnan(a), np.isnan(b)
    return np.array_equal(na, nb) and np.array_equal(np.where(na, 0.0, a).view(np.uint64),
                                                     np.where(nb, 0.0, b).view(np.uint64))


def k1m_launches(ctx):
    """(screen or two-pass kernel launches, log re-check launches, k-means layouts) since the last
    call, on a context with timing on: the single pass is (1, 1, .), the two-pass kernel alone
    (1, 0, 0), a single pass whose log overflowed (2, 1, .)"""
    return tuple(ctx.kernel_time(k, reset=True)[1] for k in ("knn_mfma", "knn_mfma_final", "knn_mfma_order"))


@functools.lru_cache(maxsize=4)
def _pairs(n):
    i, j = np.triu_indices(n, 1)
    return i.astype(np.int32), j.astype(np.int32)


def kruskal_mst(X, core):
    """The minimum spanning tree of the mutual-reachability graph under the exact leaf's strict
    total edge order (w, s, lo, hi) (csrc/spatial.hip key_less, DESIGN "Exact pruning"): w =
    max(sqrt(s), core_lo, core_hi), s the squared distance summed in dimension order
    (EuclideanDistance.java:31-33, every operation rounded once), lo < hi the point indices.
    A total order makes the MST unique, so plain Kruskal over all pairs pins every edge.
    A pair whose weight is NaN is not an edge; if the rest does not span, ValueError names the
    rows outside the largest component.  Returns (lo, hi, w) of the n - 1 edges in key order.

    All pairs are formed at once (vectorised); the sorted prefix is consumed in chunks, and
    after each chunk the pairs inside one component are dropped, so the Python union-find loop
    sees a few n pairs in all."""
    X = np.ascontiguousarray(X, np.float64)
    core = np.ascontiguousarray(core, np.float64)
    n, d = X.shape
    i, j = _pairs(n)
    with np.errstate(over="ignore", under="ignore", invalid="ignore"):
        t = X[i, 0] - X[j, 0]
        s = t * t
        for k in range(1, d):
            t = X[i, k] - X[j, k]
            s = s + t * t
        # weights compare as numbers: + 0.0 turns a -0.0 (from -0.0 cores) into the +0.0 it ties with
        w = np.maximum(np.sqrt(s), np.maximum(core[i], core[j])) + 0.0
    parent = list(range(n))

    def find(x):
        while parent[x] != x:
            parent[x] = parent[parent[x]]
            x = parent[x]
        return x

    out = []
    idx = np.flatnonzero(~np.isnan(w))  # a pair whose weight is NaN is not an edge
    while len(out) < n - 1:
        if idx.shape[0] == 0:
            root = np.fromiter((find(x) for x in range(n)), np.int64, n)
            big = np.bincount(root).argmax()
            raise ValueError("the non-NaN pairs do not span: isolated rows %s" % np.flatnonzero(root != big).tolist())
        take = min(idx.shape[0], 8 * n)
        wi = w[idx]
        sel = wi <= np.partition(wi, take - 1)[take - 1]  # whole tie groups: the rest is strictly heavier
        chunk, idx = idx[sel], idx[~sel]
        chunk = chunk[np.lexsort((j[chunk], i[chunk], s[chunk], w[chunk]))]
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


# tie-heavy inputs of the Kruskal reference: (kind, d, n, minPts); blobs at EXCL_SELF cores,
# the Skin prefix (duplicates: zero-weight ties) at the live cumulative ones
MST_CASES = [("blobs", d, n, mp) for d in (1, 2, 3, 8, 16) for n in (65, 3000) for mp in (2, 4, 9)] + \
            [("skin", 3, 3000, 4)]


@functools.lru_cache(maxsize=None)
def mst_case(kind, d, n, mp):
    """(X, semantics, oracle core distances, kruskal_mst of them), computed once per process"""
    from conftest import blobs, load_skin
    from oracle import oracle as O
    O.lib()
    if kind == "skin":
        X, sem = load_skin(n), 0
    else:
        X, sem = np.round(blobs(n, d, 6, 100 * d + n % 7 + mp), 1), 2
    core = O.core_distances(X, mp, semantics=sem)
    lo, hi, w = kruskal_mst(X, core)
    for a in (X, core, lo, hi, w):
        a.setflags(write=False)
    return X, sem, core, (lo, hi, w)


def edge_set(va, vb, w):
    """{(min, max, weight bits)} of an edge list"""
    va, vb = np.asarray(va, np.int64), np.asarray(vb, np.int64)
    wb = np.ascontiguousarray(w, np.float64).view(np.uint64)
    return set(zip(np.minimum(va, vb).tolist(), np.maximum(va, vb).tolist(), wb.tolist()))


def spanning_tree(va, vb, n):
    """host union-find: the n - 1 edges connect all n points without a cycle"""
    p = list(range(n))

    def find(x):
        while p[x] != x:
            p[x] = p[p[x]]
            x = p[x]
        return x
    assert len(va) == n - 1
    for a, b in zip(np.asarray(va).tolist(), np.asarray(vb).tolist()):
        ra, rb = find(a), find(b)
        assert ra != rb, "cycle"
        p[rb] = ra
    return True
