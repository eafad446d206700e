"""tests/validity_reference.py restates the contract of hdb_validity_index (include/hdbmi.h); these
tests pin the restatement itself, on the CPU: a vector worked by hand, the fallback of contract
item 3, the two-level shape of the sum, and the sign of the index on blobs."""
import math

import numpy as np

from conftest import blobs
from metric_kruskal import kruskal_mst_metric
from path_helpers import bits_eq
import validity_reference as V

INF = math.inf


def check(got, **want):
    for k, v in want.items():
        if k == "index":
            assert got[k] == v, (k, got[k], v)
        elif np.asarray(v).dtype.kind == "f":
            assert bits_eq(got[k], np.asarray(v, np.float64)), (k, got[k], v)
        else:
            assert np.array_equal(got[k], np.asarray(v)), (k, got[k], v)


def test_hand_worked_d1(oracle):
    """d = 1, every distance inside a cluster a power of two (or 0: a duplicate, which contributes
    nothing but counts in n_c - 1).
    cluster 1 = rows 0, 1, 2 at 0, 2, 2: row 0 sums 1/2 + 1/2 = 1, / 2, ^-1 = 2; rows 1 and 2 sum
      1/2, / 2, ^-1 = 4.  Every pair weighs 4; by s the tree is (1, 2) then (0, 1): one node of
      degree 2, no internal edge, so all members and both edges are internal: sparseness 4.
    cluster 2 = rows 4, 5 at 10, 12: cores 2, 2, one edge of weight 2.
    cluster 3 is empty.  Rows 3, 6, 7 are noise (row 6 is NaN: never read).
    separation: the closest pair is 2 -- 10 at distance 8 (cores 4 and 2): 8 for both clusters.
    validity = (8 - 4) / 8 and (8 - 2) / 8; index = 3/8 * 0.5 + 2/8 * 0.75 = 0.375."""
    X = np.array([[0.0], [2.0], [2.0], [100.0], [10.0], [12.0], [np.nan], [-50.0]])
    labels = np.array([1, 1, 1, 0, 2, 2, 0, 0])
    r = V.validity_reference(X, labels, 3, "euclidean")
    check(r, index=0.375, validity=[0.5, 0.75, 0.0], sparseness=[4.0, 2.0, 0.0], separation=[8.0, 8.0, INF],
          nearest_cluster=[2, 1, 0], size=[3, 2, 0], core=[2.0, 4.0, 4.0, 0.0, 2.0, 2.0, 0.0, 0.0],
          internal=[1, 1, 1, 0, 1, 1, 0, 0])


def test_hand_worked_d2(oracle):
    """d = 2, Manhattan and Euclidean alike (the pairs inside a cluster differ in one coordinate).
    cluster 1 = (0, 0), (0, 2): t = 1/2, t^2 = 1/4, (1/4)^(-1/2) = 2: cores 2, sparseness 2.
    cluster 2 = (8, 0), (8, 4): t^2 = 1/16, cores 4, sparseness 4.
    separation: (0, 0) -- (8, 0) at distance 8 under both metrics, the cores are smaller: 8.
    validity = 6/8 and 4/8; four noise rows: index = 2/8 * 0.75 + 2/8 * 0.5 = 0.3125."""
    X = np.array([[0.0, 0.0], [50.0, 50.0], [0.0, 2.0], [8.0, 0.0], [-50.0, 3.0], [8.0, 4.0], [7.0, 70.0], [1.0, -90.0]])
    labels = np.array([1, 0, 1, 2, 0, 2, 0, 0])
    for metric in ("euclidean", "manhattan"):
        r = V.validity_reference(X, labels, 2, metric)
        check(r, index=0.3125, validity=[0.75, 0.5], sparseness=[2.0, 4.0], separation=[8.0, 8.0],
              nearest_cluster=[2, 1], size=[2, 2], core=[2.0, 0.0, 2.0, 4.0, 0.0, 4.0, 0.0, 0.0],
              internal=[1, 0, 1, 1, 0, 1, 0, 0])


def test_internal_nodes_and_the_fallback(oracle):
    """clusters of 1, 2 and 3 members and a star have no internal edge: every member is internal
    and the sparseness is the largest tree edge (0 for the singleton); a path of four has one
    internal edge, the middle one"""
    parts = [
        np.array([[100.0, 100.0]]),                                              # 1: singleton
        np.array([[200.0, 0.0], [201.0, 0.0]]),                                  # 2: a pair
        np.array([[300.0, 0.0], [301.0, 0.0], [303.0, 0.0]]),                    # 3: three on a line
        np.array([[0.0, 0.0], [1.0, 0.0], [-1.0, 0.0], [0.0, 1.0], [0.0, -1.0]]),  # 4: a star
        np.array([[400.0, 0.0], [401.0, 0.0], [402.0, 0.0], [403.0, 0.0]]),      # 5: a path
    ]
    X = np.concatenate(parts)
    labels = np.concatenate([np.full(p.shape[0], c + 1) for c, p in enumerate(parts)])
    r = V.validity_reference(X, labels, 5, "euclidean")
    trees = {}
    for c in range(2, 6):
        idx = np.flatnonzero(labels == c)
        trees[c] = kruskal_mst_metric(X[idx], r["core"][idx], "euclidean")
    assert np.bincount(np.concatenate(trees[4][:2]))[0] == 4  # the star's centre holds every edge
    assert r["internal"][labels <= 4].tolist() == [1] * 11
    assert r["sparseness"][0] == 0.0 and r["core"][0] == 0.0
    for c in (2, 3, 4):
        assert r["sparseness"][c - 1] == trees[c][2].max()
    assert r["internal"][labels == 5].tolist() == [0, 1, 1, 0]
    lo, hi, w = trees[5]
    assert r["sparseness"][4] == w[(np.minimum(lo, hi) == 1) & (np.maximum(lo, hi) == 2)][0]
    assert np.all(r["separation"] < INF) and np.all(r["nearest_cluster"] > 0)


def test_blocked_sum_is_not_the_plain_sum(oracle):
    """600 members are two sum blocks: the two-level total of some member differs in its bits from
    the left-to-right total of the same terms, and the reference's cores are the two-level ones"""
    rng = np.random.default_rng(77)
    X = rng.normal(0.0, 1.0, size=(600, 3))
    D = V.dist_matrix(X, "euclidean")
    contributes = (D > 0) & ~np.eye(600, dtype=bool)
    with np.errstate(divide="ignore"):
        p = V.powi(1.0 / D, 3)
    blocked, plain = V.blocked_totals(p, contributes), V.plain_totals(p, contributes)
    differ = blocked.view(np.uint64) != plain.view(np.uint64)
    assert differ.any()
    assert np.allclose(blocked, plain, rtol=1e-12, atol=0.0)
    r = V.validity_reference(X, np.ones(600, np.int32), 1, "euclidean", D=D)
    want = np.array([math.pow(t / 599.0, -1.0 / 3) for t in blocked.tolist()])
    assert bits_eq(r["core"], want)


def test_index_sign_on_blobs(oracle):
    """the generating labels of well-separated blobs score above 0, uniformly random labels on the
    same rows below 0 (a prototype of this contract gave about +0.46 .. +0.72 and -0.70)"""
    for d in (2, 5, 24):
        seed = 900 + d
        X = np.round(blobs(300, d, 4, seed, spread=10.0), 1)
        rng = np.random.default_rng(seed)  # conftest.blobs replayed up to the assignment
        rng.uniform(-10.0, 10.0, size=(4, d))
        true = V.with_noise(rng.integers(0, 4, size=300) + 1, 0.1, seed)
        shuffled = np.where(true > 0, np.random.default_rng(seed + 1).integers(1, 5, 300), 0)
        D = V.dist_matrix(X, "euclidean")
        good = V.validity_reference(X, true, 4, "euclidean", D=D)["index"]
        bad = V.validity_reference(X, shuffled, 4, "euclidean", D=D)["index"]
        print("d", d, "true", good, "random", bad)
        assert good > 0 > bad, (d, good, bad)
