"""tests/metric_kruskal.py validated on the CPU: the Kruskal reference of the any-metric exact MST
(K2g) against the oracle's reference Prim, and the purpose of each input family."""
import numpy as np
import pytest

from metric_kruskal import METRICS, SHAPES, kruskal_mst_metric, metric_case, pair_distances, rays, zero_row
from path_helpers import bits_eq, kruskal_mst, spanning_tree


@pytest.mark.parametrize("d,n", SHAPES)
@pytest.mark.parametrize("family", ["rounded_blobs", "rays"])
@pytest.mark.parametrize("metric", METRICS)
def test_kruskal_metric_spans_and_has_prims_weights(oracle, metric, family, d, n):
    X, core, (lo, hi, w) = metric_case(metric, family, d, n)
    assert spanning_tree(lo, hi, n) and np.all(lo < hi)
    pw = oracle.prim_mst(X, core, metric=metric, self_edges=False)[2]
    assert bits_eq(np.sort(w), np.sort(pw)), (metric, family, d, n)
    assert np.all(w[1:] >= w[:-1])  # key order: ascending numerically, negative weights first


@pytest.mark.parametrize("d,n", SHAPES)
def test_rays_have_negative_cosine_distances(d, n):
    """the fixture's purpose: distances a few ulps below zero"""
    X = rays(n, d)
    s = pair_distances(X, "cosine")
    assert not np.isnan(s).any() and (s < 0).any(), (d, n, int((s < 0).sum()))
    assert (np.linalg.norm(X, axis=1) > 0).all() and (X.std(axis=1) > 0).all()


def test_zero_row_under_cosine_does_not_span(oracle):
    X = zero_row(65, 5)
    core = oracle.core_distances(X, 4, metric="cosine")
    with pytest.raises(ValueError, match=r"do not span: isolated rows \[7\]"):
        kruskal_mst_metric(X, core, "cosine")


def test_euclidean_is_the_path_helpers_kruskal(oracle):
    from metric_kruskal import rounded_blobs
    X = rounded_blobs(300, 5)
    core = oracle.core_distances(X, 4)
    for a, b in zip(kruskal_mst_metric(X, core, "euclidean"), kruskal_mst(X, core)):
        assert np.array_equal(a.view(np.uint8), b.view(np.uint8))
