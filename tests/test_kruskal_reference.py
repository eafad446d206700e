"""The Kruskal reference of the exact-leaf MST (path_helpers.kruskal_mst) checked on the CPU
before any device result is compared with it: on every input of the GPU test its sorted weights
equal the reference Prim's (oracle.prim_mst, HDBSCANStar.java:124-205) bit for bit, and its edges
span.  No device needed."""
import numpy as np
import pytest

from path_helpers import MST_CASES, bits_eq, kruskal_mst, mst_case, spanning_tree


@pytest.mark.parametrize("kind,d,n,mp", MST_CASES)
def test_kruskal_reference_weights_equal_prim_and_span(oracle, kind, d, n, mp):
    X, sem, core, (lo, hi, w) = mst_case(kind, d, n, mp)
    assert spanning_tree(lo, hi, n)
    assert np.all(lo < hi)
    _, _, pw = oracle.prim_mst(X, core, self_edges=False)
    assert bits_eq(np.sort(w), np.sort(pw))
    assert np.all(np.diff(w) >= 0)  # key order: weights ascending


def test_kruskal_reference_tiny_by_hand():
    """four collinear points, cores all 1: every pair closer than 1 weighs 1 and the ties go by
    the squared distance, then the ids"""
    X = np.array([[0.0], [0.5], [0.75], [3.0]])
    lo, hi, w = kruskal_mst(X, np.ones(4))
    assert list(zip(lo.tolist(), hi.tolist(), w.tolist())) == [(1, 2, 1.0), (0, 1, 1.0), (2, 3, 2.25)]
