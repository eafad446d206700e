"""The Kruskal reference of the exact-leaf MST (path_helpers.kruskal_mst) checked on the CPU
before any device result is compared with it: on every input of the GPU test its sorted weights
equal the reference Prim's (oracle.prim_mst, HDBSCANStar.java:124-205) bit for bit, and its edges
span.  No device needed."""
import numpy as np
import pytest

from degenerate_inputs import MST_SETTINGS, NAN_ROWS, SPANNING_FINITE, SPANNING_INF, family, family_case
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


@pytest.mark.parametrize("mp,sem", MST_SETTINGS)
@pytest.mark.parametrize("name", SPANNING_FINITE)
def test_kruskal_reference_degenerate_finite_families_equal_prim(oracle, name, mp, sem):
    """pure ties, zero spans, underflowing squares: every weight is finite, so the sorted weights
    are the reference Prim's bit for bit"""
    X, core, (lo, hi, w) = family_case(name, mp, sem)
    n = X.shape[0]
    assert spanning_tree(lo, hi, n) and np.all(lo < hi) and np.all(np.isfinite(w))
    _, _, pw = oracle.prim_mst(X, core, self_edges=False)
    assert bits_eq(np.sort(w), np.sort(pw))
    assert np.all(np.diff(w) >= 0)
    if name in ("same", "tiny"):
        assert not w.any()
    if name == "lattice3":
        assert np.unique(w).shape[0] == 1


@pytest.mark.parametrize("name", SPANNING_INF)
def test_kruskal_reference_infinite_weight_families_span(name):
    """+inf weights are edges (ordered by s, then the ids); inf_pair spans without its NaN pair"""
    X, core, (lo, hi, w) = family_case(name, 4, 0)
    n = X.shape[0]
    assert spanning_tree(lo, hi, n) and not np.isnan(w).any() and np.isinf(w).any()
    assert not np.any(w[1:] < w[:-1])  # key order (inf - inf is NaN: no diff here)
    if name == "huge":
        assert np.isinf(w).all()
    if name == "inf_pair":
        assert (400, 1600) not in set(zip(lo.tolist(), hi.tolist()))
        assert np.isinf(w).sum() == 2


@pytest.mark.parametrize("name", sorted(NAN_ROWS))
def test_kruskal_reference_reports_nan_rows(oracle, name):
    X, _ = family(name)
    core = oracle.core_distances(X, 4, semantics=0)
    with pytest.raises(ValueError, match="isolated rows %s" % str(NAN_ROWS[name]).replace("[", r"\[").replace("]", r"\]")):
        kruskal_mst(X, core)
