"""The inputs of tests/test_gpu_metrics.py have the properties its cases rely on -- asserted from
the CPU oracle alone -- and the oracle's Prim equals a plain-Python transcription of
HDBSCANStar.constructMST where weights are negative or tie."""
import numpy as np
import pytest

import metric_inputs as M
from metric_kruskal import pair_distances
from path_helpers import bits_eq

EREF_NEGATIVE_CLUSTER = -12


@pytest.mark.parametrize("n,d", M.NEGATIVE_PRIM_SHAPES)
@pytest.mark.parametrize("metric", M.ANGULAR)
def test_rays_trees_are_mostly_negative(oracle, metric, n, d):
    """more than half of the tree weights are below zero and at least one is not: a kernel that
    orders negative weights wrongly, or drops them, cannot pass"""
    w = M.tree_weights(M.prim_case(metric, "rays", n, d, 4, M.PRIM_SEM))
    neg = int((w < 0).sum())
    print(f"{metric} rays {n} x {d}: {neg} of {n - 1} tree weights negative")
    assert not np.isnan(w).any()
    assert neg > (n - 1) // 2 and neg < n - 1


@pytest.mark.parametrize("sem", M.SEMANTICS)
@pytest.mark.parametrize("metric", M.ANGULAR)
def test_rays_cores_are_negative_under_every_semantics(oracle, metric, sem):
    _, core = M.core_case(metric, "rays", 1025, 5, 4, sem)
    assert (core < 0).sum() > 512 and not np.isnan(core).any()


@pytest.mark.parametrize("pos", ["7", "_last"])
@pytest.mark.parametrize("metric,family", [("cosine", "zero_row"), ("pearson", "const_row")])
def test_nan_row_has_max_value_core_and_one_max_value_edge(oracle, metric, family, pos):
    n, d = M.BAD_ROW_SHAPE
    row = 7 if pos == "7" else n - 1
    X, core, ids, (va, vb, w) = M.prim_case(metric, family + pos, n, d, 4, M.BAD_ROW_SEM)
    dist = [oracle.distance(X[row], X[j], metric) for j in (0, 1, row, n - 2)]
    assert np.isnan(dist).all()
    assert core[row] == M.DBL_MAX and (core < M.DBL_MAX).sum() == n - 1
    tw = w[:n - 1]
    assert not np.isnan(tw).any() and int((tw == M.DBL_MAX).sum()) == 1
    if row == n - 1:  # the start vertex: no first-step weight is a number, the '<=' select takes vertex n - 2
        assert tw[n - 2] == M.DBL_MAX and va[n - 2] == 0  # never updated: the parent a new int[] holds
    else:
        assert tw[row] == M.DBL_MAX and va[row] == 0


@pytest.mark.parametrize("metric", ["manhattan", "supremum"])
def test_integer_grid_trees_tie(oracle, metric):
    """at least a third of the tree weights are shared with another edge, zero weights included"""
    for n, d in [(300, 5), (1025, 5), (1100, 8), (4096, 3), (4500, 3)]:
        w = M.tree_weights(M.prim_case(metric, "integer_grid", n, d, 4, M.PRIM_SEM))
        _, cnt = np.unique(w, return_counts=True)
        tied = int(cnt[cnt > 1].sum())
        print(f"{metric} integer_grid {n} x {d}: {tied} of {n - 1} weights tied, {int((w == 0).sum())} zero")
        assert 3 * tied >= n - 1
        assert (np.asarray(M.core_case(metric, "integer_grid", n, d, 4, 2)[1]) == 0).any()  # duplicates


def test_scaled_families_overflow_and_underflow(oracle):
    for fam in ("scaled_up", "scaled_down"):
        for metric in M.ANGULAR:  # no pair distance below Double.MAX_VALUE survives: NaN or not inserted
            assert (M.core_case(metric, fam, 1025, 5, 4, 2)[1] == M.DBL_MAX).all(), (fam, metric)
        for metric in ("manhattan", "supremum"):
            c = M.core_case(metric, fam, 1025, 5, 4, 2)[1]
            assert np.isfinite(c).all() and (c > 0).all() and (c < M.DBL_MAX).all(), (fam, metric)
    X = M.points("scaled_up", 1025, 5)
    vals = {oracle.distance(X[0], X[j], "cosine") for j in range(1, 200)}
    assert any(np.isnan(v) for v in vals) or 1.0 in vals


@pytest.mark.parametrize("metric,family", [("cosine", "rays"), ("pearson", "rays"), ("manhattan", "integer_grid"),
                                           ("supremum", "integer_grid")])
@pytest.mark.parametrize("sem", [0, 2])
def test_python_prim_equals_the_oracle(oracle, metric, family, sem):
    """edge for edge at 300 rows: parents, vertices and weight bits, self edges included"""
    n = 300
    X, core, ids, (va, vb, w) = M.prim_case(metric, family, n, 5, 4, sem)
    pa, pb, pw = M.prim_reference(n, pair_distances(X, metric), core, ids)
    assert pa == va.tolist() and pb == vb.tolist()
    assert bits_eq(np.asarray(pw), w)
    if metric in M.ANGULAR:
        assert (w[:n - 1] < 0).sum() > n // 2


def test_python_prim_on_a_nan_start_vertex(oracle):
    n = 300
    X, core, ids, (va, vb, w) = M.prim_case("cosine", "zero_row_last", n, 5, 4, 2)
    pa, pb, pw = M.prim_reference(n, pair_distances(X, "cosine"), core, ids)
    assert pa == va.tolist() and pb == vb.tolist() and bits_eq(np.asarray(pw), w)


def test_local_model_cases_mostly_return_a_model(oracle):
    """of the 16 singleton-bubble local models at least 8 return a model; every other one raises
    the reference's own "Cluster cannot have less than 0 points" """
    res = {c: M.local_model_case(*c) for c in M.BUBBLE_CASES}
    assert len(res) == 16
    models = [c for c, r in res.items() if not isinstance(r, int)]
    print(f"{len(models)} of 16 local models returned; raised: {sorted(c for c in res if c not in models)}")
    assert len(models) >= 8
    assert all(r == EREF_NEGATIVE_CLUSTER for r in res.values() if isinstance(r, int))


def test_leaf_partitions_cover_both_core_paths(oracle):
    X, ids, off, ref = M.leaf_case("cosine")
    assert np.diff(off).tolist() == M.LEAF_SIZES and len(ref) == len(M.LEAF_SIZES)
    core, (va, vb, w) = ref[-1]
    assert off[-2] > 0 and core.shape[0] == 1100 and (w[:1099] < 0).sum() > 550
    assert ref[2][1][2].shape[0] == 1  # one row: its self edge only
