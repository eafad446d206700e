"""Host-only checks of tests/nonleaf_inputs.py: the cases reach the paths they are named for."""
import numpy as np
import pytest

import nonleaf_inputs as N
from degenerate_inputs import FAMILIES, SPANNING

DBL_MAX = np.finfo(np.float64).max


def test_min_normal_is_not_a_leaf_family():
    assert "min_normal" not in FAMILIES and "min_normal" not in SPANNING
    X = N.nl_family("min_normal", N.N_BIG)
    t = X[:64, None, :] - X[None, :64, :]
    s = (t * t).sum(-1)[np.triu_indices(64, 1)]
    tiny = np.finfo(np.float64).tiny
    assert (s < tiny).any() and (s > tiny).any()  # squared distances on both sides of DBL_MIN


def test_sample_variants(oracle):
    for name in N.SPECIAL:
        X = N.nl_family(name, N.N_BIG)
        sp = N.special_rows(X)
        fin, forced = N.sample_ids(name, N.N_BIG, "finite"), N.sample_ids(name, N.N_BIG, "forced")
        assert fin.shape[0] >= 1024 and not np.isin(fin, sp).any()
        assert forced[0] == sp[0] and np.isin(sp, forced).all() and forced[forced.shape[0] // 2] in sp
        assert N.k3g_runs(X, X[fin]) == 1
    for name in N.DUPLICATED:
        ids = N.sample_ids(name, N.N_BIG, "dup")
        m = ids.shape[0] // 2
        assert np.array_equal(np.sort(ids[:m]), np.sort(ids[m:])) and not np.array_equal(ids[:m], ids[m:])


def test_keyed_metric_shapes_cover_the_sizes():
    kinds = {k: {(n, m) for kind, n, m in N.KM_SHAPES.values() if kind == k} for k in ("one", "seven", "zero", "rays")}
    assert {n for _, n, _ in N.KM_SHAPES.values()} == {1, 255, 257, 1500}
    assert {m for _, _, m in N.KM_SHAPES.values()} == {1, 64, 300}
    assert all(kinds.values())
    assert [N.km_scan("euclidean", d) for d in N.KM_DIMS] == ["nearest_sq"] * 3 + ["nearest_generic", "nearest_sq"] + \
        ["nearest_generic"] * 2
    assert all(N.km_scan(mt, d) == "nearest_generic" for mt in N.METRICS for d in N.KM_DIMS)
    assert all(N.k3g_runs(np.zeros((n, 8)), np.zeros((m, 8))) == 0 for _, n, m in N.KM_SHAPES.values())


@pytest.mark.parametrize("d", N.KM_DIMS)
@pytest.mark.parametrize("metric", N.ALL_METRICS)
@pytest.mark.parametrize("name", list(N.KM_SHAPES))
def test_keyed_metric_cases_hold_what_they_are_there_for(oracle, name, metric, d):
    kind, n, m = N.KM_SHAPES[name]
    X, S, xk, sk, idx, dist, t = N.keyed_metric_case(name, metric, d)
    assert X.shape == (n, d) and S.shape == (m, d) and xk.shape == (n,) and sk.shape == (m,)
    angular = metric in ("cosine", "pearson")
    # the oracle left exactly the rows without a sample, or with NaN distances only, at index 0 and MAX
    assert t["no_candidate"] == t["no_sample"] + t["all_nan"]
    assert (idx[dist == DBL_MAX] == 0).all() and not np.isnan(dist).any()
    if metric == "pearson" and d == 1:          # a one-column row has no variance: every distance is NaN
        assert t["no_candidate"] == n and t["nan_pairs"] == sum(int((sk == k).sum()) for k in xk)
        return
    if not angular:
        assert t["nan_pairs"] == 0 and t["all_nan"] == 0
    if kind == "one":
        assert len(set(xk.tolist()) | set(sk.tolist())) == 1
        assert t["no_sample"] == 0 and t["unkeyed_differs"] == 0
        return
    assert set(xk.tolist()) == set(N.KM_KEYS) and np.any(np.diff(xk) < 0) and np.any(np.diff(sk) < 0)
    assert t["no_sample"] == int((xk == N.KM_NO_SAMPLE).sum()) > 0 and not (sk == N.KM_NO_SAMPLE).any()
    assert int((sk == N.KM_ONE_SAMPLE).sum()) == 1
    one = xk == N.KM_ONE_SAMPLE
    assert (idx[one & (dist < DBL_MAX)] == m // 2).all()
    for first, later in t["slots"]["dup"]:      # repeated inside key 5: only the first copy is ever chosen
        assert first < later and np.array_equal(S[first], S[later]) and sk[first] == sk[later] == N.KM_DUP
        assert not (idx == later).any()
    c, e = t["slots"]["copy"]                   # the same row under key 2, earlier in the list
    assert e < c and np.array_equal(S[e], S[c]) and (sk[c], sk[e]) == (N.KM_DUP, N.KM_COPY)
    assert not (idx[(xk != N.KM_COPY) & (dist < DBL_MAX)] == e).any()
    p = t["slots"]["on_copy"]
    assert xk[p] == N.KM_DUP and np.array_equal(X[p], S[c])
    # a scan without the key filter answers differently on most rows; on some only because a foreign
    # sample at the SAME distance comes first in the list (the copy, at the least, where the point on
    # it has a distance to it at all)
    assert t["unkeyed_differs"] > n // 4 and t["foreign_nearer"] > 0
    if not (angular and kind == "zero" and t["all_nan"] and np.isnan(oracle.distance(X[p], X[p], metric))):
        assert t["foreign_first"] >= 1
    if kind == "zero" and angular and d > 1:
        zs = t["slots"]["zero_samples"]
        assert t["nan_pairs"] > 0 and not np.isin(idx[dist < DBL_MAX], zs).any()  # NaN: never selected
        if metric == "cosine":
            assert t["all_nan"] == int(((xk != N.KM_NO_SAMPLE) & ~X.any(axis=1)).sum()) == 2
    if (d == 1 and metric == "cosine") or (d == 2 and metric == "pearson"):
        v = dist[dist < DBL_MAX]                # a correlation of +-1 up to rounding: 0 or 2, a few ulps off at most
        assert (np.minimum(np.abs(v), np.abs(v - 2.0)) < 1e-15).all() and t["distinct"] <= 8 and t["tied"] > n // 4
    if kind == "rays" and metric == "cosine" and d > 1:
        has = dist < DBL_MAX                    # scaled copies: distances a few ulps either side of 0
        assert (np.abs(dist[has]) < 1e-14).sum() > n // 2 and (dist[has] < 0).any() and (dist[has] > 0).any()
    if d <= 2 and not angular and kind != "rays":
        assert t["tied"] > 0                    # values rounded to 0.1


def test_model_families_have_at_least_8_bubbles(oracle):
    for name in N.NONLEAF_FAMILIES:
        assert (N.bubbles_of(name)[2] >= 8) == (name in N.MODEL_FAMILIES), name
    assert N.bubbles_of("lattice3")[2] > 1024  # K5's chunked scan: 4 chunks
