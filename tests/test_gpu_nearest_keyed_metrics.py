"""Keyed nearest sample (D3) under every metric, at the kernel: the call the driver makes at every
level (hdb_nearest_sample with keys and the run's metric) against the oracle's keyed first minimum,
on the inputs of nonleaf_inputs.keyed_metric_case -- one key; seven unsorted keys with a key that
has no sample, a key with one sample, a sample repeated inside a key and the same sample under a
foreign key earlier in the list; zero rows (NaN distances under cosine and Pearson); Pearson at
d = 1 (every distance NaN) and d = 2 (all ties); scaled copies (cosine values either side of 0).

The existing nearest-sample tests have keys with the Euclidean metric, or a metric without keys,
never both: the key filter of nearest_generic_kernel, the stable key sorts, the row gather and the
two permutations of nearest_merge_kernel are compared here, bit for bit, for the first time.
Index and distance must equal the oracle's; the launch counts say which of K3g, the fast scan
(nearest_sq) and the generic scan ran, with the nearest_grouped option on and off."""
import numpy as np
import pytest

import nonleaf_inputs as N
from path_helpers import bits_eq, options

pytestmark = pytest.mark.gpu

SCANS = ("nearest_grouped", "nearest_sq", "nearest_generic")


@pytest.fixture(scope="module")
def ctx(pkg):
    c = pkg.Context(0)  # private: launch counts and options of this module only
    c.use_torch_stream()
    c.set_timing(True)
    return c


def launches(ctx):
    return {k: ctx.kernel_time(k, reset=True)[1] for k in SCANS}


@pytest.mark.parametrize("d", N.KM_DIMS)
@pytest.mark.parametrize("metric", N.ALL_METRICS)
@pytest.mark.parametrize("name", list(N.KM_SHAPES))
def test_keyed_nearest_under_every_metric(pkg, ctx, name, metric, d):
    X, S, xk, sk, r_idx, r_dist, traits = N.keyed_metric_case(name, metric, d)
    want = dict.fromkeys(SCANS, 0)
    want[N.km_scan(metric, d)] = 1  # n <= 1500: below K3g's thresholds whatever the option says
    for grouped in (1, 0):
        launches(ctx)
        with options(ctx, nearest_grouped=grouped):
            idx, dist = pkg.nearest_sample(X, S, metric, xk, sk, ctx=ctx, with_dist=True)
        ran = launches(ctx)
        bad = np.flatnonzero((idx != r_idx) | ~((dist == r_dist) | (np.isnan(dist) & np.isnan(r_dist))))
        print(f"{name} {metric} d={d} grouped={grouped}: launches {ran}, differing rows {bad.shape[0]}, "
              f"{ {k: v for k, v in traits.items() if k != 'slots'} }")
        assert ran == want, (name, metric, d, grouped)
        assert np.array_equal(idx, r_idx), (bad[:5], idx[bad[:5]], r_idx[bad[:5]], dist[bad[:5]], r_dist[bad[:5]])
        assert bits_eq(dist, r_dist), (bad[:5], dist[bad[:5]], r_dist[bad[:5]])


@pytest.mark.parametrize("metric", N.ALL_METRICS)
def test_keyed_index_only(pkg, ctx, metric):
    """the driver's form of the call: no distance output (out_d NULL in nearest_merge_kernel)"""
    X, S, xk, sk, r_idx, _, _ = N.keyed_metric_case("zero-1500x300", metric, 7)
    assert np.array_equal(pkg.nearest_sample(X, S, metric, xk, sk, ctx=ctx), r_idx)
