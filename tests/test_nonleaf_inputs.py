"""Host-only checks of tests/nonleaf_inputs.py: the cases reach the paths they are named for."""
import numpy as np

import nonleaf_inputs as N
from degenerate_inputs import FAMILIES, SPANNING


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


def test_model_families_have_at_least_8_bubbles(oracle):
    for name in N.NONLEAF_FAMILIES:
        assert (N.bubbles_of(name)[2] >= 8) == (name in N.MODEL_FAMILIES), name
    assert N.bubbles_of("lattice3")[2] > 1024  # K5's chunked scan: 4 chunks
