"""The families of tests/highdim_inputs.py are what their names say (host only), so that the GPU
tests over them (tests/test_gpu_highdim_degenerate.py) cannot pass for the wrong reason.  Every
number here is the oracle's or numpy's, never the library's: the regime each family is meant to
hit (max |x - mu| against 2^-1024, 2^-512 and 2^512; lists all 0, all non-zero subnormal squares,
all Double.MAX_VALUE), the oracle's lists against an independent numpy evaluation of the same
sequential sum (which pins the oracle whatever its build flags), and the candidate count that
makes a K1m log fill in `descending`."""
import math

import numpy as np
import pytest

from highdim_inputs import (ALL_TIE, DIMS, FAMILIES, FINITE, NONFINITE, ROWS, SCALES, SLOW, hd_family, hd_lists,
                            numpy_knn_rows, numpy_sq_rows, scan_rows, special_rows)
from path_helpers import bits_eq

JMAX = np.finfo(np.float64).max
TINY = np.finfo(np.float64).tiny  # the smallest normal number
LOG_CAP = 512  # csrc/knn_mfma.hip S_LOGCAP: log entries per query (two half logs of 256 where KC <= 15)

# every (family, d, rows) the GPU tests compare at: K1m's, and the FP64 scan's (fewer rows at 256, 257)
CASES = sorted(set([(name, d, ROWS[name]) for name in FINITE for d in DIMS[name]] +
                   [(name, d, scan_rows(name, d)) for name in FAMILIES for d in (17, 33, 256, 257)]),
               key=lambda c: (FAMILIES.index(c[0]), c[1], c[2]))


def centred_max(X):
    """max |x - mu| over all coordinates (numpy; good to a few ulps, the regimes are octaves apart)"""
    with np.errstate(over="ignore"):
        mu = X.sum(axis=0) / X.shape[0]
        return float(np.abs(X - mu).max())


def test_names_shapes_and_read_only():
    assert sorted(FAMILIES) == sorted(set(FINITE) | set(NONFINITE)) and len(set(FAMILIES)) == len(FAMILIES)
    for name in FAMILIES:
        X = hd_family(name, 33)
        assert X.shape == (1500, 33) and X.dtype == np.float64 and not X.flags.writeable
        assert hd_family(name, 33) is X
        assert np.isfinite(X).all() == (name in FINITE), name
    assert all(33 in DIMS[n] and (129 in DIMS[n] or 256 in DIMS[n]) for n in FINITE)
    assert all(d % 32 == 1 for d in DIMS["last_col"])


@pytest.mark.parametrize("d", [17, 33, 256])
def test_finite_families_are_what_they_say(d):
    n = 1500
    F = lambda name: hd_family(name, d)
    X = F("same")
    assert (X == X[0]).all() and len(set(X[0].tolist())) > 1
    assert not any(float(v).as_integer_ratio()[1] in (1, 2, 4, 8) for v in X[0, :7]), "non-dyadic values"
    X = F("two_values")
    u, c = np.unique(X, axis=0, return_counts=True)
    assert u.shape[0] == 2 and sorted(c.tolist()) == [750, 750]
    assert not F("zeros").any()
    X = F("lattice")
    assert (X[:, :3] == np.round(X[:, :3])).all() and (X[:, 3:] == X[0, 3:]).all()
    assert np.unique(X[:, :3], axis=0).shape[0] == n
    X = F("one_hot")
    assert ((X == 0) | (X == 1)).all() and (X.sum(axis=1) == 1).all()
    assert X.sum(axis=0).min() >= n // d and X.sum(axis=0).max() <= -(-n // d)
    X = F("last_col")
    assert (X[:, :d - 1] == X[0, :d - 1]).all() and np.unique(X[:, d - 1]).shape[0] > 100
    X = F("late_cols")
    assert (X[:, :d // 2] == X[0, :d // 2]).all() and (np.ptp(X[:, d // 2:], axis=0) > 0).all()
    X = F("offset9")
    assert np.abs(X - 1e9).max() <= 1.0000001e-6 and np.unique(X).shape[0] > 10
    X = F("offset15")
    assert (X == np.round(X)).all() and np.abs(X - 1e15).max() == 8
    # the regimes of the scale sc = 2^-e, 2^(e-1) <= M < 2^e, M = the bound on max |x - mu|
    for name, lo, hi in (("tiny", 0.0, 2.0 ** -512), ("subnormal_s", 0.0, 2.0 ** -512), ("below_sc2", 2.0 ** -519, 2.0 ** -512),
                         ("denormal", 0.0, 2.0 ** -1024), ("huge", 2.0 ** 512, 2.0 ** 538), ("above_sc2", 2.0 ** 512, 2.0 ** 515)):
        X = F(name)
        m = centred_max(X)
        assert lo < m and 2.0 * m < hi, (name, m)  # 2 m: the kernel bounds |x - mu| by max |x| + |mu|
        assert np.abs(X).max() <= SCALES[name] and np.abs(X).max() > 0.99 * SCALES[name]
    assert (np.abs(F("denormal")) < TINY).all()  # every coordinate is subnormal
    X = F("mixed_huge")
    big = np.abs(X).max(axis=1) > 1.0
    assert big.sum() == 10 and np.abs(X[~big]).max() <= 1.0 and np.abs(X[big]).max() > 1e199
    X = F("wide_range")
    big = np.abs(X).max(axis=1) > 1e150
    m = centred_max(X)
    # scale 2^-e with e >= 538: its square rounds to 0 (2^-1076 and below), the scale itself is normal
    assert big.sum() == 10 and 2.0 ** 537 <= m and 2.0 * m < 2.0 ** 562 and np.abs(X.sum(axis=0)).max() < 1e153
    s = numpy_sq_rows(X, np.flatnonzero(~big)[::97])
    assert np.isfinite(s[:, ~big]).all() and np.isinf(s[:, big]).all()  # finite among the small rows only
    X = F("max_range")
    assert sorted(X[:, 1][np.abs(X[:, 1]) > 1.0].tolist()) == [-1.7e308, 1.7e308]
    assert np.isfinite(X.sum(axis=0)).all() and (np.abs(np.delete(X, 1, axis=1)) <= 1.0).all()


@pytest.mark.parametrize("d", [17, 33, 257])
def test_nonfinite_rows_are_where_special_rows_says(d):
    n = 700 if d > 33 else 1500
    for name in NONFINITE:
        X = hd_family(name, d, n)
        bad = np.flatnonzero(~np.isfinite(X).all(axis=1))
        assert bad.tolist() == sorted(special_rows(name, n)), name
        assert np.isnan(X).any() == name.startswith("nan"), name
    X = hd_family("inf_rows", d, n)
    r0, r1 = special_rows("inf_rows", n)
    assert (X[r0] == np.inf).all() and X[r1, d - 1] == -np.inf and np.isfinite(X[r1, :d - 1]).all()
    X = hd_family("inf_pair", d, n)
    r0, r1 = special_rows("inf_pair", n)
    s = numpy_sq_rows(X, [r0])[0]
    assert np.isnan(s[r1]) and np.isnan(s[r0]) and np.isinf(np.delete(s, [r0, r1])).all()


@pytest.mark.parametrize("name,d,n", CASES, ids=lambda v: str(v))
def test_oracle_lists_equal_a_numpy_evaluation(name, d, n):
    """16 sampled rows, all special rows among them: the oracle's lists equal numpy's sequential
    s = s + t * t in dimension order, sqrt, k smallest values below Double.MAX_VALUE -- bit for bit"""
    X, incl, excl = hd_lists(name, d, n)
    rows = np.random.default_rng(d).choice(n, 16, replace=False)
    if name in NONFINITE:
        rows[:len(special_rows(name, n))] = special_rows(name, n)
    rows[-1] = n - 1
    rows = np.unique(rows)
    for lists, ex in ((incl, False), (excl, True)):
        assert lists.shape == (n, 31)
        assert bits_eq(lists[rows], numpy_knn_rows(X, rows, 31, ex)), (name, d, ex)
        assert not np.isnan(lists).any() and (lists <= JMAX).all() and (np.diff(lists, axis=1) >= 0).all()


def test_oracle_shorter_lists_are_prefixes(oracle):
    """what lets the GPU tests compute the oracle's lists once, at k = 31"""
    for name in ("one_hot", "subnormal_s", "inf_pair", "nan_rows", "descending"):
        X, incl, excl = hd_lists(name, 17 if name in SLOW else 33)
        for k in (1, 3, 15):
            assert bits_eq(oracle.knn_lists(X, k + 1, excl_self=False), incl[:, :k]), (name, k)
            assert bits_eq(oracle.knn_lists(X, k + 1, excl_self=True), excl[:, :k]), (name, k)


@pytest.mark.parametrize("d", [17, 33, 256])
def test_regimes_show_in_the_oracle_lists(d):
    for name in ("denormal", "tiny", "zeros", "same"):
        _, incl, excl = hd_lists(name, d) if d in DIMS[name] else hd_lists(name, 33)
        assert not incl.any() and not excl.any(), name  # every entry +0.0
    # the listed distances are square roots of non-zero subnormal squares: a few thousand units of
    # 2^-1074 in subnormal_s (coarse: rounding moves them by a per cent), 1e8 times as many in below_sc2
    for name, units in (("subnormal_s", 1e6), ("below_sc2", 1e14)):
        dd = d if d in DIMS[name] else 129
        _, incl, excl = hd_lists(name, dd)
        with np.errstate(under="ignore"):
            sq = excl * excl
        assert (excl > 0).all() and (sq < TINY).all() and (sq > 0).all() and (sq < units * 2.0 ** -1074).all(), name
        s = numpy_sq_rows(hd_family(name, dd, ROWS[name]), [0, ROWS[name] - 1])
        assert ((s < TINY) & (s >= 0)).all() and (s > 0).sum() == 2 * (ROWS[name] - 1), name
    _, incl, excl = hd_lists("huge", d) if d in DIMS["huge"] else hd_lists("huge", 33)
    assert (excl == JMAX).all() and (incl[:, 0] == 0).all() and (incl[:, 1:] == JMAX).all()


@pytest.mark.parametrize("d", [24, 33, 128, 256])
def test_descending_fills_a_log_with_droppable_entries(d):
    """every query among the last 128 rows meets, in caller order, more than LOG_CAP earlier rows
    that are each strictly closer than all rows before them (a running minimum of the exact
    distance: each one's lower bound is below the k-th smallest seen so far, so the screen logs
    it), and more than LOG_CAP / 2 of them in each half of every 32-row block's rows as the
    register-list kernel splits them (rows 8 g + 4 h + u of a block belong to half h)"""
    n = 1500
    X = hd_family("descending", d)
    rows = np.arange(n - 128, n)
    s = numpy_sq_rows(X, rows)
    half = (np.arange(n) % 8) // 4
    for qi, q in enumerate(rows):
        before = s[qi, :q]
        record = before < np.concatenate([[np.inf], np.minimum.accumulate(before)[:-1]])
        assert record.sum() > LOG_CAP, (q, record.sum())
        for h in (0, 1):
            sub = before[half[:q] == h]
            rec = sub < np.concatenate([[np.inf], np.minimum.accumulate(sub)[:-1]])
            assert rec.sum() > LOG_CAP // 2, (q, h, rec.sum())
        # and of all those only the nearest few can be among the final k = 31
        assert (before <= np.sort(s[qi])[31]).sum() <= 32


def test_all_tie_families_exceed_a_log():
    """ALL_TIE: every row has more than LOG_CAP other rows at distance 0, in either half of the
    candidate split more than LOG_CAP / 2; one_hot: every row has more than LOG_CAP rows at
    exactly sqrt 2 and at most ceil(n / d) at 0"""
    for name in ALL_TIE:
        X = hd_family(name, 33)
        s = numpy_sq_rows(X, np.arange(0, 1500, 97))
        assert ((s == 0).sum(axis=1) > LOG_CAP + 1).all(), name
    for d in (17, 33, 256):
        X = hd_family("one_hot", d)
        s = numpy_sq_rows(X, np.arange(0, 1500, 97))
        assert ((s == 2.0).sum(axis=1) > LOG_CAP).all() and ((s == 0).sum(axis=1) <= math.ceil(1500 / d)).all()
        assert ((s == 0) | (s == 2.0)).all()
