"""The k-NN paths of high dimensions -- K1m (csrc/knn_mfma.hip: single pass pruned and unpruned,
two-pass kernel, log-overflow fallback) and the FP64 scan (csrc/knn.hip knn_generic_kernel) -- on
the inputs of tests/highdim_inputs.py, where K1m's rounding-error bound is thinnest.  Everything
is compared bit for bit, on every row, with the oracle (oracle.knn_lists, oracle.core_distances
for the three semantics); tests/test_highdim_inputs.py pins the oracle and the families on the
host.  Every case asserts through launch counts which kernel produced the compared lists and
prints family, d, k, mode, the launch triple (path_helpers.k1m_launches) and the overflow count,
so the log shows which families live on the fallback.  Also: the non-finite contract of
include/hdbmi.h at d > 16 (K1m declines, the FP64 scan answers), a log compaction that makes room
without an overflow, and the shape edges n = 1 .. 513."""
import functools
import math

import numpy as np
import pytest
import torch

from highdim_inputs import (ALL_TIE, CORE_DIMS, DIMS, FAMILIES, FINITE, NONFINITE, ROWS, hd_core, hd_family, hd_lists,
                            scan_rows)
from path_helpers import bits_eq, k1m_launches, options
from test_gpu_mfma import embeddings

pytestmark = pytest.mark.gpu

JMAX = np.finfo(np.float64).max
KS = (1, 3, 15, 31)
# mode -> (options, k-means layouts of a single pass; None: the two-pass kernel alone)
MODES = {"default": (dict(), 1), "unpruned": (dict(knn_mfma_prune=0), 0), "two_pass": (dict(knn_mfma_single=0), None)}
# may decline K1m (include/hdbmi.h): a bound on max |x - mu| that is not finite
MAY_DECLINE = ("max_range", "denormal")


@pytest.fixture(scope="module")
def ctx(pkg):
    c = pkg.Context(0)  # private: no option set here can leak into another module's context
    c.use_torch_stream()
    c.set_timing(True)  # launch counts
    return c


@pytest.fixture(scope="module")
def star(pkg, ctx):
    return pkg.HDBSCANStar(ctx)


def dev(X):
    return torch.tensor(X, dtype=torch.float64, device="cuda")


def host(t):
    return t.cpu().numpy() if isinstance(t, torch.Tensor) else np.asarray(t)


def must_overflow(name, n, d, k):
    """more candidates than a log holds tie at or below every row's k-th distance (the argument of
    test_gpu_paths.test_k1m_log_overflow_falls_back_to_two_pass; the counts are asserted on the
    host in test_highdim_inputs.test_all_tie_families_exceed_a_log).  one_hot: only where k
    exceeds the at most ceil(n / d) rows at distance 0, so that the k-th distance is the sqrt 2
    all other rows share; with fewer the k-th distance is 0 and the screen rightly drops the rest."""
    return name in ALL_TIE or (name == "one_hot" and k > math.ceil(n / d))


def run_k1m(ctx, what, name, n, d, k, mode, fn):
    """fn() under the mode's options; asserts and prints the launch triple; returns fn's result"""
    kw, layouts = MODES[mode]
    k1m_launches(ctx)
    ctx.kernel_time("knn_generic", reset=True)
    with options(ctx, knn_mfma_min_n=0, **kw):
        got = fn()
    triple = k1m_launches(ctx)
    scans = ctx.kernel_time("knn_generic", reset=True)[1]
    if triple == (0, 0, 0):
        ovf = None
        assert name in MAY_DECLINE, (what, name, d, k, mode, "K1m declined")
        assert scans == 1, (what, name, d, k, mode, "no K1m kernel and no FP64 scan")
        print(f"{name} d={d} {what} k={k} {mode}: K1m declined, knn_generic x{scans}")
        return got
    assert scans == 0, (what, name, d, k, mode, "K1m and the FP64 scan both ran")
    if layouts is None:
        ovf = None
        assert triple == (1, 0, 0), (what, name, d, k, mode, triple)
    else:
        ovf = ctx.get_stat("knn_mfma_log_overflow")
        assert triple == ((2, 1, layouts) if ovf > 0 else (1, 1, layouts)), (what, name, d, k, mode, triple, ovf)
        if must_overflow(name, n, d, k):
            assert ovf > 0, (what, name, d, k, mode)
    print(f"{name} d={d} {what} k={k} {mode}: launches {triple} overflow {ovf}")
    return got


FINITE_CASES = [(name, d) for name in FINITE for d in DIMS[name]]


@pytest.mark.parametrize("name,d", FINITE_CASES, ids=lambda v: str(v))
def test_k1m_lists_equal_oracle(ctx, star, name, d):
    X, incl, excl = hd_lists(name, d)
    n = X.shape[0]
    Xd = dev(X)
    for mode in MODES:
        for k in KS:
            for ex, ref in ((False, incl), (True, excl)):
                got = run_k1m(ctx, "knn excl=%d" % ex, name, n, d, k, mode, lambda: star.knn(Xd, k, None, ex))
                assert bits_eq(host(got), ref[:, :k]), (name, d, k, ex, mode)


CORE_CASES = [(name, d) for name in FINITE for d in CORE_DIMS[name]]


@pytest.mark.parametrize("name,d", CORE_CASES, ids=lambda v: str(v))
def test_k1m_cores_equal_oracle(ctx, star, name, d):
    X = hd_family(name, d, ROWS[name])
    n = X.shape[0]
    Xd = dev(X)
    for mp in (4, 16):
        for sem in range(3):
            ref = hd_core(name, d, mp, sem)
            for mode in MODES:
                got = run_k1m(ctx, "core sem=%d" % sem, name, n, d, mp - 1, mode,
                              lambda: star.calculateCoreDistances(Xd, mp, None, sem))
                assert bits_eq(host(got), ref), (name, d, mp, sem, mode)


# ------------------------------------------------------------------------------ the FP64 scan
@pytest.mark.parametrize("d", [17, 33, 256, 257])
@pytest.mark.parametrize("name", FAMILIES)
def test_fp64_scan_equals_oracle(ctx, star, name, d):
    """knn_mfma=0, and at d = 257 the default knn_mfma=1 (with knn_mfma_min_n=0, so that K1m
    declines by the dimension and not by the row count): one knn_generic launch, no K1m kernel"""
    n = scan_rows(name, d)
    X, incl, excl = hd_lists(name, d, n)
    Xd = dev(X)
    kw = dict(knn_mfma_min_n=0) if d == 257 else dict(knn_mfma=0)
    for k in (3, 31):
        for ex, ref in ((False, incl), (True, excl)):
            k1m_launches(ctx)
            ctx.kernel_time("knn_generic", reset=True)
            with options(ctx, **kw):
                got = star.knn(Xd, k, None, ex)
            assert k1m_launches(ctx) == (0, 0, 0) and ctx.kernel_time("knn_generic", reset=True)[1] == 1
            assert bits_eq(host(got), ref[:, :k]), (name, d, k, ex)


@pytest.mark.parametrize("d", [17, 33, 256, 257])
@pytest.mark.parametrize("name", NONFINITE)
def test_nonfinite_rows_k1m_declines_and_the_scan_answers(ctx, star, name, d):
    """include/hdbmi.h: with a NaN or infinite coordinate K1m declines (no K1m kernel runs), the
    FP64 scan answers, and a pair whose distance is NaN or not below Double.MAX_VALUE enters no
    list -- lists and the three cores equal the oracle's"""
    n = scan_rows(name, d)
    X, incl, excl = hd_lists(name, d, n)
    Xd = dev(X)
    assert (excl == JMAX).any() or name in ("nan_row", "nan_rows")
    for k in KS:
        for ex, ref in ((False, incl), (True, excl)):
            k1m_launches(ctx)
            ctx.kernel_time("knn_generic", reset=True)
            with options(ctx, knn_mfma=1, knn_mfma_min_n=0):
                got = star.knn(Xd, k, None, ex)
            assert k1m_launches(ctx) == (0, 0, 0) and ctx.kernel_time("knn_generic", reset=True)[1] == 1
            assert bits_eq(host(got), ref[:, :k]), (name, d, k, ex)
    for mp in (4, 16):
        for sem in range(3):
            with options(ctx, knn_mfma=1, knn_mfma_min_n=0):
                got = star.calculateCoreDistances(Xd, mp, None, sem)
            assert k1m_launches(ctx) == (0, 0, 0) and ctx.kernel_time("knn_generic", reset=True)[1] == 1
            assert bits_eq(host(got), hd_core(name, d, mp, sem, n)), (name, d, mp, sem)


# ------------------------------------------------------------- compaction without an overflow
@pytest.mark.parametrize("k", [3, 31])   # KC 3: 256-entry half logs in registers; KC 31: the 512-entry log
@pytest.mark.parametrize("d", [24, 128])  # DP 32 and DP 128
def test_k1m_log_compaction_makes_room(ctx, star, d, k):
    """`descending` under knn_mfma_prune=0, where the screen visits the candidates in caller order
    (knn_mfma_screen_kernel: the superblocks in index order, perm the identity): every query among
    the last 128 rows logs each earlier row -- its lower bound lb <= exact < the running k-th
    smallest exact value <= thr, and there are more of them than a log or half log holds
    (test_highdim_inputs.test_descending_fills_a_log_with_droppable_entries).  No overflow
    therefore proves that log_compact made room, and the lists show it dropped nothing needed."""
    X, incl, excl = hd_lists("descending", d)
    Xd = dev(X)
    for ex, ref in ((False, incl), (True, excl)):
        got = run_k1m(ctx, "knn excl=%d" % ex, "descending", X.shape[0], d, k, "unpruned", lambda: star.knn(Xd, k, None, ex))
        assert ctx.get_stat("knn_mfma_log_overflow") == 0
        assert bits_eq(host(got), ref[:, :k]), (d, k, ex)


# ---------------------------------------------------------------------------------- shape edges
@functools.lru_cache(maxsize=None)
def edge_case(n):
    from oracle import oracle as O
    X = embeddings(n, 33, 4, 900 + n)
    X.setflags(write=False)
    return X, O.knn_lists(X, 32, excl_self=False), O.knn_lists(X, 32, excl_self=True)


@pytest.mark.parametrize("n", [1, 2, 31, 33, 511, 512, 513])
def test_k1m_shape_edges(ctx, star, n):
    """fewer than k candidates: Double.MAX_VALUE padding exactly as the oracle pads"""
    X, incl, excl = edge_case(n)
    Xd = dev(X)
    assert (excl[:, n - 1:] == JMAX).all() and (n == 1 or (excl[:, :min(n - 1, 31)] < JMAX).all())
    for mode in MODES:
        for k in (1, 31):
            for ex, ref in ((False, incl), (True, excl)):
                got = run_k1m(ctx, "knn excl=%d" % ex, "embeddings n=%d" % n, n, 33, k, mode, lambda: star.knn(Xd, k, None, ex))
                assert bits_eq(host(got), ref[:, :k]), (n, k, ex, mode)
