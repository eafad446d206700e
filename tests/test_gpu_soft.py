"""Soft clustering on the device: the exemplar-distance scan (csrc/soft.hip, hdb_exemplar_distances)
bit for bit against the restatement over oracle distances (tests/soft_reference.py) for all five
metrics, around the 8-wide dimension chunk, the 256-query workgroup, the 4-row batch and the 64-row
candidate tile, over hand-built segment layouts; the split count changes no bit; the device
membership kernel and membership_vectors end to end, for training rows and for new rows, against the
restatement; host and device pointers mix; bad input is refused before anything is written."""
import functools

import numpy as np
import pytest
import torch

from metric_inputs import points
from predict_ref import attach_ref, cross_distances, predict_ref
from soft_reference import (exemplar_distances_ref, exemplars_ref, membership_ref, min_by_segment, new_row_anchors)
from test_outlier_scores import bits
from test_predict_host import blob_tree_edges, tie_heavy

pytestmark = pytest.mark.gpu

NAN, INF = float("nan"), float("inf")
N_TRAIN = 330


@pytest.fixture(scope="module")
def ctx(pkg):
    c = pkg.Context(0)
    c.use_torch_stream()  # the scan is stream-ordered: results are read on torch's stream
    return c


def cuda(x, dt):
    return torch.from_numpy(np.array(x, dtype=dt, order="C")).cuda()


def host(x):
    return x.cpu().numpy() if torch.is_tensor(x) else np.asarray(x)


# ------------------------------------------------------------------------------ segment layouts
def _cuts(E, C, seed):
    """C + 1 ascending offsets from 0 to E with repeats (empty segments)"""
    rng = np.random.default_rng(seed)
    return np.r_[0, np.sort(rng.integers(0, E + 1, C - 1)), E].astype(np.int64)


# name -> offsets; E = offsets[-1].  A boundary inside a batch of 4 (2, 3, 5), exactly on a 64-row
# tile edge (64), segments that straddle one (60..130 over 64 and 128), empty segments at the
# start, in the middle and at the end, one segment with every row, C = 1 and C = 130
LAYOUTS = {
    "e1": [0, 1],
    "e63": [0, 2, 2, 5, 63],
    "e64_all": [0, 64],
    "e64_empty_ends": [0, 0, 64, 64],
    "e65_edge": [0, 64, 65],
    "e300": [0, 3, 3, 60, 64, 130, 130, 200, 300, 300],
    "e300_all": [0, 300],
    "e300_c130": _cuts(300, 130, 5).tolist(),
}


def layout(name):
    off = np.asarray(LAYOUTS[name], np.int64)
    E = int(off[-1])
    ids = np.random.default_rng(E).integers(0, N_TRAIN, E).astype(np.int32)  # arbitrary rows, repeats allowed
    ids[::5] = 7  # the zero / constant row of the families that have one
    return ids, off


@functools.lru_cache(maxsize=None)
def scan_rows(metric, family, d, m):
    """(X, Q, distances of every query to every training row), computed once: queries are copies of
    training rows (distance 0 or NaN), scaled copies (the same direction) and fresh rows"""
    X = np.array(points(family, N_TRAIN, d))
    d = X.shape[1]
    rng = np.random.default_rng(31 * m + d)
    Q = np.array(points(family, m + 9, d))[:m]
    pick, kind = rng.integers(0, N_TRAIN, m), rng.integers(0, 3, m)
    Q[kind == 0] = X[pick][kind == 0]
    Q[kind == 1] = (X[pick] * np.round(rng.uniform(0.5, 3.0, (m, 1)), 1))[kind == 1]
    D = cross_distances(Q, X, metric)
    for a in (X, Q, D):
        a.setflags(write=False)
    return X, Q, D


def dev_scan(pkg, ctx, X, ids, off, Q, metric, splits=0):
    out = pkg.HDBSCANStar(ctx).exemplarDistances(cuda(X, np.float64), cuda(ids, np.int32), cuda(off, np.int64),
                                                 cuda(Q, np.float64), metric, splits)
    assert torch.is_tensor(out) and out.is_cuda and tuple(out.shape) == (Q.shape[0], off.shape[0] - 1)
    return host(out)


def same_bits(got, want, where=None):
    bad = np.argwhere(bits(np.asarray(got)) != bits(np.asarray(want)))
    assert bad.shape[0] == 0, (where, bad[:5], np.asarray(got)[tuple(bad[:5].T)], np.asarray(want)[tuple(bad[:5].T)])


# every d in {1, 3, 8, 9, 17, 40}, m in {1, 255, 257, 600}, layout and metric; rays: cosine and
# Pearson values either side of 0; zero_row7 / const_row7: NaN distances; scaled_up: overflowing norm
# products; integer_grid: duplicates and exact zeros
SCAN = [
    ("euclidean", "integer_grid", 3, 257, "e300"),
    ("euclidean", "rounded_blobs", 1, 1, "e1"),
    ("euclidean", "integer_grid", 8, 255, "e63"),
    ("euclidean", "scaled_up", 9, 600, "e300_c130"),
    ("euclidean", "rounded_blobs", 17, 257, "e65_edge"),
    ("euclidean", "integer_grid", 40, 255, "e64_empty_ends"),
    ("manhattan", "integer_grid", 9, 600, "e300"),
    ("manhattan", "integer_grid", 1, 257, "e64_all"),
    ("manhattan", "scaled_up", 40, 1, "e300_all"),
    ("supremum", "integer_grid", 17, 255, "e300_c130"),
    ("supremum", "integer_grid", 3, 600, "e65_edge"),
    ("supremum", "rounded_blobs", 8, 257, "e63"),
    ("cosine", "rays", 9, 257, "e300"),
    ("cosine", "zero_row7", 3, 600, "e300_c130"),
    ("cosine", "scaled_up", 8, 255, "e65_edge"),
    ("cosine", "rays", 40, 1, "e64_empty_ends"),
    ("cosine", "integer_grid", 17, 257, "e63"),
    ("pearson", "rays", 17, 600, "e300"),
    ("pearson", "const_row7", 9, 255, "e300_c130"),
    ("pearson", "rays", 1, 257, "e64_all"),  # d = 1: no variance, every distance NaN, every entry +inf
    ("pearson", "scaled_up", 40, 257, "e1"),
    ("pearson", "rays", 3, 1, "e300_all"),
]


@pytest.mark.parametrize("case", SCAN, ids=lambda c: "-".join(str(x) for x in c))
def test_scan_equals_the_restatement(pkg, ctx, case):
    metric, family, d, m, name = case
    X, Q, D = scan_rows(metric, family, d, m)
    ids, off = layout(name)
    want = min_by_segment(D[:, ids], off)
    got = dev_scan(pkg, ctx, X, ids, off, Q, metric)
    same_bits(got, want, case)
    assert not np.isnan(got).any() and not np.signbit(got[got == 0]).any()
    assert np.all(got[:, np.diff(off) == 0] == INF)
    if case == SCAN[-3]:
        assert np.all(got == INF)
    if family in ("zero_row7", "const_row7"):
        assert np.isnan(D[:, 7]).all()  # the NaN row is among the exemplars and never wins


@pytest.mark.parametrize("case", [("euclidean", "integer_grid", 9, 257, "e300"),
                                  ("cosine", "rays", 9, 257, "e300_c130"),
                                  ("pearson", "const_row7", 9, 255, "e65_edge")],
                         ids=lambda c: "-".join(str(x) for x in c))
def test_split_count_changes_no_bit(pkg, ctx, case):
    metric, family, d, m, name = case
    X, Q, D = scan_rows(metric, family, d, m)
    ids, off = layout(name)
    want = min_by_segment(D[:, ids], off)
    for splits in (1, 2, 7, 0):
        same_bits(dev_scan(pkg, ctx, X, ids, off, Q, metric, splits), want, (case, splits))
        if splits:
            assert ctx.get_stat("soft_last_splits") == splits
        else:
            assert ctx.get_stat("soft_last_splits") >= 1


# ----------------------------------------------------------------------------------- end to end
CASE = (600, 3, 150, 4, 25)  # n, d, duplicated rows, minPts, minClSize


@functools.lru_cache(maxsize=None)
def fitted(pkg):
    """(X, the host tree, its exemplars and dmin of the training rows by the restatement)"""
    n, d, dup, min_pts, mcs = CASE
    X = tie_heavy(n, d, dup)
    t = pkg.cluster_tree(*blob_tree_edges(n, d, dup, min_pts), n, mcs)
    assert t.n_clusters >= 2
    ids, off = exemplars_ref(t)
    return X, t, ids, off, exemplar_distances_ref(X, ids, off, X)


def device_tree(pkg, t):
    dts = (np.int32, np.float64, np.float64, np.float64, np.int32, np.int32, np.int32, np.int32, np.float64)
    return pkg.ClusterTree(*[cuda(getattr(t, k), dt) for k, dt in zip(t.FIELDS, dts)], t.n_clusters)


def same_membership(r, want, where=None):
    same_bits(host(r.vectors), want[0], (where, "vectors"))
    same_bits(host(r.prob), want[1], (where, "prob"))
    lab = host(r.labels)
    assert lab.dtype == np.int32 and np.array_equal(lab, want[2]), where


def test_training_rows_end_to_end(pkg, ctx):
    X, t, ids, off, dmin = fitted(pkg)
    want = membership_ref(t, t.point_cluster, t.point_level, dmin)
    r = pkg.membership_vectors(device_tree(pkg, t), cuda(X, np.float64), ctx=ctx)
    assert all(torch.is_tensor(x) and x.is_cuda for x in (r.vectors, r.prob, r.labels, r.dist))
    same_bits(host(r.dist), dmin, "dist")
    same_membership(r, want, "device")
    # host arrays, no ctx: the scan stages through the device, the membership runs on the host
    rh = pkg.membership_vectors(t, X)
    assert all(isinstance(x, np.ndarray) for x in (rh.vectors, rh.prob, rh.labels, rh.dist))
    same_bits(rh.dist, dmin, "dist host")
    same_membership(rh, want, "host")
    ex = pkg.exemplars(device_tree(pkg, t))
    assert ex[0].is_cuda and np.array_equal(host(ex[0]), ids) and np.array_equal(host(ex[1]), off)
    # every exemplar carries its flat label and its row is zero off Z
    seg = np.repeat(np.arange(1, off.shape[0]), np.diff(off))
    assert np.array_equal(host(r.labels)[ids], seg)
    assert np.all(host(r.vectors)[ids][dmin[ids] > 0] == 0)


@pytest.mark.parametrize("metric", ["euclidean", "cosine"])
def test_new_rows_end_to_end(pkg, ctx, oracle, metric):
    X, t, ids, off, _ = fitted(pkg)
    n, d, m = X.shape[0], X.shape[1], 257
    rng = np.random.default_rng(11)
    Q = X[rng.integers(0, n, m)].copy()                       # copies of training rows
    Q[100:180] += rng.normal(0, 3.0, (80, d))                  # near rows
    Q[180:250] = rng.uniform(-1e4, 1e4, (70, d))               # far rows
    Q[250] = NAN
    Q[251] = 0.0                                               # cosine: every distance NaN, no anchor
    core = np.ascontiguousarray(oracle.core_distances(X, CASE[3], metric=metric), np.float64)
    core_q, nearest, level = attach_ref(X, core, Q, CASE[3], metric)
    tl = predict_ref(t, nearest, level)[0]
    anchor, lv = new_row_anchors(t, nearest, level, tl)
    dmin = exemplar_distances_ref(X, ids, off, Q, metric)
    want = membership_ref(t, anchor, lv, dmin)
    assert nearest[250] == -1 and (metric != "cosine" or nearest[251] == -1)
    r = pkg.membership_vectors(device_tree(pkg, t), cuda(X, np.float64), cuda(Q, np.float64), cuda(core, np.float64),
                               CASE[3], metric, ctx=ctx)
    assert r.vectors.is_cuda and tuple(r.vectors.shape) == (m, off.shape[0] - 1)
    same_bits(host(r.dist), dmin, "dist")
    same_membership(r, want, metric)
    assert np.all(host(r.vectors)[250] == 0) and host(r.prob)[250] == 0 and host(r.labels)[250] == 0
    rh = pkg.membership_vectors(t, X, Q, core, CASE[3], metric)  # host arrays
    same_membership(rh, want, (metric, "host"))


def test_device_membership_on_arbitrary_anchors(pkg, ctx):
    """the LCA by binary lifting against the plain walk: anchors anywhere in the tree, levels at
    births (M == B ties), zero, no anchor; the tree's own selection and one with an unused label"""
    X, t, ids, off, dmin = fitted(pkg)
    rng = np.random.default_rng(5)
    m = 700
    anchor = rng.integers(0, t.n_tree + 1, m).astype(np.int32)
    level = rng.choice(np.r_[t.birth[1:], 0.0, t.point_level[:5]], m)
    rows = dmin[rng.integers(0, t.n, m)]
    want = membership_ref(t, anchor, level, rows)
    same_membership(pkg.membership_rows(device_tree(pkg, t), cuda(anchor, np.int32), cuda(level, np.float64),
                                        cuda(rows, np.float64), ctx=ctx), want, "device")
    # pointers mix: the tree on the host, the queries on the device
    same_membership(pkg.membership_rows(t, cuda(anchor, np.int32), level, cuda(rows, np.float64), ctx=ctx), want, "mixed")
    flat = np.where(t.flat_label > 0, t.flat_label + 1, 0).astype(np.int32)  # label 1 carried by no cluster
    wide = np.c_[rows[:, :1] * 2 + 1, rows]
    want = membership_ref(t, anchor, level, wide, flat)
    assert np.all(want[0][:, 0] == 0)
    same_membership(pkg.membership_rows(device_tree(pkg, t), cuda(anchor, np.int32), cuda(level, np.float64),
                                        cuda(wide, np.float64), cuda(flat, np.int32), ctx=ctx), want, "shifted")


# ------------------------------------------------------------------------------------- plumbing
def test_pointers_mix_and_scratch_is_reused(pkg, ctx):
    X, Q, D = scan_rows("euclidean", "integer_grid", 9, 257)
    ids, off = layout("e300")
    want = min_by_segment(D[:, ids], off)
    H = pkg.HDBSCANStar(ctx)
    out = H.exemplarDistances(X, cuda(ids, np.int32), off, cuda(Q, np.float64), "euclidean")
    assert out.is_cuda
    same_bits(host(out), want, "mixed")
    out = H.exemplarDistances(cuda(X, np.float64), ids, cuda(off, np.int64), Q, "euclidean")
    assert isinstance(out, np.ndarray)
    same_bits(out, want, "host queries")
    # one context: a large call, a small one, the large one again
    ids1, off1 = layout("e1")
    small = min_by_segment(D[:3][:, ids1], off1)
    for _ in range(2):
        same_bits(dev_scan(pkg, ctx, X, ids, off, Q, "euclidean", 7), want, "again")
        same_bits(dev_scan(pkg, ctx, X, ids1, off1, Q[:3], "euclidean"), small, "small")


def test_bad_input_is_refused_before_any_write(pkg, ctx):
    A = pkg._capi
    X, Q, _ = scan_rows("euclidean", "integer_grid", 9, 257)
    ids, off = layout("e300")
    C, E, m = off.shape[0] - 1, ids.shape[0], Q.shape[0]
    dX, dQ = cuda(X, np.float64), cuda(Q, np.float64)

    def scan(ids_, off_, n_ids=E, on_device=True):
        out = torch.full((m, C), -7.0, dtype=torch.float64, device="cuda")
        i_, o_ = (cuda(ids_, np.int32), cuda(off_, np.int64)) if on_device else (A.Arr(ids_, np.int32).obj,
                                                                                 A.Arr(off_, np.int64).obj)
        rc = A.lib().hdb_exemplar_distances(ctx.h, A.ptr(dX), N_TRAIN, X.shape[1], A.ptr(i_), n_ids, A.ptr(o_), C,
                                            A.ptr(dQ), m, 0, A.ptr(out))
        torch.cuda.synchronize()
        return rc, host(out)

    def changed(a, pos, v):
        a = a.copy()
        a[pos] = v
        return a

    bad = [(changed(ids, 17, -1), off), (changed(ids, E - 1, N_TRAIN), off), (changed(ids, 0, 2 ** 31 - 1), off),
           (ids, changed(off, 0, 1)), (ids, changed(off, 4, 59)), (ids, changed(off, C, E + 1)),
           (ids, changed(off, C, E - 1))]
    for ids_, off_ in bad:
        for on_device in (True, False):
            rc, out = scan(ids_, off_, on_device=on_device)
            assert rc == -1 and np.all(out == -7.0)
    assert scan(ids[:-1], off, n_ids=E - 1)[0] == -1
    rc, out = scan(ids, off)
    assert rc == 0 and not np.any(out == -7.0)
    # a flat_label outside 0..C, on the device
    _, t, _, _, dmin = fitted(pkg)
    dt = device_tree(pkg, t)
    flat = t.flat_label.copy()
    flat[np.flatnonzero(flat > 0)[0]] = t.n_clusters + 1
    vec = torch.full((t.n, t.n_clusters), 7.0, dtype=torch.float64, device="cuda")
    for f in (flat, np.where(t.flat_label == 1, -1, t.flat_label)):
        rc = A.lib().hdb_membership_vectors(ctx.h, A.ptr(dt.parent), A.ptr(dt.birth), A.ptr(dt.death),
                                            A.ptr(cuda(f, np.int32)), t.n_tree, t.n_clusters, A.ptr(dt.point_cluster),
                                            A.ptr(dt.point_level), A.ptr(cuda(dmin, np.float64)), t.n, A.ptr(vec), None,
                                            None)
        torch.cuda.synchronize()
        assert rc == -1 and bool((vec == 7.0).all())
    with pytest.raises(pkg._capi.HdbError):
        pkg.membership_rows(dt, cuda(changed(t.point_cluster, 3, t.n_tree + 1), np.int32), dt.point_level,
                            cuda(dmin, np.float64), ctx=ctx)


def test_empty_calls_are_ok(pkg, ctx):
    X, Q, _ = scan_rows("euclidean", "integer_grid", 9, 257)
    ids, off = layout("e300")
    H = pkg.HDBSCANStar(ctx)
    out = H.exemplarDistances(cuda(X, np.float64), cuda(ids, np.int32), cuda(off, np.int64), cuda(Q[:0], np.float64))
    assert tuple(out.shape) == (0, off.shape[0] - 1)
    out = H.exemplarDistances(cuda(X, np.float64), cuda(ids[:0], np.int32), cuda(off[:1], np.int64), cuda(Q, np.float64))
    assert tuple(out.shape) == (Q.shape[0], 0)
    # no exemplar at all: every segment is empty
    out = H.exemplarDistances(cuda(X, np.float64), cuda(ids[:0], np.int32), cuda([0, 0, 0], np.int64), cuda(Q, np.float64))
    assert tuple(out.shape) == (Q.shape[0], 2) and bool((out == INF).all())
    _, t, _, _, dmin = fitted(pkg)
    r = pkg.membership_rows(device_tree(pkg, t), cuda(t.point_cluster[:0], np.int32), cuda(t.point_level[:0], np.float64),
                            cuda(dmin[:0], np.float64), ctx=ctx)
    assert tuple(r.vectors.shape) == (0, t.n_clusters)
