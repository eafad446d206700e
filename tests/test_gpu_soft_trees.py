"""The membership kernels of soft clustering on the device (csrc/soft.hip: sm_depth_kernel,
sm_select_kernel, sm_lift, sm_merge_birth, sm_member_kernel, over the ancestor / eps_max tables of
csrc/flat.hip sections 8 and 9) on trees the blob tree of test_gpu_soft.py never gives them: the
hand-built chains, combs, binary trees, star, forest and random recursive trees of
tests/soft_trees.py (every sizing boundary of the ancestor tables, depth differences up to 1,024,
nested selections, labels carried by several clusters or by none), more queries than one launch has
threads, K = 0, C = 0 and K = 1, a bad parent array, real trees at minClSize 2 end to end, and the
trees of tests/hierarchy_weights.py.

References, stated per test: the restatement (tests/soft_reference.py), or the host path of
csrc/soft.cpp where the Python walk over every row would take minutes -- test_soft_trees.py pins
the host path to the restatement on those very inputs.  Every comparison is on bits.  The reference
of every case is asserted NaN-free, and no row is left out of any comparison."""
import numpy as np
import pytest
import torch

import soft_trees as T
import test_soft_reference as R
from predict_ref import attach_ref, predict_ref
from soft_reference import exemplar_distances_ref, exemplars_ref, membership_ref, new_row_anchors
from test_gpu_soft import cuda, device_tree, host, same_bits, same_membership
from test_soft_trees import WEIGHT_IDS, WEIGHT_TREES, weight_tree

pytestmark = pytest.mark.gpu

INF = float("inf")


@pytest.fixture(scope="module")
def ctx(pkg):
    c = pkg.Context(0)
    c.use_torch_stream()  # stream-ordered kernels: results are read on torch's stream
    return c


def no_nan(want, where=None):
    assert not np.isnan(want[0]).any() and not np.isnan(want[1]).any(), where
    return want


def host_path(pkg, tree, anchor, level, dmin, flat=None):
    r = pkg.membership_rows(tree, anchor, level, dmin, flat)  # host arrays, no ctx: csrc/soft.cpp
    return r.vectors, r.prob, r.labels


def dev_rows(pkg, ctx, tree, anchor, level, dmin, flat=None):
    r = pkg.membership_rows(device_tree(pkg, tree), cuda(anchor, np.int32), cuda(level, np.float64),
                            cuda(dmin, np.float64), None if flat is None else cuda(flat, np.int32), ctx=ctx)
    assert all(torch.is_tensor(x) and x.is_cuda for x in (r.vectors, r.prob, r.labels))
    return r


# ------------------------------------------------------------------------- a. hand-built trees
@pytest.mark.parametrize("case", T.CASES, ids=T.CASE_IDS)
def test_hand_built_trees(pkg, ctx, case):
    """reference: case[2] -- the restatement on every row (all (anchor, cluster) pairs of the tree
    for the "all" selections), or the host path on every row (chain-1024, chain-1025, comb-600,
    binary-11)"""
    tree, flat, C, anchor, level, dmin = T.case_inputs(pkg, case)
    if case[2] == "restatement":
        want = membership_ref(tree, anchor, level, dmin, flat)
    else:
        want = host_path(pkg, tree, anchor, level, dmin, flat)
    no_nan(want, case)
    same_membership(dev_rows(pkg, ctx, tree, anchor, level, dmin, flat), want, case)
    if case[:2] == ("forest", "all"):  # pointers mix: the tree on the host, the queries on the device
        r = pkg.membership_rows(tree, cuda(anchor, np.int32), cuda(level, np.float64), cuda(dmin, np.float64), flat, ctx=ctx)
        assert r.vectors.is_cuda
        same_membership(r, want, (case, "mixed"))


def test_a_count_above_every_carried_label(pkg, ctx):
    """C = 8 with labels 1, 2, 4, 5 carried (the C ABI directly: the wrapper takes C from the largest
    label).  Reference: the restatement"""
    A = pkg._capi
    parent, birth, death, _ = T.shape("forest")
    flat = T.selection("forest", "multi")[0]
    C = 8
    anchor, level, dmin = T.queries("forest", C)
    m = anchor.shape[0]
    want = no_nan(membership_ref(T.make_tree(pkg, "forest", flat, C), anchor, level, dmin, flat, C))
    vec = torch.full((m, C), 7.0, dtype=torch.float64, device="cuda")
    prob = torch.full((m,), 7.0, dtype=torch.float64, device="cuda")
    lab = torch.full((m,), 7, dtype=torch.int32, device="cuda")
    dev = [cuda(x, dt) for x, dt in ((parent, np.int32), (birth, np.float64), (death, np.float64), (flat, np.int32),
                                    (anchor, np.int32), (level, np.float64), (dmin, np.float64))]  # kept alive
    rc = A.lib().hdb_membership_vectors(ctx.h, A.ptr(dev[0]), A.ptr(dev[1]), A.ptr(dev[2]), A.ptr(dev[3]), parent.shape[0],
                                        C, A.ptr(dev[4]), A.ptr(dev[5]), A.ptr(dev[6]), m, A.ptr(vec), A.ptr(prob),
                                        A.ptr(lab))
    torch.cuda.synchronize()
    assert rc == 0
    same_bits(host(vec), want[0], "vectors")
    same_bits(host(prob), want[1], "prob")
    assert np.array_equal(host(lab), want[2])
    assert np.all(host(vec)[:, [2, 5, 6, 7]] == 0)


# ------------------------------------------------------------------ b. the second grid-stride trip
def test_more_queries_than_one_launch_has_threads(pkg, ctx):
    """16,384 x 256 + 300 queries on the forest, C = 2: the last 300 rows belong to the second trip of
    the grid-stride loop.  References: the host path on every row; the restatement on 500 fixed
    rows, the last 300 among them"""
    m = T.GRID_CAP + 300
    flat, C, _ = T.selection("forest", "two")
    tree = T.make_tree(pkg, "forest", flat, C)
    anchor, level, dmin = T.tiled_queries("forest", C, m)
    want = no_nan(host_path(pkg, tree, anchor, level, dmin))
    r = dev_rows(pkg, ctx, tree, anchor, level, dmin)
    got = (host(r.vectors), host(r.prob), host(r.labels))
    del r
    assert np.array_equal(got[0].view(np.uint64), want[0].view(np.uint64))
    assert np.array_equal(got[1].view(np.uint64), want[1].view(np.uint64))
    assert got[2].dtype == np.int32 and np.array_equal(got[2], want[2])
    rows = np.r_[np.random.default_rng(3).integers(0, T.GRID_CAP, 200), np.arange(m - 300, m)]
    ref = no_nan(membership_ref(tree, anchor[rows], level[rows], dmin[rows]))
    same_bits(got[0][rows], ref[0], "vectors")
    same_bits(got[1][rows], ref[1], "prob")
    assert np.array_equal(got[2][rows], ref[2])
    assert (got[0][m - 300:] != 0).any() and len(set(got[2][m - 300:].tolist())) == 3


# --------------------------------------------------------------------------- c. degenerate sizes
def test_degenerate_sizes(pkg, ctx):
    """K = 0 and C = 0 with m > 0, and K = 1.  Reference: the contract's zeros, and the restatement"""
    e32, e64 = np.zeros(0, np.int32), np.zeros(0)
    m = 300
    for C in (2, 0):  # no cluster at all: every anchor is 0
        t0 = pkg.ClusterTree(e32, e64, e64, e64, e32, e32, e32, e32, e64, C)
        r = dev_rows(pkg, ctx, t0, np.zeros(m, np.int32), np.full(m, 0.5), np.full((m, C), 0.5))
        assert tuple(r.vectors.shape) == (m, C) and tuple(r.prob.shape) == (m,)
        assert np.all(host(r.vectors) == 0) and np.all(host(r.prob) == 0) and np.all(host(r.labels) == 0)
        assert not np.signbit(host(r.vectors)).any() and not np.signbit(host(r.prob)).any()
        with pytest.raises(pkg._capi.HdbError, match="anchor out of range"):
            dev_rows(pkg, ctx, t0, np.ones(m, np.int32), np.full(m, 0.5), np.full((m, C), 0.5))
    # no selected cluster: the all_inf tree is the root alone
    t = weight_tree(pkg, ("all_inf", 300), 2)
    assert t.n_tree == 1 and t.n_clusters == 0
    want = no_nan(membership_ref(t, t.point_cluster, t.point_level, np.zeros((t.n, 0))))
    r = dev_rows(pkg, ctx, t, t.point_cluster, t.point_level, np.zeros((t.n, 0)))
    assert tuple(r.vectors.shape) == (t.n, 0)
    same_membership(r, want, "C == 0")
    assert np.all(host(r.prob) == 0) and np.all(host(r.labels) == 0)
    # the root alone, selected, the only anchor
    flat, C, _ = T.selection("chain-1", "all")
    t1 = T.make_tree(pkg, "chain-1", flat, C)
    anchor, level, dmin = np.ones(4, np.int32), np.array([0.0, INF, 0.0, INF]), np.array([[0.5], [0.5], [INF], [-0.0]])
    want = no_nan(membership_ref(t1, anchor, level, dmin))
    assert np.array_equal(want[0][:, 0], [1.0, 0.0, 0.0, 0.0]) and np.array_equal(want[1], [1.0, 0.0, 1.0, 0.0])
    same_membership(dev_rows(pkg, ctx, t1, anchor, level, dmin), want, "K == 1")


# -------------------------------------------------------------------------------- d. validation
@pytest.mark.parametrize("pos,value", [(3, 5), (0, 1), (6, -2)])
def test_a_bad_parent_is_refused_before_any_write(pkg, ctx, pos, value):
    A = pkg._capi
    tree, flat, C, anchor, level, dmin = T.case_inputs(pkg, ("binary-4", "all", "restatement"))
    parent = np.array(tree.parent)
    parent[pos] = value
    m = anchor.shape[0]
    vec = torch.full((m, C), 7.0, dtype=torch.float64, device="cuda")
    prob = torch.full((m,), 7.0, dtype=torch.float64, device="cuda")
    lab = torch.full((m,), 7, dtype=torch.int32, device="cuda")
    dev = [cuda(x, dt) for x, dt in ((parent, np.int32), (tree.birth, np.float64), (tree.death, np.float64),
                                    (flat, np.int32), (anchor, np.int32), (level, np.float64), (dmin, np.float64))]
    rc = A.lib().hdb_membership_vectors(ctx.h, A.ptr(dev[0]), A.ptr(dev[1]), A.ptr(dev[2]), A.ptr(dev[3]), tree.n_tree, C,
                                        A.ptr(dev[4]), A.ptr(dev[5]), A.ptr(dev[6]), m, A.ptr(vec), A.ptr(prob), A.ptr(lab))
    torch.cuda.synchronize()
    assert rc == -1 and "parent label out of range" in A.lib().hdb_last_error().decode()
    assert bool((vec == 7.0).all()) and bool((prob == 7.0).all()) and bool((lab == 7).all())
    tree.parent = parent
    with pytest.raises(A.HdbError, match="parent label out of range") as e:
        dev_rows(pkg, ctx, tree, anchor, level, dmin, flat)
    assert e.value.code == -1


# ------------------------------------------------------------------- e. real trees end to end
DEEP = (600, 3, 150, 4, 2)  # the data of test_gpu_soft.py at minClSize 2: K = 418, C = 209, depth 40
REAL = R.CASES + [DEEP]


def constrained(pkg, t, case):
    """test_soft_reference.constrained_selection under the first seed whose cannot-link pairs change
    the selection (at minClSize 2 most seeds leave it as it is)"""
    for seed in (case[0], 1, 2, 3):
        flat = R.constrained_selection(pkg, t, seed)
        if not np.array_equal(flat, t.flat_label):
            return flat
    raise AssertionError("no seed changes the selection")


@pytest.mark.parametrize("case", REAL, ids=lambda c: "-".join(str(x) for x in c))
def test_real_trees_end_to_end(pkg, ctx, case):
    """reference: the restatement (exemplars_ref, exemplar_distances_ref over oracle distances,
    membership_ref) on every training row, under the tree's own selection and a constrained one"""
    X, t = R.fitted(pkg, case)
    if case == DEEP:
        assert t.n_tree == 418 and t.n_clusters == 209
    dt, dX = device_tree(pkg, t), cuda(X, np.float64)
    for name, flat in (("own", None), ("constrained", constrained(pkg, t, case))):
        ids, off = exemplars_ref(t, flat)
        dflat = None if flat is None else cuda(flat, np.int32)
        ex = pkg.exemplars(dt, dflat)
        assert ex[0].is_cuda and np.array_equal(host(ex[0]), ids) and np.array_equal(host(ex[1]), off), name
        dmin = exemplar_distances_ref(X, ids, off, X)
        want = no_nan(membership_ref(t, t.point_cluster, t.point_level, dmin, flat), (case, name))
        r = pkg.membership_vectors(dt, dX, flat_label=dflat, ctx=ctx)
        assert all(torch.is_tensor(x) and x.is_cuda for x in (r.vectors, r.prob, r.labels, r.dist))
        same_bits(host(r.dist), dmin, (case, name, "dist"))
        same_membership(r, want, (case, name))
        # every exemplar carries its segment's flat label
        seg = np.repeat(np.arange(1, off.shape[0]), np.diff(off))
        assert ids.shape[0] > 0 and np.array_equal(host(r.labels)[ids], seg), name


def test_new_rows_on_the_deep_tree(pkg, ctx, oracle):
    """257 new rows (test_gpu_soft.test_new_rows_end_to_end's) on the K = 418 tree, Euclidean, the
    constrained selection passed through approximate_predict.  Reference: the restatement"""
    X, t = R.fitted(pkg, DEEP)
    flat = constrained(pkg, t, DEEP)
    n, d, m = X.shape[0], X.shape[1], 257
    rng = np.random.default_rng(11)
    Q = X[rng.integers(0, n, m)].copy()
    Q[100:180] += rng.normal(0, 3.0, (80, d))
    Q[180:250] = rng.uniform(-1e4, 1e4, (70, d))
    Q[250] = float("nan")
    Q[251] = 0.0
    core = np.ascontiguousarray(oracle.core_distances(X, DEEP[3]), np.float64)
    _, nearest, level = attach_ref(X, core, Q, DEEP[3], "euclidean")
    anchor, lv = new_row_anchors(t, nearest, level, predict_ref(t, nearest, level)[0])
    ids, off = exemplars_ref(t, flat)
    dmin = exemplar_distances_ref(X, ids, off, Q)
    want = no_nan(membership_ref(t, anchor, lv, dmin, flat))
    assert nearest[250] == -1 and len(set(anchor.tolist())) > 50
    r = pkg.membership_vectors(device_tree(pkg, t), cuda(X, np.float64), cuda(Q, np.float64), cuda(core, np.float64),
                               DEEP[3], "euclidean", flat_label=cuda(flat, np.int32), ctx=ctx)
    assert tuple(r.vectors.shape) == (m, off.shape[0] - 1)
    same_bits(host(r.dist), dmin, "dist")
    same_membership(r, want, "new rows")
    assert np.all(host(r.vectors)[250] == 0) and host(r.prob)[250] == 0 and host(r.labels)[250] == 0


# ------------------------------------------------------------------------- f. the weight families
ROWS_F = 400
PALETTE_P = [.05, .2, .2, .2, .2, .15]


def training_rows(t):
    """400 random training rows under their own anchors (point_cluster, point_level) with rows of
    palette distances.  No other anchor or level: inf / inf is reachable on these trees"""
    rng = np.random.default_rng(1)
    rows = rng.integers(0, t.n, ROWS_F)
    dmin = rng.choice(np.array(T.PALETTE), (ROWS_F, t.n_clusters), p=PALETTE_P)
    return t.point_cluster[rows], t.point_level[rows], dmin


@pytest.mark.parametrize("case,mcs", WEIGHT_TREES, ids=WEIGHT_IDS)
def test_weight_family_trees(pkg, ctx, case, mcs):
    """reference: the restatement on all 400 rows; the caterpillar (K = 4,319, C = 1,880, depth 333):
    the restatement on the first 48 rows and the host path on all 400"""
    t = weight_tree(pkg, case, mcs)
    anchor, level, dmin = training_rows(t)
    r = dev_rows(pkg, ctx, t, anchor, level, dmin)
    k = 48 if case[0] == "caterpillar" else ROWS_F
    want = no_nan(membership_ref(t, anchor[:k], level[:k], dmin[:k]), (case, mcs))
    assert np.isfinite(want[0]).all() and np.isfinite(want[1]).all()
    same_bits(host(r.vectors)[:k], want[0], (case, mcs, "vectors"))
    same_bits(host(r.prob)[:k], want[1], (case, mcs, "prob"))
    assert np.array_equal(host(r.labels)[:k], want[2]), (case, mcs)
    if case[0] == "caterpillar":
        assert t.n_tree == 4319 and t.n_clusters == 1880
        same_membership(r, no_nan(host_path(pkg, t, anchor, level, dmin), case), (case, "host path"))
    if case == ("tiny_normal", 1500):
        assert t.n_tree == 769 and t.n_clusters == 270
