"""Device code that only a rare input or a runtime option reaches, each against an independent
reference: K1m's log-overflow fallback, its two-pass kernel and its unpruned single pass (FP64
scan, oracle); every K6 divide-and-conquer variant (host algorithm, Python oracle); the bubble,
cooperative-Prim and traversal options (oracle, goldens); the exact-leaf MST edge for edge
against a plain Kruskal on the leaf's total edge order; host/device pointer kinds of the
local-model and merge entry points.  Every test asserts, through a stat or a kernel launch
count, that the path it asked for is the one that ran."""
import functools

import numpy as np
import pytest
import torch

from conftest import blobs, golden
from path_helpers import MST_CASES, bits_eq, edge_set, k1m_launches, mst_case, options, spanning_tree
from test_flat_labels import lib_flat
from test_gpu_mfma import embeddings
from test_gpu_parity import split_scan_case

pytestmark = pytest.mark.gpu

EINVAL = -1  # include/hdbmi.h


@pytest.fixture(scope="module")
def ctx(pkg):
    c = pkg.Context(0)  # private: no option set here can leak into another module's context
    c.use_torch_stream()
    return c


@pytest.fixture(scope="module")
def star(pkg, ctx):
    return pkg.HDBSCANStar(ctx)


# ----------------------------------------------------------------------------------- K1m
@pytest.fixture()
def timed(ctx):
    ctx.set_timing(True)
    k1m_launches(ctx)
    try:
        yield ctx
    finally:
        ctx.set_timing(False)


@functools.lru_cache(maxsize=None)
def duplicated_rows(d, dup):
    """C4-shaped embeddings, 3072 rows, rows 1200 .. 1200 + dup - 1 identical"""
    X = embeddings(3072, d, 20, 1000 + d)
    X[1200:1200 + dup] = X[1200]
    X.setflags(write=False)
    return X


@pytest.mark.parametrize("k", [3, 31])   # KC 3: 256-entry half logs in registers; KC 31: the 512-entry log
@pytest.mark.parametrize("d", [24, 128])  # DP 32 and DP 128
def test_k1m_log_overflow_falls_back_to_two_pass(timed, star, oracle, d, k):
    """800 identical rows: each of them logs its 799 twins (lower bound <= 0 <= threshold), more
    than a log holds and nothing a compaction can drop, so the call must report the overflow and
    redo every list with the two-pass kernel on the rows re-split in caller order"""
    ctx = timed
    X = duplicated_rows(d, 800)
    with options(ctx, knn_mfma=0):
        ref = star.knn(X, k, None, exclSelf=True)
    assert k1m_launches(ctx) == (0, 0, 0)
    got = star.knn(X, k, None, exclSelf=True)
    ovf = ctx.get_stat("knn_mfma_log_overflow")
    print(f"d={d} k={k} D=800: knn_mfma_log_overflow={ovf}")
    assert ovf > 0
    assert k1m_launches(ctx) == (2, 1, 1)
    assert bits_eq(got, ref)
    for sem in range(3):
        core = star.calculateCoreDistances(X, k + 1, None, sem)
        assert ctx.get_stat("knn_mfma_log_overflow") > 0 and k1m_launches(ctx) == (2, 1, 1), sem
        assert bits_eq(core, oracle.core_distances(X, k + 1, semantics=sem)), sem


@pytest.mark.parametrize("k", [3, 31])
@pytest.mark.parametrize("d", [24, 128])
def test_k1m_hundred_duplicates_fit_the_log(timed, star, d, k):
    """100 identical rows (about 50 per half log): no overflow, no second kernel"""
    ctx = timed
    X = duplicated_rows(d, 100)
    with options(ctx, knn_mfma=0):
        ref = star.knn(X, k, None, exclSelf=True)
    got = star.knn(X, k, None, exclSelf=True)
    ovf = ctx.get_stat("knn_mfma_log_overflow")
    print(f"d={d} k={k} D=100: knn_mfma_log_overflow={ovf}")
    assert ovf == 0
    assert k1m_launches(ctx) == (1, 1, 1)
    assert bits_eq(got, ref)


K1M_MODES = {"two_pass": (dict(knn_mfma_single=0), (1, 0, 0)), "unpruned": (dict(knn_mfma_prune=0), (1, 1, 0))}


@pytest.mark.parametrize("mode", sorted(K1M_MODES))
@pytest.mark.parametrize("d", [17, 64, 100, 256])
def test_k1m_two_pass_and_unpruned_equal_fp64(timed, star, mode, d):
    ctx = timed
    kw, launches = K1M_MODES[mode]
    X = embeddings(1500, d, 12, 31 * d)
    for k in (1, 15, 31):
        for excl in (False, True):
            with options(ctx, knn_mfma=0):
                ref = star.knn(X, k, None, exclSelf=excl)
            assert k1m_launches(ctx) == (0, 0, 0)
            with options(ctx, knn_mfma_min_n=0, **kw):
                got = star.knn(X, k, None, exclSelf=excl)
            assert k1m_launches(ctx) == launches, (k, excl)
            if mode == "unpruned":  # at most every 32-candidate block for every query group
                rows = ctx.get_stat("knn_mfma_group_rows")
                assert 0 < ctx.get_stat("knn_mfma_blocks") <= (1536 // rows) * 47 and ctx.get_stat("knn_mfma_log_overflow") == 0
            assert bits_eq(got, ref), (k, excl)


@pytest.mark.parametrize("mode", sorted(K1M_MODES))
def test_k1m_two_pass_and_unpruned_offset_duplicates(timed, star, mode):
    """far from the origin, unnormalised, a block of 40 identical rows and rounded rows (ties)"""
    ctx = timed
    kw, launches = K1M_MODES[mode]
    X = embeddings(3000, 64, 10, 5, noise=1.0, normalise=False, offset=1e6)
    X[100:140] = X[99]
    X[2000:2100] = np.round(X[2000:2100], 1)
    for k in (3, 15):
        with options(ctx, knn_mfma=0):
            ref = star.knn(X, k, None, exclSelf=True)
        k1m_launches(ctx)
        with options(ctx, knn_mfma_min_n=0, **kw):
            got = star.knn(X, k, None, exclSelf=True)
        assert k1m_launches(ctx) == launches
        assert bits_eq(got, ref), k


def test_k1m_removed_option_is_rejected(pkg, ctx):
    """knn_mfma_two_pass was accepted and ignored; the two-pass kernel is selected by knn_mfma_single=0"""
    with pytest.raises(pkg.HdbError):
        ctx.set_option("knn_mfma_two_pass", 0)


# ------------------------------------------------------------------------------------ K6
def hub_tree(m, wmax, seed):
    """the random tree of test_device_random_trees_equal_host (ragged depth, star-like hubs) with
    m edges, integer weights 0..wmax (huge tie groups) or continuous ones, in merged order"""
    n = m + 1
    rng = np.random.default_rng(seed)
    hub = rng.random(n - 1) < 0.3
    par = np.where(hub, 0, (rng.random(n - 1) * np.arange(1, n)).astype(np.int64))
    va, vb = par.astype(np.int32), np.arange(1, n, dtype=np.int32)
    w = rng.random(n - 1) if wmax is None else rng.integers(0, wmax + 1, n - 1).astype(np.float64)
    perm = rng.permutation(n).astype(np.int32)
    va, vb = perm[va], perm[vb]
    d = np.argsort(-w, kind="stable")
    return va[d], vb[d], w[d]


class K6Tree:
    """a merged tree on the device plus its references (host algorithm; the Python oracle up to
    5,000 edges), computed once"""

    def __init__(self, pkg, va, vb, w):
        self.pkg, self.m, self.n = pkg, int(w.shape[0]), int(w.shape[0]) + 1
        self.host = (np.ascontiguousarray(va, np.int32), np.ascontiguousarray(vb, np.int32),
                     np.ascontiguousarray(w, np.float64))
        self.dev = tuple(torch.from_numpy(x).cuda() for x in self.host)
        self.refs = {}

    def ref(self, mcs):
        if mcs not in self.refs:
            lab, k = lib_flat(self.pkg, *self.host, self.n, mcs)
            if self.m <= 5000:
                from oracle.flat_labels import flat_labels
                olab, ok = flat_labels(self.n, *self.host, mcs)
                assert ok == k and np.array_equal(olab, lab)
            self.refs[mcs] = (lab, k)
        return self.refs[mcs]

    def check(self, ctx, what, **kw):
        """labels and cluster count under the options kw equal the references, and the call ran
        the global / dc_mid depth counts that the options ask for (flat.hip, "2. Kruskal tree")"""
        J = self.m.bit_length()  # 2^J > m
        blk, mid = kw.get("flat_block_log", 10), kw.get("flat_mid_log", 12)
        LB = blk if 8 <= blk <= 10 else 8
        LM = max(LB, min(mid, J)) if mid > LB else LB
        for mcs in (2, 5):
            lab, k = self.ref(mcs)
            with options(ctx, **kw):
                got, kg = self.pkg.flat_labels(*self.dev, self.n, mcs, ctx=ctx)
                depths = ctx.get_stat("flat_global_depths"), ctx.get_stat("flat_mid_depths")
            assert depths == (max(0, J - LM), LM - LB), (what, kw, depths)
            assert kg == k and np.array_equal(got.cpu().numpy(), lab), (what, mcs, kw)
        return max(0, J - LM)


K6_INPUTS = {"hub4095": (4095, 3), "hub4096": (4096, 3), "hub4097": (4097, 3), "hub16384": (16384, 3),
             "hub16385": (16385, 3), "hub40000": (40000, 3), "cont40000": (40000, None), "hub5000": (5000, 3)}


@pytest.fixture(scope="module")
def k6_trees(pkg, ctx, star):
    cache = {}

    def get(name):
        if name not in cache:
            if name == "mst30000":  # a real tree: the exact MST of rounded blobs (weight ties)
                X = torch.from_numpy(np.round(blobs(30000, 3, 12, 5), 1)).cuda()
                _, g = star.exactMST(X, 4, None, 2, selfEdges=False)
                va, vb, w = pkg.sort_edges_desc(g.getVerticeA(), g.getVericeB(), g.getEges(), ctx)
                cache[name] = K6Tree(pkg, va.cpu().numpy(), vb.cpu().numpy(), w.cpu().numpy())
            else:
                m, wmax = K6_INPUTS[name]
                cache[name] = K6Tree(pkg, *hub_tree(m, wmax, m + (wmax or 0)))
        return cache[name]
    return get


K6_NAMES = ["hub4095", "hub4096", "hub4097", "hub16384", "hub16385", "hub40000", "cont40000", "mst30000"]


# A tied hub is a multi-way node with thousands of children, which one thread sorts by smallest id
# (fo_paths_init; a heapsort beyond 16 children since these trees showed the insertion sort taking
# 0.2-0.8 s per call).  The fine parametrisation keeps every case at a few device calls.
@pytest.mark.parametrize("mid", [0, 11, 12, 14, 24])
@pytest.mark.parametrize("relabel", [0, 1])
@pytest.mark.parametrize("name", K6_NAMES)
def test_k6_mid_and_block_matrix(ctx, k6_trees, name, relabel, mid):
    """rank-block boundaries of 2^LB and 2^LM, a partial last block, huge tie groups: all global
    depths (flat_mid_log 0), dc_mid over some depths, over all of them (24 clamps to J), with
    the sequential dc_local (flat_block_log 0) and dc_block<8..10> below"""
    t = k6_trees(name)
    for blk in (0, 8, 9, 10):
        t.check(ctx, name, flat_mid_log=mid, flat_block_log=blk, flat_relabel=relabel)


# every depth global as well (flat_mid_log 0) where the default split leaves at most one global depth
K6_ROOT_LINK = [(n, 12) for n in K6_NAMES] + [(n, 0) for n in K6_NAMES if "40000" not in n]


@pytest.mark.parametrize("root", range(6))
@pytest.mark.parametrize("name,mid", K6_ROOT_LINK)
def test_k6_root_and_link_variants(ctx, k6_trees, name, mid, root):
    """dc_root<256, 512> / <1024, 4096>, dc_root_direct, the three dc_root_multi shapes x dc_link /
    dc_link_multi on the global depths, with the default dc_mid and block settings"""
    t = k6_trees(name)
    for link in range(2):
        g = t.check(ctx, name, flat_mid_log=mid, flat_root_variant=root, flat_link_variant=link)
    assert g == max(0, t.m.bit_length() - (12 if mid else 10))


@pytest.mark.parametrize("root", range(6))
@pytest.mark.parametrize("name", ["hub16385", "hub40000", "cont40000", "mst30000"])
def test_k6_deep_variants(ctx, k6_trees, name, root):
    """global depths >= 2 take flat_deep_root / flat_deep_link instead (the others keep the defaults)"""
    t = k6_trees(name)
    for link in range(2):
        g = t.check(ctx, name, flat_deep_depth=2, flat_deep_root=root, flat_deep_link=link)
    assert g >= 3  # a deep depth ran


@pytest.mark.parametrize("mid", [9, 11])
def test_k6_oracle_leg_global_mid_and_block_depths(ctx, k6_trees, mid):
    """5,000 edges (what the Python oracle handles): global depths, dc_mid depths and dc_block<8>
    all run (2^13 > 5000: 13 - mid global depths, mid - 8 in dc_mid)"""
    t = k6_trees("hub5000")
    for relabel in (0, 1):
        for root, link in ((3, 1), (0, 0), (2, 0), (5, 1)):
            g = t.check(ctx, "hub5000", flat_mid_log=mid, flat_block_log=8, flat_relabel=relabel,
                        flat_root_variant=root, flat_link_variant=link)
            assert g == 13 - mid


def test_k6_option_ranges(pkg, ctx):
    for name, bad in (("flat_block_log", 7), ("flat_block_log", 11), ("flat_block_log", -1), ("flat_root_variant", 6),
                      ("flat_root_variant", -1), ("flat_link_variant", 2), ("flat_deep_root", 6),
                      ("flat_deep_link", 2), ("flat_deep_depth", -1), ("flat_mid_log", 25)):
        with pytest.raises(pkg.HdbError):
            ctx.set_option(name, bad)


# a child of its own: HDB_OPTS is read when a context is created, and this process has its contexts
# already.  ctypes only (no torch import): a 5,000-edge tree in host arrays, K6 on the device
# against the host algorithm, then two rejected settings.  One line per case on stdout.
HDB_OPTS_CHILD = r"""
import ctypes as C, os, sys
import numpy as np
L = C.CDLL(sys.argv[1])
L.hdb_last_error.restype = C.c_char_p
vp, i64 = C.c_void_p, C.c_int64
L.hdb_flat_labels.argtypes = [vp, vp, vp, vp, i64, i64, C.c_int32, vp, vp]
L.hdb_ctx_get_stat.argtypes = [vp, C.c_char_p, vp]
L.hdb_ctx_destroy.argtypes = [vp]
L.hdb_ctx_destroy.restype = None
h = vp()
rc = L.hdb_ctx_create(0, C.byref(h))
assert rc == 0, (rc, L.hdb_last_error())
m = 5000
va = (np.arange(1, m + 1) // 2).astype(np.int32)  # vertex i hangs below i // 2
vb = np.arange(1, m + 1, dtype=np.int32)
w = np.arange(m, 0, -1).astype(np.float64)       # merged order: descending
out = []
for ctx in (h, None):
    lab, k = np.zeros(m + 1, np.int32), i64()
    rc = L.hdb_flat_labels(ctx, va.ctypes.data, vb.ctypes.data, w.ctypes.data, m, m + 1, 5, lab.ctypes.data, C.byref(k))
    assert rc == 0, (rc, L.hdb_last_error())
    out.append((k.value, lab))
assert out[0][0] == out[1][0] and np.array_equal(out[0][1], out[1][1])
st = {}
for name in (b"flat_global_depths", b"flat_mid_depths"):
    v = i64()
    assert L.hdb_ctx_get_stat(h, name, C.byref(v)) == 0
    st[name] = v.value
print("depths", st[b"flat_global_depths"], st[b"flat_mid_depths"])
L.hdb_ctx_destroy(h)
for bad in sys.argv[2:]:
    os.environ["HDB_OPTS"] = bad
    h = vp()
    print("rejected", L.hdb_ctx_create(0, C.byref(h)), h.value, L.hdb_last_error().decode())
"""


def test_hdb_opts_environment_goes_through_set_option(pkg):
    """HDB_OPTS applies its pairs with hdb_ctx_set_option when a context is created: block log 9
    reaches K6 (2^13 > 5000 edges, mid log 12: 1 global depth and 12 - 9 = 3 dc_mid depths; the
    default block log 10 gives 2), and a value outside the option's range, an unknown name, a
    pair without a value or a value beyond 64 bits (for an option with no range of its own)
    fails the creation with HDB_EINVAL and no context"""
    import os
    import subprocess
    import sys
    bad_opts = ("flat_block_log=7", "no_such=1", "flat_block_log", "knn_tree_min_n=99999999999999999999")
    env = dict(os.environ, HDB_OPTS="flat_block_log=9")
    r = subprocess.run([sys.executable, "-c", HDB_OPTS_CHILD, pkg._capi.LIB_PATH, *bad_opts], capture_output=True,
                       text=True, timeout=60, env=env)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    lines = r.stdout.splitlines()
    assert lines[0] == "depths 1 3", lines
    assert len(lines) == 1 + len(bad_opts)
    for line, bad in zip(lines[1:], bad_opts):
        assert line.startswith(f"rejected {EINVAL} None HDB_OPTS: ") and bad in line, line


# ------------------------------------------------------------- bubble statistics and cores
@pytest.mark.parametrize("name", ["iris", "skin_bubbles2k", "blobs2k"])
def test_bubble_stats_one_lane_per_bubble_golden(pkg, ctx, name):
    g = golden(name)
    with options(ctx, bubble_fold_dim=0):
        ls, ss, rep, info = pkg.bubble_stats(g["X"], g["b_bubble_of"], g["b_used"].shape[0], ctx=ctx)
    assert bits_eq(ls, g["b_ls"]) and bits_eq(ss, g["b_ss"]) and bits_eq(rep, g["b_rep"]) and bits_eq(info, g["b_info"])


def test_bubble_stats_one_lane_per_bubble_empty_and_d1(pkg, ctx, oracle):
    X = np.random.default_rng(1).normal(size=(1000, 1))
    bo = np.random.default_rng(2).integers(0, 300, 1000).astype(np.int32)
    bo[bo == 7] = 8  # bubble 7 empty
    with options(ctx, bubble_fold_dim=0):
        ls, ss, rep, info = pkg.bubble_stats(X, bo, 300, ctx=ctx)
    r = oracle.bubble_stats(X, bo, 300)
    assert bits_eq(ls, r["ls"]) and bits_eq(ss, r["ss"]) and bits_eq(rep, r["rep"]) and bits_eq(info, r["info"])


@pytest.mark.parametrize("case", ["ties", "descending"])
def test_bubble_core_unsplit_scan_vs_oracle(pkg, ctx, oracle, case):
    """bubble_knn_split 0: one thread per bubble scans every candidate (no chunks, no replay)"""
    X, nB, eB, nnB = split_scan_case(case)
    model = pkg.HdbscanDataBubbles(ctx)
    before = ctx.get_stat("bubble_knn_replay_overflows")
    for k in (4, 8):
        with options(ctx, bubble_knn_split=0):
            core = model.calculateCoreDistancesBubbles(X, nB, eB, nnB, k)
        assert bits_eq(core, oracle.bubble_core_distances(X, nB, eB, nnB, k)), (case, k)
    assert ctx.get_stat("bubble_knn_replay_overflows") == before  # no chunked scan ran


@pytest.mark.parametrize("d", [3, 8])
def test_nearest_plain_scan_at_the_grouped_shape_vs_oracle(pkg, timed, oracle, d):
    """nearest_grouped 0 at a shape K3g takes by default (n >= 8192 points, m >= 1024 samples,
    rounded coordinates: ties between samples): the plain scan keeps the first minimum in
    sample order"""
    ctx = timed
    X = np.round(blobs(20000, d, 7, 40 + d), 1)
    S = X[::13].copy()
    r_idx, r_dist = oracle.nearest_sample(X, S)
    for grouped in (1, 0):
        ctx.kernel_time("nearest_grouped")
        with options(ctx, nearest_grouped=grouped):
            idx, dist = pkg.nearest_sample(X, S, ctx=ctx, with_dist=True)
        assert ctx.kernel_time("nearest_grouped")[1] == grouped
        assert np.array_equal(idx, r_idx) and bits_eq(dist, r_dist), grouped


# ------------------------------------------------------------------- cooperative Prim
@functools.lru_cache(maxsize=None)
def prim_case(oracle, n, kind):
    """d = 3 points or d = 8 bubbles (n > 4096: the cooperative Prim's range) and the oracle's tree"""
    rng = np.random.default_rng(n)
    ids = np.arange(n, dtype=np.int32) * 3 + 1
    if kind == "points":
        X = blobs(n, 3, 9, n + 3, spread=20.0)
        core = oracle.core_distances(X, 4, semantics=0)
        return X, ids, core, None, oracle.prim_mst(X, core, ids)
    X = blobs(n, 8, 9, n + 8, spread=20.0)
    eB, nnB = np.abs(rng.normal(0.3, 0.1, n)), np.abs(rng.normal(0.2, 0.05, n))
    nB = rng.integers(1, 9, n).astype(np.int32)
    core = oracle.bubble_core_distances(X, nB, eB, nnB, 4)
    return X, ids, core, (nB, eB, nnB), oracle.bubble_prim_mst(X, eB, nnB, core, ids)


@pytest.mark.parametrize("kind", ["points", "bubbles"])
@pytest.mark.parametrize("n", [4097, 9000])
def test_prim_coop_workgroup_size_xcd_and_launch_kind(pkg, ctx, star, oracle, n, kind):
    """prim_coop_bs x prim_coop_xcd x prim_coop_plain: the reference Prim's edges in its order
    under every combination, and the launch that ran is the one asked for -- the workgroup
    size (0: the smallest of 128..1024 that keeps the Prim within 32 workgroups, launch_coop4),
    the XCD spread factor of the plain attempt (8 when the workgroups fit one XCD), one
    cooperative-Prim launch per call.  More than 64 workgroups (9000 rows at 128) are outside
    the kernel's exchange layout: launch_coop4_bs declines and the counter-barrier kernel runs."""
    X, ids, core, bub, (va, vb, w) = prim_case(oracle, n, kind)
    model = pkg.HdbscanDataBubbles(ctx)
    for bs in (0, 128, 256, 512, 1024):
        want_bs = bs or next((b for b in (128, 256, 512) if -(-n // b) <= 32), 1024)
        nwg = -(-n // want_bs)
        for xcd in (0, 1):
            for plain in (0, 1):
                s0 = {k: ctx.get_stat(k) for k in ("prim_coop_launches", "prim_coop_plain_retries")}
                with options(ctx, prim_coop_bs=bs, prim_coop_xcd=xcd, prim_coop_plain=plain):
                    if bub is None:
                        g = star.constructMST(X, core, True, None, ids)
                    else:
                        g = model.constructMSTBubbles(X, bub[0], bub[1], bub[2], ids, core, True)
                what = (n, kind, bs, xcd, plain)
                assert bits_eq(g.getVerticeA(), va) and bits_eq(g.getVericeB(), vb) and bits_eq(g.getEges(), w), what
                retried = ctx.get_stat("prim_coop_plain_retries") - s0["prim_coop_plain_retries"]
                assert ctx.get_stat("prim_coop_launches") - s0["prim_coop_launches"] == (1 if nwg <= 64 else 0), what
                if not plain:
                    assert retried == 0, what
                if nwg <= 64:
                    assert ctx.get_stat("prim_coop_last_bs") == want_bs, what
                    spread = 8 if (plain and xcd and nwg <= 32 and not retried) else 1
                    assert ctx.get_stat("prim_coop_last_spread") == spread, what
    print(f"n={n} {kind}: prim_coop_bs=0 ran {next((b for b in (128, 256, 512) if -(-n // b) <= 32), 1024)} threads per workgroup")


def test_prim_coop_slots_accepts_only_4_and_0(pkg, ctx, star, oracle):
    """every other prim_coop_slots value is HDB_EINVAL and leaves the option at 4: the next call
    runs the register kernel (the counter-barrier kernel of slots 0 does not count a launch)"""
    for v in (-1, 1, 2, 3, 5, 6, 7):
        with pytest.raises(pkg.HdbError) as ei:
            ctx.set_option("prim_coop_slots", v)
        assert ei.value.code == EINVAL, v
    X, ids, core, _, (va, vb, w) = prim_case(oracle, 4097, "points")
    before = ctx.get_stat("prim_coop_launches")
    g = star.constructMST(X, core, True, None, ids)
    assert ctx.get_stat("prim_coop_launches") == before + 1
    assert bits_eq(g.getVerticeA(), va) and bits_eq(g.getVericeB(), vb) and bits_eq(g.getEges(), w)


def test_prim_coop_rows_wider_than_the_register_kernel(pkg, timed, oracle):
    """d = 17 has no prim_coop4_kernel instantiation (rows of d <= 16 in registers), n = 4097 is the
    smallest cooperative size: under the default options points and bubbles take the
    counter-barrier kernel, one launch each and no stepwise launches, and give the reference
    Prim's edges in its order"""
    ctx, n, d = timed, 4097, 17
    rng = np.random.default_rng(n + d)
    X = blobs(n, d, 9, n + d, spread=20.0)
    ids = np.arange(n, dtype=np.int32) * 3 + 1
    eB, nnB = np.abs(rng.normal(0.3, 0.1, n)), np.abs(rng.normal(0.2, 0.05, n))
    nB = rng.integers(1, 9, n).astype(np.int32)
    core = oracle.core_distances(X, 4, semantics=0)
    bcore = oracle.bubble_core_distances(X, nB, eB, nnB, 4)
    runs = (("points", lambda: pkg.HDBSCANStar(ctx).constructMST(X, core, True, None, ids),
             oracle.prim_mst(X, core, ids)),
            ("bubbles", lambda: pkg.HdbscanDataBubbles(ctx).constructMSTBubbles(X, nB, eB, nnB, ids, bcore, True),
             oracle.bubble_prim_mst(X, eB, nnB, bcore, ids)))
    for kind, run, (va, vb, w) in runs:
        before = ctx.get_stat("prim_coop_launches")
        for k in ("prim_coop", "prim_step_total"):
            ctx.kernel_time(k)
        g = run()
        assert bits_eq(g.getVerticeA(), va) and bits_eq(g.getVericeB(), vb) and bits_eq(g.getEges(), w), kind
        assert ctx.get_stat("prim_coop_launches") == before, kind
        assert (ctx.kernel_time("prim_coop")[1], ctx.kernel_time("prim_step_total")[1]) == (1, 0), kind


# ------------------------------------------------------------ popped-node re-tests (K1t, K2b)
@pytest.mark.parametrize("pop", [1, 2, 3])
@pytest.mark.parametrize("d", [2, 3, 8])
def test_trav_pop_test_k1t_cores_vs_oracle(ctx, star, oracle, d, pop):
    X = blobs(2500, d, 6, 7 * d + 8)
    for sem in range(3):
        with options(ctx, knn_tree=1, knn_tree_min_n=0, trav_pop_test=pop):
            got = star.calculateCoreDistances(X, 8, None, sem)  # 7-NN lists
        assert bits_eq(got, oracle.core_distances(X, 8, semantics=sem)), sem


def check_exact_mst(ctx, star, case, **kw):
    """hdb_exact_mst under the options kw: the oracle's cores, a spanning tree, and exactly the
    edges (and weight bits) of the Kruskal reference"""
    X, sem, core, (lo, hi, w) = mst_case(*case)
    n = X.shape[0]
    with options(ctx, **kw):
        c, g = star.exactMST(X, case[3], None, sem, selfEdges=False)
    assert bits_eq(c, core), (case, kw)
    va, vb, gw = g.getVerticeA(), g.getVericeB(), g.getEges()
    assert spanning_tree(va, vb, n)
    got, ref = edge_set(va, vb, gw), edge_set(lo, hi, w)
    assert got == ref, (case, kw, sorted(got - ref)[:3], sorted(ref - got)[:3])


@pytest.mark.parametrize("pop", [1, 2, 3])
def test_trav_pop_test_exact_mst_vs_kruskal(ctx, star, pop):
    check_exact_mst(ctx, star, ("blobs", 3, 6000, 4), trav_pop_test=pop)


# ------------------------------------------------- exact leaf: every edge against Kruskal
@pytest.mark.parametrize("kind,d,n,mp", MST_CASES)
def test_exact_mst_edges_equal_kruskal(ctx, star, kind, d, n, mp):
    """K2b's topology against a reference that shares no code with it: (w, s, lo, hi) is a strict
    total order, so the MST is unique and Kruskal over all pairs names every edge"""
    check_exact_mst(ctx, star, (kind, d, n, mp))


@pytest.mark.parametrize("kw", [dict(boruvka_knn_seed=0), dict(boruvka_early_rounds=0), dict(boruvka_early_rounds=2),
                                dict(boruvka_early_pts=16), dict(boruvka_early_pts=32, boruvka_early_rounds=2),
                                dict(boruvka_early_pts=16, boruvka_early_rounds=0, boruvka_knn_seed=0),
                                # the options test_exact_mst_seeding_options_equal pins against K2b itself
                                dict(leaf_seed_k=0), dict(leaf_seed_k=15, leaf_list_rounds=1), dict(leaf_list_rounds=0),
                                dict(boruvka_seed=0), dict(boruvka_adj_seed=0), dict(boruvka_wave_pts=16),
                                dict(boruvka_wave_pts=32, count_evals=1), dict(bor_xcd_chunks=0, k1t_xcd_chunks=0),
                                dict(bor_xcd_chunks=3, k1t_xcd_chunks=3)],
                         ids=lambda kw: "-".join(f"{k}{v}" for k, v in kw.items()))
def test_exact_mst_seed_and_early_round_options_vs_kruskal(ctx, star, kw):
    for case in (("blobs", 3, 3000, 4), ("blobs", 8, 3000, 9), ("skin", 3, 3000, 4)):
        check_exact_mst(ctx, star, case, **kw)


# ------------------------------------------------------- pointer kinds (C-ABI contract)
def local_model_call(A, ctx, rep, info, core, out=None):
    b, d = rep.shape
    ne = 2 * b - 1
    o = dict(lab=np.zeros(b, np.int32), mva=np.zeros(ne, np.int32), mvb=np.zeros(ne, np.int32), mw=np.zeros(ne),
             iva=np.zeros(ne, np.int32), ivb=np.zeros(ne, np.int32), iw=np.zeros(ne), nic=np.zeros(1, np.int64))
    o.update(out or {})
    rc = A.lib().hdb_local_model_cores(ctx.h, A.ptr(rep), A.ptr(info), b, d, 4, 4, 0, A.ptr(core), A.ptr(o["lab"]),
                                       A.ptr(o["mva"]), A.ptr(o["mvb"]), A.ptr(o["mw"]), A.ptr(o["iva"]),
                                       A.ptr(o["ivb"]), A.ptr(o["iw"]), A.ptr(o["nic"]))
    return rc, o


@pytest.fixture(scope="module")
def blobs2k_model(pkg, ctx, oracle):
    g = golden("blobs2k")
    rep, info = np.ascontiguousarray(g["b_rep"]), np.ascontiguousarray(g["b_info"])
    core = oracle.bubble_core_distances(rep, info[:, 2].astype(np.int32), info[:, 0].copy(), info[:, 1].copy(), 4)
    return rep, info, core, oracle.local_model(rep, info, 4, 4)


@pytest.mark.parametrize("on_device", [("core",), ("rep",), ("info",), ("core", "rep", "info")],
                         ids=lambda t: "+".join(t))
def test_local_model_cores_device_inputs(pkg, ctx, blobs2k_model, on_device):
    """hdbmi.h: an array argument may be host or device memory -- core, rep, info as device
    tensors, alone and together, give the all-host call's outputs and the oracle's, bit for bit"""
    A = pkg._capi
    rep, info, core, lm = blobs2k_model
    rc0, ref = local_model_call(A, ctx, rep, info, core)
    assert rc0 == 0
    arrs = dict(rep=rep, info=info, core=core)
    for k in on_device:
        arrs[k] = torch.from_numpy(arrs[k]).cuda()
    torch.cuda.synchronize()
    rc, got = local_model_call(A, ctx, arrs["rep"], arrs["info"], arrs["core"])
    assert rc == 0
    k = int(got["nic"][0])
    assert k == int(ref["nic"][0]) == lm["inter"][2].shape[0]
    for f in ("lab", "mva", "mvb", "iva", "ivb"):
        assert np.array_equal(got[f], ref[f]), f
    assert bits_eq(got["mw"], ref["mw"]) and bits_eq(got["iw"][:k], ref["iw"][:k])
    assert np.array_equal(got["lab"], lm["labels"])
    assert np.array_equal(got["mva"], lm["mst"][0]) and np.array_equal(got["mvb"], lm["mst"][1])
    assert bits_eq(got["mw"], lm["mst"][2])
    assert np.array_equal(got["iva"][:k], lm["inter"][0]) and np.array_equal(got["ivb"][:k], lm["inter"][1])
    assert bits_eq(got["iw"][:k], lm["inter"][2])


@pytest.mark.parametrize("which", ["lab", "mw", "iva", "nic"])
def test_local_model_device_output_is_einval(pkg, ctx, blobs2k_model, which):
    """the outputs are written by the host algorithm: a device pointer there is HDB_EINVAL with
    a message, for hdb_local_model_cores and hdb_local_model alike, and the process lives"""
    A = pkg._capi
    rep, info, core, _ = blobs2k_model
    b, d = rep.shape
    ne = 2 * b - 1
    dt = {"lab": torch.int32, "mw": torch.float64, "iva": torch.int32, "nic": torch.int64}[which]
    dev = torch.zeros(1 if which == "nic" else (b if which == "lab" else ne), dtype=dt, device="cuda")
    rc, _ = local_model_call(A, ctx, rep, info, core, {which: dev})
    assert rc == EINVAL
    with pytest.raises(pkg.HdbError, match="host memory"):
        A.check(rc, "hdb_local_model_cores")
    if which == "lab":
        rc = A.lib().hdb_local_model(ctx.h, A.ptr(rep), A.ptr(info), b, d, 4, 4, 0, A.ptr(dev), None, None, None,
                                     None, None, None, None)
        assert rc == EINVAL
    rc, _ = local_model_call(A, ctx, rep, info, core)  # and the context still works
    assert rc == 0


def test_merge_sorted_runs_device_run_offsets(pkg, ctx, oracle):
    """run_off in device memory (hdbmi.h: like every other array): the same merge"""
    A = pkg._capi
    rng = np.random.default_rng(9)
    sizes = [5000, 0, 3000, 9000, 1]
    raw, srt = [], []
    for m in sizes:
        tri = (rng.integers(0, 1 << 30, m).astype(np.int32), rng.integers(0, 1 << 30, m).astype(np.int32),
               rng.integers(0, 3, m) * 0.25)
        raw.append(tri)
        srt.append(pkg.sort_edges_desc(*(torch.from_numpy(x.copy()).cuda() for x in tri), ctx))
    off = np.r_[0, np.cumsum(sizes)].astype(np.int64)
    cat = [torch.cat([s_[i] for s_ in srt]) for i in range(3)]
    ne = int(off[-1])
    ra, rb, rw = oracle.merge_edges(raw)
    for off_arg in (off, torch.from_numpy(off).cuda()):
        oa, ob = (torch.empty(ne, dtype=torch.int32, device="cuda") for _ in range(2))
        ow = torch.empty(ne, dtype=torch.float64, device="cuda")
        torch.cuda.synchronize()
        A.check(A.lib().hdb_merge_sorted_runs(ctx.h, A.ptr(cat[0]), A.ptr(cat[1]), A.ptr(cat[2]), A.ptr(off_arg),
                                              len(sizes), A.ptr(oa), A.ptr(ob), A.ptr(ow)), "merge_sorted_runs")
        torch.cuda.synchronize()
        assert np.array_equal(oa.cpu().numpy(), ra) and np.array_equal(ob.cpu().numpy(), rb)
        assert bits_eq(ow.cpu().numpy(), rw)
    bad = torch.from_numpy(np.r_[0, 7, 3, int(off[-1])].astype(np.int64)).cuda()  # a device run_off is validated too
    assert A.lib().hdb_merge_sorted_runs(ctx.h, A.ptr(cat[0]), A.ptr(cat[1]), A.ptr(cat[2]), A.ptr(bad), 3,
                                         A.ptr(oa), A.ptr(ob), A.ptr(ow)) == EINVAL
