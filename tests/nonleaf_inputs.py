"""Inputs and CPU references for the recursive-sampling half (nearest sample K3/K3g, bubble
statistics K4, bubble k-NN K5, the bubble Prims, the local model) on the degenerate families of
tests/degenerate_inputs.py: the families at 8,230 rows (32 x 256 + 38: a ragged last workgroup,
and n >= 8192 with 1,176 samples X[::7] is K3g's shape), one new family min_normal whose squared
distances straddle DBL_MIN, sample sets without and with the special (non-finite or huge) rows,
duplicated samples, keyed calls, and the bubbles the oracle's own nearest-sample result makes of
them.  Plain numpy and the CPU oracle, no device; every reference is computed once per process
and handed out read-only."""
import functools

import numpy as np

from degenerate_inputs import FAMILIES, family

N_BIG = 8230
STEP = 7
MIN_NORMAL = ["min_normal"]                  # a list of its own: SPANNING / FAMILIES stay as they are
NONLEAF_FAMILIES = FAMILIES + MIN_NORMAL
SPECIAL = ["inf_rows", "inf_pair", "nan_row", "nan_rows", "mixed_huge", "max_range"]
DUPLICATED = ["lattice3", "constcol", "min_normal"]
# (family, sample variant) of the Euclidean nearest-sample cases
NEAREST_CASES = [(f, "base") for f in NONLEAF_FAMILIES] + [(f, v) for f in SPECIAL for v in ("finite", "forced")] + \
                [(f, "dup") for f in DUPLICATED]
KEYED = ["constcol", "tiny", "inf_rows", "nan_rows"]   # one finite, one underflowing, one +inf, one NaN
METRIC_FAMILIES = ["same", "constcol", "tiny", "huge", "inf_rows", "nan_rows"]
METRICS = ["cosine", "pearson", "manhattan", "supremum"]
GLOBAL_BOX_M = 16448                          # 514 groups of 32 (d = 8), 257 of 64 (d = 16): 65,792 B of boxes
COOP_BUBBLES = ["lattice3", "same", "tiny", "huge", "inf_rows"]
K3G_DIMS = (2, 3, 4, 8, 16)


def ro(*arrays):
    for a in arrays:
        a.setflags(write=False)
    return arrays[0] if len(arrays) == 1 else arrays


@functools.lru_cache(maxsize=None)
def nl_family(name, n=None):
    """family(name, n) of degenerate_inputs, plus min_normal"""
    if name != "min_normal":
        return family(name, n)[0]
    X = np.random.default_rng(2000).uniform(-1.0, 1.0, size=(n or 2000, 3)) * 1.5e-154
    return ro(np.ascontiguousarray(X))  # squared distances around 2.2e-308 = DBL_MIN, some subnormal


def special_rows(X):
    """rows that are non-finite or huge (their squared distance to a unit row overflows)"""
    with np.errstate(invalid="ignore"):
        return np.flatnonzero(~(np.abs(X) < 1e100).all(axis=1))


@functools.lru_cache(maxsize=None)
def sample_ids(name, n, variant):
    """row numbers of the sample list: base X[::7]; finite: the special rows removed; forced: the
    special rows removed, then put back at list position 0 (the first) and in the middle (the
    others); dup: every sample twice, the copies at unrelated list positions"""
    X = nl_family(name, n)
    ids = np.arange(0, X.shape[0], STEP)
    if variant == "base":
        return ro(ids)
    if variant == "dup":
        return ro(np.concatenate([ids, ids[np.random.default_rng(7).permutation(ids.shape[0])]]))
    sp = special_rows(X)
    assert sp.shape[0] >= 1, name
    keep = ids[~np.isin(ids, sp)]
    if variant == "finite":
        return ro(keep)
    assert variant == "forced"
    h = keep.shape[0] // 2
    return ro(np.concatenate([sp[:1], keep[:h], sp[1:] if sp.shape[0] > 1 else sp[:1], keep[h:]]))


@functools.lru_cache(maxsize=None)
def nearest_case(name, variant, n=N_BIG):
    """(X, S, oracle index, oracle distance); n = None: the family's native size"""
    from oracle import oracle as O
    X = nl_family(name, n)
    S = np.ascontiguousarray(X[sample_ids(name, n, variant)])
    idx, dist = O.nearest_sample(X, S)
    return ro(X, S, idx, dist)


def k3g_runs(X, S, grouped=1):
    """nearest.hip nearest_grouped(): the shapes and inputs K3g takes"""
    return int(bool(grouped) and X.shape[1] in K3G_DIMS and X.shape[0] >= 8192 and S.shape[0] >= 1024
               and bool(np.isfinite(S).all()))


@functools.lru_cache(maxsize=None)
def keyed_case(name):
    """keys 0..5 of uneven sizes; key 0 has no sample, key 1 has 20 (a single group), the samples
    of key 2 are all one row.  (X, S, x_key, s_key, oracle index, oracle distance)"""
    from oracle import oracle as O
    X = nl_family(name, N_BIG)
    rng = np.random.default_rng(300 + NONLEAF_FAMILIES.index(name))
    xk = rng.choice(6, X.shape[0], p=[0.05, 0.1, 0.15, 0.2, 0.2, 0.3]).astype(np.int32)
    ids = sample_ids(name, N_BIG, "base")
    S, sk = np.array(X[ids]), xk[ids].copy()
    sk[sk == 0] = 5
    sk[np.flatnonzero(sk == 1)[20:]] = 4
    two = np.flatnonzero(sk == 2)
    S[two] = S[two[0]]
    assert (sk == 1).sum() == 20 and two.shape[0] > 64 and np.isfinite(S[two[0]]).all()
    idx, dist = O.nearest_sample(X, S, x_key=xk, s_key=sk)
    return ro(X, S, xk, sk, idx, dist)


@functools.lru_cache(maxsize=None)
def metric_case(name, metric):
    from oracle import oracle as O
    X = nl_family(name)
    S = np.ascontiguousarray(X[::STEP])
    idx, dist = O.nearest_sample(X, S, metric)
    return ro(X, S, idx, dist)


@functools.lru_cache(maxsize=None)
def global_box_case(d):
    """8,230 points against 16,448 samples, rounded to 0.1: more group boxes than K3g keeps in LDS"""
    from oracle import oracle as O
    rng = np.random.default_rng(900 + d)
    C = rng.uniform(-30.0, 30.0, size=(7, d))
    Z = np.round(C[rng.integers(0, 7, N_BIG + GLOBAL_BOX_M)] + rng.normal(0, 1.0, size=(N_BIG + GLOBAL_BOX_M, d)), 1)
    X, S = np.ascontiguousarray(Z[:N_BIG]), np.ascontiguousarray(Z[N_BIG:])
    G = 32 if d <= 8 else 64
    assert -(-S.shape[0] // G) * 2 * d * 8 > 65536
    idx, dist = O.nearest_sample(X, S)
    return ro(X, S, idx, dist)


# ------------------------------------------------------- keyed nearest sample under every metric
ALL_METRICS = ["euclidean"] + METRICS
KM_DIMS = (1, 2, 3, 7, 8, 9, 24)          # 1, 2, 3, 8: a fast Euclidean instantiation; 7, 9, 24: none
KM_FAST_DIMS = (1, 2, 3, 4, 5, 6, 8, 16)  # nearest.hip nearest_sample_device(): fast = Euclidean and one of these
KM_KEYS = (3, 11, 5, 40, 7, 2, 19)        # unsorted; 40 has points but no sample, 7 a single sample
KM_NO_SAMPLE, KM_ONE_SAMPLE, KM_DUP, KM_COPY = 40, 7, 5, 2
# name: (key set, n, m).  one: a single key; seven: KM_KEYS interleaved, two samples of key 5 repeated
# later in the list under key 5, and one sample of key 5 copied to an EARLIER list position under key 2
# (same distance to every point, a foreign key, first in sample order: it must not win); zero: seven
# with two zero rows among the points and two among the samples; rays: seven on metric_kruskal.rays
KM_SHAPES = {
    "one-1x1": ("one", 1, 1), "one-1x300": ("one", 1, 300), "one-255x1": ("one", 255, 1),
    "one-257x64": ("one", 257, 64), "one-1500x300": ("one", 1500, 300),
    "seven-255x64": ("seven", 255, 64), "seven-257x300": ("seven", 257, 300), "seven-1500x64": ("seven", 1500, 64),
    "seven-1500x300": ("seven", 1500, 300),
    "zero-257x64": ("zero", 257, 64), "zero-1500x300": ("zero", 1500, 300),
    "rays-255x300": ("rays", 255, 300), "rays-1500x64": ("rays", 1500, 64),
}


def km_scan(metric, d):
    """the timer name of the scan nearest_sample_device() launches below K3g's thresholds"""
    return "nearest_sq" if metric == "euclidean" and d in KM_FAST_DIMS else "nearest_generic"


@functools.lru_cache(maxsize=None)
def _km_input(name, d):
    """(X, S, x_key, s_key, slots): the same rows and keys for every metric"""
    from metric_kruskal import rays
    kind, n, m = KM_SHAPES[name]
    rng = np.random.default_rng(7000 + 31 * d + 7 * n + m)
    if kind == "rays":
        Z = rays(n + m, d)
    else:  # rounded to 0.1: distances tie at small d
        C = rng.uniform(-4.0, 4.0, size=(5, d))
        Z = np.round(C[rng.integers(0, 5, n + m)] + rng.normal(0, 1.0, size=(n + m, d)), 1)
    X, S = np.ascontiguousarray(Z[:n]), np.ascontiguousarray(Z[n:])
    if kind == "one":
        return ro(X, S, np.full(n, 9, np.int32), np.full(m, 9, np.int32)) + ({},)
    keys = np.array(KM_KEYS, np.int32)
    xk = keys[rng.integers(0, 7, n)]
    xk[:7] = keys[rng.permutation(7)]                      # every key has a point
    sk = keys[[0, 1, 2, 5, 6]][rng.integers(0, 5, m)]      # 40 and 7 left out
    sk[:5] = keys[[5, 0, 6, 1, 2]]                         # key 2 first: an early slot for the copy
    sk[m // 2] = KM_ONE_SAMPLE
    slots = {}
    if kind == "zero":
        z = [int(np.flatnonzero(sk == 3)[0]), int(np.flatnonzero(sk == 19)[-1])]
        S[z] = 0.0
        X[[np.flatnonzero(xk == 11)[0], np.flatnonzero(xk == 3)[-1]]] = 0.0  # keys that have samples
        slots["zero_samples"] = z
    a = np.flatnonzero(sk == KM_DUP)
    assert a.shape[0] >= 6
    S[a[-1]], S[a[-2]] = S[a[0]], S[a[1]]                  # repeated inside the key: the first must win
    c = int(a[a.shape[0] // 2])
    e = int(np.flatnonzero(sk == KM_COPY)[0])
    assert e < c
    S[e] = S[c]                                            # the same row under a foreign key, earlier in the list
    p = int(np.flatnonzero(xk == KM_DUP)[0])
    X[p] = S[c]                                            # a point of key 5 on it
    slots.update(dup=[(int(a[0]), int(a[-1])), (int(a[1]), int(a[-2]))], copy=(c, e), on_copy=p)
    return ro(X, S, xk, sk) + (slots,)


@functools.lru_cache(maxsize=None)
def keyed_metric_case(name, metric, d):
    """(X, S, x_key, s_key, oracle index, oracle distance, traits) of the keyed call.  traits counts,
    with the oracle alone, what the input holds:
      no_sample     rows whose key has no sample
      nan_pairs     (row, sample of its key) pairs whose distance is NaN: one of the two has a NaN
                    distance to itself (zero norm under cosine, zero variance under Pearson)
      all_nan       rows whose key has samples, all of them at a NaN distance
      no_candidate  rows the oracle left at index 0 and Double.MAX_VALUE
      tied          rows whose minimum is reached by more than one sample of their key (the scan
                    over the reversed list ends at another sample)
      unkeyed_differs  rows on which the unkeyed scan picks another sample (a missing key filter shows)
      foreign_nearer   rows with a foreign sample strictly nearer than the chosen one
      foreign_first    rows with a foreign sample at the same distance, earlier in the list
      distinct      distinct distances among the rows that have a candidate"""
    from oracle import oracle as O
    X, S, xk, sk, slots = _km_input(name, d)
    n, m = X.shape[0], S.shape[0]
    idx, dist = O.nearest_sample(X, S, metric, x_key=xk, s_key=sk)
    ridx, rdist = O.nearest_sample(X, S[::-1], metric, x_key=xk, s_key=sk[::-1])
    uidx, udist = O.nearest_sample(X, S, metric)
    assert bits_same(dist, rdist)
    has = dist < O.JMAX
    bad_x = np.array([np.isnan(O.distance(r, r, metric)) for r in X])
    bad_s = np.array([np.isnan(O.distance(r, r, metric)) for r in S])
    cnt = {int(k): int((sk == k).sum()) for k in np.unique(xk)}
    cnt_bad = {int(k): int(((sk == k) & bad_s).sum()) for k in np.unique(xk)}
    own = np.array([cnt[int(k)] for k in xk])
    own_nan = np.where(bad_x, own, np.array([cnt_bad[int(k)] for k in xk]))
    foreign = sk[uidx] != xk
    traits = dict(no_sample=int((own == 0).sum()), nan_pairs=int(own_nan.sum()),
                  all_nan=int(((own > 0) & (own_nan == own)).sum()), no_candidate=int((~has).sum()),
                  tied=int((has & (m - 1 - ridx != idx)).sum()), unkeyed_differs=int((uidx != idx).sum()),
                  foreign_nearer=int((has & foreign & (udist < dist)).sum()),
                  foreign_first=int((has & foreign & (udist == dist) & (uidx < idx)).sum()),
                  distinct=int(np.unique(dist[has]).shape[0]), slots=slots)
    return ro(X, S, xk, sk, idx, dist) + (traits,)


def bits_same(a, b):
    na, nb = np.isnan(a), np.isnan(b)
    return np.array_equal(na, nb) and np.array_equal(a[~na], b[~nb])


# ------------------------------------------------------------------------------------ bubbles
def compact(near, m):
    """bubble ids 0..nb-1 of the samples some point chose, in sample order (tests/golden/make_golden.py)"""
    used = np.unique(near)
    remap = -np.ones(m, np.int32)
    remap[used] = np.arange(used.shape[0], dtype=np.int32)
    return np.ascontiguousarray(remap[near]), int(used.shape[0])


@functools.lru_cache(maxsize=None)
def bubbles_of(name):
    """(X, bubble_of, nb): the bubbles the ORACLE's nearest-sample result makes of the family"""
    X, S, idx, _ = nearest_case(name, "base")
    bo, nb = compact(idx, S.shape[0])
    return X, ro(bo), nb


def slice_cuts(n):
    a, b = n // 3, (2 * n) // 3 + 1
    return [0, a, a, b, n]  # the second slice is empty


@functools.lru_cache(maxsize=None)
def stats_case(name, variant, sliced=False):
    """oracle bubble statistics dict(ls, ss, rep, info); variant "combine" or "cf" """
    from oracle import oracle as O
    X, bo, nb = bubbles_of(name)
    r = O.bubble_stats(X, bo, nb, variant, cuts=slice_cuts(X.shape[0]) if sliced else None)
    ro(*r.values())
    return r


WRAP_SIZES = (46341, 46342, 65536, 5)  # n (n - 1) as a Java int: exact, wrapped negative, wrapped to 0, small


@functools.lru_cache(maxsize=None)
def wrap_case():
    """d = 2, four bubbles of WRAP_SIZES members, rows shuffled; (X, bubble_of, oracle combine, oracle cf)"""
    from oracle import oracle as O
    rng = np.random.default_rng(46341)
    bo = rng.permutation(np.repeat(np.arange(4, dtype=np.int32), WRAP_SIZES))
    X = np.round(rng.normal(0, 10.0, size=(bo.shape[0], 2)) + 3.0 * bo[:, None], 3)
    comb, cf = O.bubble_stats(X, bo, 4, "combine"), O.bubble_stats(X, bo, 4, "cf")
    ro(X, bo, *comb.values(), *cf.values())
    return X, bo, comb, cf


def split_info(info):
    """(nB, eB, nnB) of an info[:, (extent, nnDist, n)]"""
    return (np.ascontiguousarray(info[:, 2].astype(np.int32)), np.ascontiguousarray(info[:, 0]),
            np.ascontiguousarray(info[:, 1]))


# the families whose 8,230 rows make at least 8 bubbles: same and tiny collapse to one (every
# distance is 0: sample 0 wins), two_values to two
FEW_BUBBLES = ["same", "two_values", "tiny"]
MODEL_FAMILIES = [f for f in NONLEAF_FAMILIES if f not in FEW_BUBBLES]


@functools.lru_cache(maxsize=None)
def bubble_core_case(name, min_pts):
    from oracle import oracle as O
    st = stats_case(name, "combine")
    return ro(O.bubble_core_distances(st["rep"], *split_info(st["info"]), min_pts))


@functools.lru_cache(maxsize=None)
def bubble_prim_case(name):
    from oracle import oracle as O
    st = stats_case(name, "combine")
    _, eB, nnB = split_info(st["info"])
    return ro(*O.bubble_prim_mst(st["rep"], eB, nnB, bubble_core_case(name, 4)))


@functools.lru_cache(maxsize=None)
def coop_case(name):
    """4,100 singleton bubbles (nB = 1, extent = nnDist = 0: CombineStep's one-member bubble):
    (rep, nB, eB, nnB, oracle cores at minPts 4, oracle bubble Prim)"""
    from oracle import oracle as O
    rep = nl_family(name, 4100)
    b = rep.shape[0]
    assert b == 4100
    nB, eB, nnB = np.ones(b, np.int32), np.zeros(b), np.zeros(b)
    core = O.bubble_core_distances(rep, nB, eB, nnB, 4)
    va, vb, w = O.bubble_prim_mst(rep, eB, nnB, core)
    return ro(rep, nB, eB, nnB, core, va, vb, w)


@functools.lru_cache(maxsize=None)
def local_model_case(name):
    """the oracle's local model at minPts 4, minClSize 4, or the error code it raises"""
    from oracle import oracle as O
    st = stats_case(name, "combine")
    try:
        return O.local_model(st["rep"], st["info"], 4, 4)
    except O.OracleError as e:
        return e.code
