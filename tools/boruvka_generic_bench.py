"""K2g (csrc/boruvka_generic.hip) against the reference Prim, the only other MST route for its shapes.

Per shape (n d metric): one warm-up, then RUNS alternating calls of hdb_mst_boruvka (this tree's
library) and hdb_prim_mst (the library named by --prim-lib, e.g. the parent commit's build; default:
this tree's), each inside a pair of HIP events on the stream the context runs on; median and range.
A further untimed K2g call with count_evals on reads the pruning counters: candidate tiles evaluated
and skipped by each rule per round, and the executed pair evaluations.  From those:
  pair evaluations / s   = executed pair evaluations / median time (whole call, not scan alone)
  share of FP64 peak     = pair evaluations * padded d * ops per dimension / time / PEAK, with
                           PEAK = 256 CUs * 4 SIMDs * 16 FP64 lanes per clock * 2.4 GHz = 39.3e12
                           FP64 vector operations / s (no FMA on this path; a wave64 FP64
                           instruction issues over 4 cycles on a SIMD)
Cores are the library's own (hdb_core_distances, minPts 4), not timed.  Prints one JSON line per
shape.  usage: python tools/boruvka_generic_bench.py [--runs 5] [--prim-lib PATH] [--no-prim]
               [--prim-max-s 60] n d metric [n d metric ...]"""
import argparse
import ctypes as C
import importlib
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
pkg = importlib.import_module("232-hierarchical-density-based-clustering-using-mapreduce_amd")
A = importlib.import_module("232-hierarchical-density-based-clustering-using-mapreduce_amd._capi")

PEAK_FP64_VALU = 256 * 4 * 16 * 2.4e9
OPS_PER_DIM = {"euclidean": 3, "manhattan": 2, "supremum": 2, "cosine": 2, "pearson": 2}
STAT_NAMES = ("tiles_eval", "tiles_skip_comp", "tiles_skip_core", "tiles_skip_seed", "pair_evals")

ap = argparse.ArgumentParser()
ap.add_argument("--runs", type=int, default=5)
ap.add_argument("--prim-lib", default=None)
ap.add_argument("--no-prim", action="store_true")
ap.add_argument("--prim-max-s", type=float, default=60.0, help="skip the Prim's timed runs if its warm-up took longer")
ap.add_argument("shapes", nargs="+")
a = ap.parse_args()

ctx = pkg.Context.get(0)
ctx.use_torch_stream()
stream = torch.cuda.current_stream(0).cuda_stream

prim_lib, prim_ctx = A.lib(), ctx.h
if a.prim_lib:
    prim_lib = C.CDLL(os.path.abspath(a.prim_lib))
    prim_ctx = C.c_void_p()
    assert prim_lib.hdb_ctx_create(0, C.byref(prim_ctx)) == 0
    assert prim_lib.hdb_ctx_set_stream(prim_ctx, C.c_void_p(stream)) == 0
vp, i64, i32 = C.c_void_p, C.c_int64, C.c_int32
prim_lib.hdb_prim_mst.argtypes = [vp, vp, i64, i32, vp, vp, i32, i32, vp, vp, vp]


def timed(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1)


def summary(ms):
    return {"median_ms": round(float(np.median(ms)), 3), "min_ms": round(min(ms), 3), "max_ms": round(max(ms), 3),
            "runs": len(ms)} if ms else None


for n, d, metric in zip(a.shapes[0::3], a.shapes[1::3], a.shapes[2::3]):
    n, d, m = int(n), int(d), A.METRIC[metric]
    rng = np.random.default_rng(n + d)
    centres = rng.uniform(-30.0, 30.0, size=(16, d))
    X = torch.from_numpy(centres[rng.integers(0, 16, n)] + rng.normal(0, 2.0, size=(n, d))).cuda()
    core = pkg.HDBSCANStar(ctx).calculateCoreDistances(X, 4, m)
    va = torch.empty(n - 1, dtype=torch.int32, device="cuda")
    vb = torch.empty_like(va)
    w = torch.empty(n - 1, dtype=torch.float64, device="cuda")
    pa, pb, pw = torch.empty_like(va), torch.empty_like(vb), torch.empty_like(w)

    def k2g():
        A.check(A.lib().hdb_mst_boruvka(ctx.h, X.data_ptr(), n, d, core.data_ptr(), m, 0, va.data_ptr(), vb.data_ptr(),
                                        w.data_ptr()), "hdb_mst_boruvka")

    def prim():
        rc = prim_lib.hdb_prim_mst(prim_ctx, X.data_ptr(), n, d, core.data_ptr(), None, m, 0, pa.data_ptr(),
                                   pb.data_ptr(), pw.data_ptr())
        assert rc == 0, rc

    warm_k2g = timed(k2g)
    do_prim = not a.no_prim
    warm_prim = timed(prim) if do_prim else None
    same = bool(torch.equal(torch.sort(w).values.view(torch.int64), torch.sort(pw).values.view(torch.int64))) if do_prim else None
    if do_prim and warm_prim > a.prim_max_s * 1e3:
        do_prim = False
    tg, tp = [], []
    for _ in range(a.runs):
        tg.append(timed(k2g))
        if do_prim:
            tp.append(timed(prim))
    rounds = ctx.get_stat("boruvka_gen_rounds")
    ctx.set_option("count_evals", 1)
    k2g()
    ctx.set_option("count_evals", 0)
    per_round = [{k: ctx.get_stat("boruvka_gen_r%d_%s" % (r, k)) for k in STAT_NAMES} for r in range(rounds)]
    pairs = ctx.get_stat("boruvka_gen_pair_evals")
    dp = -(-d // ctx.get_stat("boruvka_gen_dc")) * ctx.get_stat("boruvka_gen_dc")
    med = float(np.median(tg)) * 1e-3
    for r in per_round:
        tot = sum(r[k] for k in STAT_NAMES[:4])
        r["share_skipped"] = {k[11:]: round(r[k] / tot, 4) for k in STAT_NAMES[1:4]} if tot else {}
    print(json.dumps({
        "n": n, "d": d, "metric": metric, "padded_d": dp, "rounds": rounds,
        "k2g": summary(tg), "k2g_warmup_ms": round(warm_k2g, 3),
        "prim": summary(tp), "prim_warmup_ms": None if warm_prim is None else round(warm_prim, 3),
        "prim_lib": a.prim_lib or "this tree", "sorted_weights_equal": same,
        "pair_evals": pairs, "pair_evals_per_s": pairs / med,
        "fp64_ops_per_s": pairs * dp * OPS_PER_DIM[metric] / med,
        "share_of_fp64_valu_peak": round(pairs * dp * OPS_PER_DIM[metric] / med / PEAK_FP64_VALU, 4),
        "per_round": per_round}), flush=True)
