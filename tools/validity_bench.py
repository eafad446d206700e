"""The DBCV validity index (csrc/validity.hip, hdb_validity_index) on device-resident input.

Shapes (any number, each one word):
  c2                 bench.py's C2 input (1M x 3 blobs, 20 centres, minPts 4) under its own flat labels
                     (minClSize 4): the fit is not timed
  gen:N:D:K:METRIC   N x D Gaussian blobs of K centres under the generating labels: a few large
                     clusters, trees through the Boruvka route
  small:N:D:K        N x D rows in K tight blobs of N / K rows each: the small-cluster Prim route
One warm-up, then RUNS whole calls inside a pair of HIP events on the context's stream: median and
range.  A further RUNS calls with kernel timing on give the spans of validity_core,
validity_mst_small, validity_sep and of the Boruvka route (boruvka_total, boruvka_gen_total).
  pair evaluations / s = executed pair evaluations / median time.  The core scan evaluates every
      (query lane, member of the lane's cluster) pair, query lanes being each cluster's members
      rounded up to whole waves of 64; the separation scan every (internal query lane, internal row)
      pair outside the tiles that lie wholly inside the wave's own cluster.
Compare with the attach scan's and K2g's rates (tools/predict_bench.py, tools/boruvka_generic_bench.py)
taken in the same session.  Prints one JSON line per shape; logs belong in profiles/validity/.
usage: python tools/validity_bench.py [--runs 5] [--splits 0] [--small-max 1024] shape [shape ...]"""
import argparse
import importlib
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
pkg = importlib.import_module("232-hierarchical-density-based-clustering-using-mapreduce_amd")

ap = argparse.ArgumentParser()
ap.add_argument("--runs", type=int, default=5)
ap.add_argument("--splits", type=int, default=0)
ap.add_argument("--small-max", type=int, default=1024)
ap.add_argument("shapes", nargs="+")
a = ap.parse_args()

ctx = pkg.Context(0)
ctx.use_torch_stream()
TIMERS = ("validity_core", "validity_mst_small", "validity_sep", "boruvka_total", "boruvka_gen_total")


def timed(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1)


def summary(ms):
    return {"median_ms": round(float(np.median(ms)), 3), "min_ms": round(min(ms), 3), "max_ms": round(max(ms), 3),
            "runs": len(ms)}


def blobs(n, d, centres, seed, spread, sigma):
    rng = np.random.default_rng(seed)
    C = rng.uniform(-spread, spread, size=(centres, d))
    lab = rng.integers(0, centres, size=n)
    return C[lab] + rng.normal(0, sigma, size=(n, d)), (lab + 1).astype(np.int32)


for shape in a.shapes:
    kind, *f = shape.split(":")
    metric = "euclidean"
    if kind == "c2":
        Xh, _ = blobs(1_000_000, 3, 20, 1, 100.0, 1.0)
        X = torch.from_numpy(Xh).cuda()
        core, g = pkg.HDBSCANStar(ctx).exactMST(X, 4, None, pkg.CORE_EXCL_SELF, selfEdges=True)
        labels, K = pkg.flat_labels(g.getVerticeA(), g.getVericeB(), g.getEges(), X.shape[0], 4, ctx=ctx)
    elif kind == "gen":
        n, d, K, metric = int(f[0]), int(f[1]), int(f[2]), f[3]
        Xh, lab = blobs(n, d, K, n + d, 30.0, 2.0)
        X, labels = torch.from_numpy(Xh).cuda(), torch.from_numpy(lab).cuda()
    else:
        n, d, K = int(f[0]), int(f[1]), int(f[2])
        rng = np.random.default_rng(7)
        lab = (rng.permutation(n) % K + 1).astype(np.int32)  # K clusters of n / K rows
        Xh = np.random.default_rng(8).uniform(-1000.0, 1000.0, size=(K, d))[lab - 1] + rng.normal(0, 1.0, size=(n, d))
        X, labels = torch.from_numpy(Xh).cuda(), torch.from_numpy(lab).cuda()
    n, d = X.shape

    def call():
        return pkg.validity_index(X, labels, metric, K, ctx=ctx, splits=a.splits, small_max=a.small_max)

    warm = timed(call)
    whole = [timed(call) for _ in range(a.runs)]
    ctx.set_timing(True)
    spans = {t: [] for t in TIMERS}
    for _ in range(a.runs):
        for t in TIMERS:
            ctx.kernel_time(t)
        v = call()
        for t in TIMERS:
            spans[t].append(ctx.kernel_time(t)[0])
    ctx.set_timing(False)
    size = v.size.cpu().numpy().astype(np.int64)
    lab_h, internal = labels.cpu().numpy(), v.internal.cpu().numpy()
    ni = np.bincount(lab_h[internal == 1], minlength=K + 1)[1:].astype(np.int64)
    lanes = lambda c: -(-c // 64) * 64
    core_pairs = int(np.sum(lanes(size[size >= 2]) * size[size >= 2]))
    sep_pairs = int(np.sum(lanes(ni) * (ni.sum() - (ni // 64) * 64)))  # own tiles skipped, up to the two edge tiles
    rate = lambda p, ms: p / (float(np.median(ms)) * 1e-3) if np.median(ms) > 0 else 0.0
    out = {"shape": shape, "n": int(n), "d": int(d), "K": int(K), "metric": metric, "index": v.index,
           "noise_share": round(float(np.mean(lab_h == 0)), 4), "largest_cluster": int(size.max()) if K else 0,
           "clusters_above_small_max": int(np.sum(size > a.small_max)), "internal_rows": int(ni.sum()),
           "splits": ctx.get_stat("validity_last_splits"), "core_splits": ctx.get_stat("validity_last_core_splits"),
           "whole_call": summary(whole), "warmup_ms": round(warm, 3),
           "timers": {t: summary(spans[t]) for t in TIMERS},
           "pair_evals": {"core": core_pairs, "sep": sep_pairs},
           "pairs_per_s": {"core": rate(core_pairs, spans["validity_core"]), "sep": rate(sep_pairs, spans["validity_sep"])}}
    print(json.dumps(out), flush=True)
