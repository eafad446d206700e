"""Soft clustering (csrc/soft.hip; hdb_exemplars, hdb_exemplar_distances, hdb_membership_vectors) on
device-resident input.

Shapes:
  c2            bench.py's C2 input (1M x 3 blobs, 20 centres, minPts 4) under its own cluster tree
                (minClSize 4), every training point as a query.  The m x C output is produced in
                chunks of --chunk queries, as the memory rule of include/hdbmi.h asks
  gen:n:d:m     n x d Gaussian blobs (16 centres), minPts 4, minClSize 25, m fresh draws as queries
Per shape: the fit (exactMST, cluster_tree; not timed), then one warm-up and RUNS whole calls of the
exemplar-distance scan inside a pair of HIP events on the context's stream: median and range;
a further RUNS calls with kernel timing on give the spans of soft_scan and soft_merge; the same for
hdb_membership_vectors over the scan's output and for hdb_exemplars (host work, wall clock).
  pair evaluations / s = query lanes (m rounded up to whole waves of 64) x exemplars / median time
Beside the scan, what a user would write today: FP64 torch.cdist(Q, X[ids]) followed by a segmented
amin (not bit-exact; time only), and -- with --attach -- the attach scan of the same queries against
all n rows for its pair rate in the same session.  Prints one JSON line per shape; logs belong in
profiles/soft/.
usage: python tools/soft_bench.py [--runs 5] [--splits 0] [--chunk 65536] [--attach] shape [shape ...]"""
import argparse
import importlib
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
pkg = importlib.import_module("232-hierarchical-density-based-clustering-using-mapreduce_amd")

ap = argparse.ArgumentParser()
ap.add_argument("--runs", type=int, default=5)
ap.add_argument("--splits", type=int, default=0)
ap.add_argument("--chunk", type=int, default=65536)
ap.add_argument("--attach", action="store_true")
ap.add_argument("shapes", nargs="+")
a = ap.parse_args()

ctx = pkg.Context(0)
ctx.use_torch_stream()
H = pkg.HDBSCANStar(ctx)


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


def spans(fn, names):
    ctx.set_timing(True)
    got = {t: [] for t in names}
    for _ in range(a.runs):
        for t in names:
            ctx.kernel_time(t)
        fn()
        for t in names:
            got[t].append(ctx.kernel_time(t)[0])
    ctx.set_timing(False)
    return {t: summary(v) for t, v in got.items()}


for shape in a.shapes:
    kind, *f = shape.split(":")
    if kind == "c2":
        rng = np.random.default_rng(1)
        centres = rng.uniform(-100.0, 100.0, size=(20, 3))
        X = torch.from_numpy(centres[rng.integers(0, 20, size=1_000_000)] + rng.normal(0, 1.0, size=(1_000_000, 3))).cuda()
        Q, mcs = None, 4
    else:
        n, d, m = int(f[0]), int(f[1]), int(f[2])
        rng = np.random.default_rng(n + d + m)
        centres = rng.uniform(-30.0, 30.0, size=(16, d))
        draw = lambda k: torch.from_numpy(centres[rng.integers(0, 16, k)] + rng.normal(0, 2.0, size=(k, d))).cuda()
        X, Q, mcs = draw(n), draw(m), 25
    n, d = X.shape
    core, g = H.exactMST(X, 4, None, pkg.CORE_EXCL_SELF, selfEdges=True)
    tree = pkg.cluster_tree(g.getVerticeA(), g.getVericeB(), g.getEges(), n, mcs, ctx=ctx)
    t0 = time.perf_counter()
    ids, offsets = pkg.exemplars(tree, ctx=ctx)
    ex_ms = (time.perf_counter() - t0) * 1e3
    C, E = tree.n_clusters, int(ids.shape[0])
    if Q is None:
        queries, anchor, level = X, tree.point_cluster, tree.point_level
    else:
        queries = Q
        pred = pkg.approximate_predict(tree, X, core, Q, 4, ctx=ctx)
        anchor = pred.tree_labels
        pl = tree.point_level[pred.nearest.to(torch.int64).clamp(min=0)]
        level = torch.where(pl > pred.level, pl, pred.level)
    m = int(queries.shape[0])
    chunks = [(s, min(s + a.chunk, m)) for s in range(0, m, a.chunk)]
    keep = {}

    def scan():
        for s, e in chunks:
            keep["dist"] = H.exemplarDistances(X, ids, offsets, queries[s:e], None, a.splits)

    def member():  # over the last chunk's distances
        s, e = chunks[-1]
        keep["mem"] = pkg.membership_rows(tree, anchor[s:e], level[s:e], keep["dist"], ctx=ctx)

    def yardstick():
        seg = torch.repeat_interleave(torch.arange(C, device="cuda"), offsets[1:] - offsets[:-1])
        for s, e in chunks:
            D = torch.cdist(queries[s:e], X[ids.to(torch.int64)])
            out = torch.full((e - s, C), float("inf"), dtype=torch.float64, device="cuda")
            out.scatter_reduce_(1, seg.expand(e - s, -1), D, "amin")
            keep["yard"] = out

    warm = timed(scan)
    whole = [timed(scan) for _ in range(a.runs)]
    splits = ctx.get_stat("soft_last_splits")
    lanes = sum(-(-(e - s) // 64) * 64 for s, e in chunks)
    pairs = lanes * E
    rate = lambda p, ms: p / (float(np.median(ms)) * 1e-3) if np.median(ms) > 0 else 0.0
    out = {"shape": shape, "n": int(n), "d": int(d), "m": m, "tree_clusters": tree.n_tree, "C": C, "exemplars": E,
           "chunks": len(chunks), "splits_last_chunk": splits, "exemplars_host_ms": round(ex_ms, 3),
           "scan": summary(whole), "scan_warmup_ms": round(warm, 3), "scan_timers": spans(scan, ("soft_scan", "soft_merge")),
           "pair_evals": pairs, "pairs_per_s": rate(pairs, whole)}
    timed(member)
    out["membership_last_chunk"] = dict(summary([timed(member) for _ in range(a.runs)]), rows=chunks[-1][1] - chunks[-1][0])
    if max(e - s for s, e in chunks) * E * 8 / 2 ** 30 <= 40.0:
        try:
            timed(yardstick)
            out["cdist_segmented_amin"] = summary([timed(yardstick) for _ in range(a.runs)])
            same = torch.isclose(keep["yard"], keep["dist"], rtol=1e-9, atol=1e-9) | (keep["yard"] == keep["dist"])
            out["cdist_agrees_to_1e-9"] = bool(same.all())
        except RuntimeError as err:  # out of memory in torch's temporaries
            out["cdist_segmented_amin"] = "not measured: " + str(err).splitlines()[0][:120]
    else:
        out["cdist_segmented_amin"] = "not measured: a chunk's FP64 matrix is too large"
    if a.attach and Q is not None:
        run = lambda: H.attachPoints(X, core, Q, 4)
        timed(run)
        ms = [timed(run) for _ in range(a.runs)]
        out["attach"] = dict(summary(ms), pairs_per_s=rate(2 * (-(-m // 64) * 64) * n, ms),
                             splits=ctx.get_stat("attach_last_splits"))
    print(json.dumps(out), flush=True)
