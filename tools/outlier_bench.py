"""Cost of the GLOSH outlier scores on top of K6: the C2 merged list (1M x 3 blobs, seed 1,
minPts 4, exact MST + self edges, stable descending sort), minClSize 4, warm.  One process
alternates labels-only calls (hdb_flat_labels) and labels + scores calls
(hdb_flat_outlier_scores) and prints the device span of each and the difference.
Usage: python tools/outlier_bench.py [n] [reps]"""
import importlib
import os
import statistics
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from bench import make_blobs  # noqa: E402

pkg = importlib.import_module("232-hierarchical-density-based-clustering-using-mapreduce_amd")
n = int(sys.argv[1]) if len(sys.argv) > 1 else 1_000_000
reps = int(sys.argv[2]) if len(sys.argv) > 2 else 10
ctx = pkg.Context.get(0)
ctx.use_torch_stream()
star = pkg.HDBSCANStar(ctx)
X = torch.from_numpy(make_blobs(n, 3, 20, 1)).cuda()
_, g = star.exactMST(X, 4, None, pkg.CORE_EXCL_SELF, True)
va, vb, w = pkg.sort_edges_desc(g.getVerticeA(), g.getVericeB(), g.getEges(), ctx)


def labels_only():
    return pkg.flat_labels(va, vb, w, n, 4, ctx=ctx)


def with_scores():
    return pkg.outlier_scores(va, vb, w, n, 4, ctx=ctx, with_labels=True)


lab, k = labels_only()
s, e, lab2, k2 = with_scores()
torch.cuda.synchronize()
assert k == k2 and torch.equal(lab, lab2)
ctx.set_timing(True)
ctx.kernel_time("flat_labels")
span = {"labels": [], "scores": []}
for _ in range(reps):
    for name, fn in (("labels", labels_only), ("scores", with_scores)):
        fn()
        torch.cuda.synchronize()
        ms, cnt = ctx.kernel_time("flat_labels")
        span[name].append(ms / max(cnt, 1))
med = {k_: statistics.median(v) for k_, v in span.items()}
for name in ("labels", "scores"):
    v = span[name]
    print(f"{'labels only    ' if name == 'labels' else 'labels + scores'} n={n}: median {med[name]:.3f} ms device span "
          f"(min {min(v):.3f}, max {max(v):.3f}, {reps} calls)")
finite = torch.isfinite(s)
print(f"outlier scores add {med['scores'] - med['labels']:.3f} ms ({100 * (med['scores'] / med['labels'] - 1):.1f} % of the "
      f"labels-only span); K={k}, clusters {ctx.get_stat('flat_clusters_total')}, "
      f"scores in [{float(s[finite].min()):.4f}, {float(s[finite].max()):.4f}], {int((s > 0.9).sum())} above 0.9")
