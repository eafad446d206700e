"""Cost of the cluster tree export on top of K6, and of the level-cut kernel: the C2 merged list
(1M x 3 blobs, seed 1, minPts 4, exact MST + self edges, stable descending sort), minClSize 4,
warm.  One process alternates labels-only calls (hdb_flat_labels) and tree calls
(hdb_flat_cluster_tree) and prints the device span of each and the difference; then it times
hdb_labels_at_levels for L = 1, 8 and 64 levels beside a hipMemsetAsync of the same L x n x 4
bytes on the same device and stream -- the store-bound yardstick -- and prints the ratio.
Usage: python tools/tree_bench.py [n] [reps]"""
import ctypes as C
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


def with_tree():
    return pkg.cluster_tree(va, vb, w, n, 4, ctx=ctx)


lab, k = labels_only()
tree = with_tree()
torch.cuda.synchronize()
assert k == tree.n_clusters and torch.equal(lab, tree.flat_labels())
ctx.set_timing(True)
ctx.kernel_time("flat_labels")
span = {"labels": [], "tree": []}
for _ in range(reps):
    for name, fn in (("labels", labels_only), ("tree", with_tree)):
        fn()
        torch.cuda.synchronize()
        ms, cnt = ctx.kernel_time("flat_labels")
        span[name].append(ms / max(cnt, 1))
med = {k_: statistics.median(v) for k_, v in span.items()}
for name in ("labels", "tree"):
    v = span[name]
    print(f"{'labels only ' if name == 'labels' else 'cluster tree'} n={n}: median {med[name]:.3f} ms device span "
          f"(min {min(v):.3f}, max {max(v):.3f}, {reps} calls)")
labelled = int((tree.flat_labels() > 0).sum())
print(f"the tree export adds {med['tree'] - med['labels']:.3f} ms ({100 * (med['tree'] / med['labels'] - 1):.1f} % of the "
      f"labels-only span, its host round trip for K included); K_tree={tree.n_tree}, flat clusters {k}, {labelled} points labelled")

# ---- the cut kernel beside a memset of the bytes it writes
hip = None
with open("/proc/self/maps") as fh:  # the HIP runtime this process already runs on
    for line in fh:
        if "libamdhip64" in line:
            hip = C.CDLL(line.split()[-1])
            break
assert hip is not None, "no HIP runtime mapped"
hip.hipMemsetAsync.argtypes = [C.c_void_p, C.c_int, C.c_size_t, C.c_void_p]
hip.hipMemsetAsync.restype = C.c_int
stream = torch.cuda.current_stream()
births = torch.sort(tree.birth[1:], descending=True).values
for L in (1, 8, 64):
    # levels spread over the birth levels: rows with many clusters and many noise points
    lv = births[torch.linspace(0, births.shape[0] - 1, L, device=births.device).long()].contiguous()
    rows = pkg.labels_at_levels(tree, lv, ctx=ctx)
    torch.cuda.synchronize()
    ctx.kernel_time("labels_at_levels")
    cut, fill = [], []
    for _ in range(reps):
        pkg.labels_at_levels(tree, lv, ctx=ctx)
        torch.cuda.synchronize()
        ms, cnt = ctx.kernel_time("labels_at_levels")
        cut.append(ms / max(cnt, 1))
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record(stream)
        rc = hip.hipMemsetAsync(rows.data_ptr(), 0, rows.numel() * 4, stream.cuda_stream)
        b.record(stream)
        torch.cuda.synchronize()
        assert rc == 0
        fill.append(a.elapsed_time(b))
    c, f = statistics.median(cut), statistics.median(fill)
    print(f"labels_at_levels n={n} L={L}: median {c:.3f} ms device span (tables + cut; min {min(cut):.3f}, max {max(cut):.3f}) "
          f"| hipMemsetAsync of {rows.numel() * 4 / 1e6:.1f} MB: {f:.3f} ms | ratio {c / f:.2f}")
