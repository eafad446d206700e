"""Cost of the constraint-aware flat extraction (hdb_constrained_flat_labels) on the device: the
C2 merged list (1M x 3 blobs, seed 1, minPts 4, exact MST + self edges, stable descending sort),
minClSize 4, warm, every array device-resident.  One process alternates labels-only calls
(hdb_flat_labels), tree calls (hdb_flat_cluster_tree) and constrained calls for m = 0, 10^3 and
10^6 uniform random constraints of mixed types, and prints the device span of each.  Beside each
constrained span: the time of a device-to-device copy of the bytes the call must at least move
(12 m read, 4 n written) on the same stream -- the floor -- the ratio to it, and the spans of the
call's parts (ancestor table + depths, the constraint kernel with its lifting reads, children
lists, the single-launch climb, selection + numbering, the per-point gather).  Last, the same
call on the thousands-deep chain tree of the tests: the climb's serial worst case.
Usage: python tools/constraints_bench.py [n] [reps]"""
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
PARTS = ("cfl_tables", "cfl_constraints", "cfl_children", "cfl_climb", "cfl_select", "cfl_labels")
ctx = pkg.Context.get(0)
ctx.use_torch_stream()
star = pkg.HDBSCANStar(ctx)
X = torch.from_numpy(make_blobs(n, 3, 20, 1)).cuda()
_, g = star.exactMST(X, 4, None, pkg.CORE_EXCL_SELF, True)
va, vb, w = pkg.sort_edges_desc(g.getVerticeA(), g.getVericeB(), g.getEges(), ctx)
tree = pkg.cluster_tree(va, vb, w, n, 4, ctx=ctx)
lab, k = pkg.flat_labels(va, vb, w, n, 4, ctx=ctx)
stream = torch.cuda.current_stream()


def constraints(npts, m, seed):
    rng = np.random.default_rng(seed)
    return [torch.from_numpy(x.astype(np.int32)).cuda()
            for x in (rng.integers(0, npts, m), rng.integers(0, npts, m), rng.integers(0, 2, m))]


def med(v):
    return statistics.median(v)


def constrained_spans(t, c, reps):
    """median device span of the call and of each part; the floor copy beside it"""
    npts, m = t.n, int(c[0].shape[0])
    src = torch.empty(max(3 * m + npts, 1), dtype=torch.int32, device="cuda")
    dst = torch.empty_like(src)
    pkg.constrained_flat_labels(t, *c, ctx=ctx)
    torch.cuda.synchronize()
    for name in PARTS + ("constrained_flat_labels",):
        ctx.kernel_time(name)
    total, parts, floor = [], {p: [] for p in PARTS}, []
    for _ in range(reps):
        pkg.constrained_flat_labels(t, *c, ctx=ctx)
        torch.cuda.synchronize()
        ms, cnt = ctx.kernel_time("constrained_flat_labels")
        total.append(ms / max(cnt, 1))
        for p in PARTS:
            parts[p].append(ctx.kernel_time(p)[0])
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record(stream)
        dst.copy_(src)
        b.record(stream)
        torch.cuda.synchronize()
        floor.append(a.elapsed_time(b))
    return total, {p: med(v) for p, v in parts.items()}, med(floor)


r0 = pkg.constrained_flat_labels(tree, *constraints(n, 0, 0), ctx=ctx)
torch.cuda.synchronize()
assert k == tree.n_clusters == r0.n_clusters and torch.equal(r0.labels, lab) and torch.equal(r0.flat_label, tree.flat_label)
ctx.set_timing(True)
ctx.kernel_time("flat_labels")
span = {"labels": [], "tree": []}
for _ in range(reps):
    for name, fn in (("labels", lambda: pkg.flat_labels(va, vb, w, n, 4, ctx=ctx)),
                     ("tree", lambda: pkg.cluster_tree(va, vb, w, n, 4, ctx=ctx))):
        fn()
        torch.cuda.synchronize()
        ms, cnt = ctx.kernel_time("flat_labels")
        span[name].append(ms / max(cnt, 1))
for name in ("labels", "tree"):
    v = span[name]
    print(f"{'labels only ' if name == 'labels' else 'cluster tree'} n={n}: median {med(v):.3f} ms device span "
          f"(min {min(v):.3f}, max {max(v):.3f}, {reps} calls); K_tree={tree.n_tree}")
for m in (0, 1000, 1_000_000):
    c = constraints(n, m, m + 1)
    total, parts, floor = constrained_spans(tree, c, reps)
    r = pkg.constrained_flat_labels(tree, *c, ctx=ctx)
    print(f"constrained n={n} m={m}: median {med(total):.3f} ms device span (min {min(total):.3f}, max {max(total):.3f}) | "
          f"copy of {(12 * m + 4 * n) / 1e6:.1f} MB: {floor:.3f} ms | ratio {med(total) / floor:.1f} | "
          f"flat clusters {r.n_clusters} (unconstrained {k}), satisfied {r.satisfied_fraction:.4f}")
    print("    parts (ms): " + ", ".join(f"{p[4:]} {v:.3f}" for p, v in parts.items()))

# the chain tree of the tests: 3,001 pairs chained by ascending bridges, one straggler per pair
P = 3001
i = np.arange(P)
da = np.r_[2 * i, 2 * i[:-1] + 1, 2 * i].astype(np.int32)
db = np.r_[2 * i + 1, 2 * i[1:], 2 * P + i].astype(np.int32)
dw = np.r_[1e-3 * (i + 1), 10.0 + i[:-1], 9.5 + i]
deep = pkg.cluster_tree(torch.from_numpy(da).cuda(), torch.from_numpy(db).cuda(), torch.from_numpy(dw).cuda(), 3 * P, 2, ctx=ctx)
depth = int((deep.parent > 0).sum().item() // 2)
total, parts, floor = constrained_spans(deep, constraints(3 * P, 3001, 7), reps)
print(f"deep chain tree n={3 * P} K={deep.n_tree} (about {depth} levels) m=3001: median {med(total):.3f} ms device span; "
      f"climb {parts['cfl_climb']:.3f} ms = {1e3 * parts['cfl_climb'] / depth:.2f} us per level, one lane after another")
print("    parts (ms): " + ", ".join(f"{p[4:]} {v:.3f}" for p, v in parts.items()))
