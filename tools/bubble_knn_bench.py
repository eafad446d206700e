"""K5 bubble core distances (bubble kNN + the stale-index epilogue) at C5's model size:
16,384 bubbles x 8, minPts 4 -- chunked scan with event replay vs the one-thread-per-bubble
scan (option bubble_knn_split; HDB_OPTS=bubble_knn_split=0 sets it for a whole program), equal
results.  usage: python tools/bubble_knn_bench.py [b] [d]"""
import importlib
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
pkg = importlib.import_module("232-hierarchical-density-based-clustering-using-mapreduce_amd")
b = int(sys.argv[1]) if len(sys.argv) > 1 else 16384
d = int(sys.argv[2]) if len(sys.argv) > 2 else 8
rng = np.random.default_rng(0)
X = rng.normal(size=(b, d)) * 10
eB = np.abs(rng.normal(0.3, 0.1, b))
nnB = np.abs(rng.normal(0.2, 0.05, b))
nB = rng.integers(1, 9, b).astype(np.int32)
ctx = pkg.Context.get(0)
model = pkg.HdbscanDataBubbles(ctx)
res = {}
for rep in range(2):
    for split in (0, 1):
        ctx.set_option("bubble_knn_split", split)
        model.calculateCoreDistancesBubbles(X, nB, eB, nnB, 4)
        ctx.set_timing(True)
        ctx.kernel_time("bubble_knn")
        t = time.perf_counter()
        for _ in range(3):
            c = model.calculateCoreDistancesBubbles(X, nB, eB, nnB, 4)
        dt = (time.perf_counter() - t) / 3
        ms, cnt = ctx.kernel_time("bubble_knn")
        ctx.set_timing(False)
        if 0 in res and split == 1:
            assert np.array_equal(res[0], c), "split scan differs"
        res[split] = c
        print(f"split={split} b={b} d={d}: call {dt * 1e3:.2f} ms, bubble_knn kernels {ms / max(cnt, 1):.2f} ms", flush=True)
ctx.set_option("bubble_knn_split", 1)
print("identical core distances")
