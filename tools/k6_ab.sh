# K6 A/B: dc_root variants (HDB_OPTS=flat_root_variant=N): GPU tests per variant, then interleaved 1M timings
# output under $OUT (default build/k6ab); every run keeps its stderr (tools_stderr.log)
OUT=${OUT:-build/k6ab}
mkdir -p "$OUT" && export TMPDIR=/tmp && \
for v in 3 4 5; do HDB_OPTS=flat_root_variant=$v timeout -k 10 300 python -u -m pytest tests/test_gpu_flat.py -x -q --timeout 200 --timeout-method thread > "$OUT/test_v$v.log" 2>&1 || exit 1; done && \
for r in 1 2; do for v in 0 1 3 4 5; do echo -n "root=$v "; HDB_OPTS=flat_root_variant=$v timeout -k 10 120 python -u tools/flat_bench.py 1000000 20 2>>"$OUT/tools_stderr.log" | tail -1; done; done > "$OUT/bench.log" 2>&1; echo rc=$?
