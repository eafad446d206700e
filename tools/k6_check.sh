# K6 check: flat-label GPU tests, the 1M timing, the C2 bench, and a kernel trace
# output under $OUT (default build/k6); every run keeps its stderr (tools_stderr.log)
OUT=${OUT:-build/k6}
mkdir -p "$OUT" && export TMPDIR=/tmp && \
timeout -k 10 300 python -u -m pytest tests/test_gpu_flat.py -x -v --timeout 200 --timeout-method thread > "$OUT/test.log" 2>&1 && \
for r in 1 2; do for lb in 9 10; do echo -n "lb=$lb "; HDB_OPTS=flat_block_log=$lb timeout -k 10 120 python -u tools/flat_bench.py 1000000 20 2>>"$OUT/tools_stderr.log" | tail -1; done; done > "$OUT/bench.log" 2>&1 && \
timeout -k 10 200 python -u bench.py --no-cpu-baseline > "$OUT/c2.log" 2>&1 && \
timeout -k 10 200 rocprofv3 --kernel-trace -d "$OUT/trace" -o ft --output-format csv -- python3 tools/flat_bench.py 1000000 3 > "$OUT/prof.log" 2>&1; echo rc=$?
