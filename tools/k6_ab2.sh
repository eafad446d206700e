# K6 A/B: dc_link variants (HDB_OPTS=flat_link_variant=0|1): tests, interleaved 1M timings, trace of the default
# output under $OUT (default build/k6ab2); every run keeps its stderr (tools_stderr.log)
OUT=${OUT:-build/k6ab2}
mkdir -p "$OUT" && export TMPDIR=/tmp && \
HDB_OPTS=flat_link_variant=1 timeout -k 10 300 python -u -m pytest tests/test_gpu_flat.py -x -q --timeout 200 --timeout-method thread > "$OUT/test_l1.log" 2>&1 && \
for r in 1 2 3; do for v in 0 1; do echo -n "link=$v "; HDB_OPTS=flat_link_variant=$v timeout -k 10 120 python -u tools/flat_bench.py 1000000 20 2>>"$OUT/tools_stderr.log" | tail -1; done; done > "$OUT/bench.log" 2>&1 && \
timeout -k 10 200 rocprofv3 --kernel-trace -d "$OUT/trace" -o ft --output-format csv -- python3 tools/flat_bench.py 1000000 3 > "$OUT/prof.log" 2>&1; echo rc=$?
