# GPU: parity tests -> full bench line (cpu_baseline + roofline + secondary) -> rocprofv3 kernel-trace summary
# results go to $OUT (default bench_out/)
set -o pipefail
cd "$GRAFT_REPO_ROOT"
export TMPDIR=/tmp
OUT=${OUT:-bench_out}; mkdir -p "$OUT"
timeout -k 10 900 python -u -m pytest tests -x -v -m gpu -p no:cacheprovider --timeout 300 --timeout-method thread > "$OUT"/pytest.log 2>&1
rc=$?; echo "pytest rc=$rc"; tail -3 "$OUT"/pytest.log
[ $rc -eq 0 ] || exit $rc
timeout -k 10 600 python bench.py --full > "$OUT"/bench_full.json 2> "$OUT"/bench_full.err
rc=$?; echo "bench rc=$rc"; cat "$OUT"/bench_full.json
[ $rc -eq 0 ] || exit $rc
timeout -k 10 600 rocprofv3 --kernel-trace --stats -d "$OUT"/prof -o run --output-format csv -- \
  python bench.py --full --no-cpu-baseline > "$OUT"/prof_bench.log 2>&1
echo "rocprof rc=$?"
