#!/bin/bash
# one GPU session: parity tests, bench, rocprof kernel trace.  Stops at the first GPU fault.
cd "${GRAFT_REPO_ROOT:-.}"
mkdir -p ${OUT_DIR:-bench_out}
export TMPDIR=/tmp
if [ "${SKIP_TESTS:-0}" != "1" ]; then
timeout -k 10 120 python -u -c "import __graft_entry__ as g; g.smoke()" > ${OUT_DIR:-bench_out}/smoke.log 2>&1
rc=$?; echo "smoke rc=$rc"; tail -2 ${OUT_DIR:-bench_out}/smoke.log
[ $rc -ne 0 ] && exit $rc
timeout -k 10 900 python -u -m pytest tests -m gpu -x -v --timeout 300 --timeout-method thread > ${OUT_DIR:-bench_out}/pytest_gpu.log 2>&1
rc=$?; echo "pytest rc=$rc"; tail -5 ${OUT_DIR:-bench_out}/pytest_gpu.log
if [ $rc -ne 0 ] && [ $rc -ne 1 ]; then exit $rc; fi
fi
timeout -k 10 300 python -u bench.py --full --steps 5 --warmup 2 ${BENCH_ARGS:-} > ${OUT_DIR:-bench_out}/bench.log 2>&1
rc=$?; echo "bench rc=$rc"; tail -3 ${OUT_DIR:-bench_out}/bench.log
[ $rc -ne 0 ] && exit $rc
if [ "${PROFILE:-1}" = "1" ]; then
  timeout -k 10 300 rocprofv3 --kernel-trace --stats -d ${OUT_DIR:-bench_out}/prof -o run --output-format csv -- python -u bench.py --full --steps 3 --warmup 1 --no-cpu-baseline > ${OUT_DIR:-bench_out}/prof.log 2>&1
  rc=$?; echo "rocprof rc=$rc"; tail -3 ${OUT_DIR:-bench_out}/prof.log
fi
exit 0
