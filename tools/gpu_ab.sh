#!/bin/bash
# A/B of environment switches on the training step: one short bench per line of $AB (semicolon-separated env assignments, "-" = defaults).
# usage (from the repository root): AB="-;KAI0_SIDE_STREAM=0;KAI0_SIDE_STREAM=0 KAI0_ASYNC_OPT=0" bash tools/gpu_ab.sh LOG_DIR
set -u
OUT="${1:?usage: AB=... bash tools/gpu_ab.sh LOG_DIR}"; mkdir -p "$OUT"
# a GPU step that timed out (124) or died by a signal (abort 134, kill 137, segfault 139, ...) ends the script: nothing more is
# started on a GPU that may have faulted
stop_if_fault() { if [ $1 = 124 ] || [ $1 -gt 128 ]; then echo "$2 timed out or died by a signal (rc=$1): stopping"; exit $1; fi; }
if [ -n "${PYTEST_K:-}" ]; then
  timeout -k 10 1800 python -m pytest tests -m gpu -q -x -k "$PYTEST_K" > $OUT/pytest_ab.log 2>&1; rc=$?; echo "pytest rc=$rc"; tail -3 $OUT/pytest_ab.log
  stop_if_fault $rc pytest
fi
IFS=';' read -ra CASES <<< "${AB:--}"
i=0
for c in "${CASES[@]}"; do
  [ "$c" = "-" ] && c=""
  env $c timeout -k 10 600 python bench.py --full --steps ${STEPS:-8} --warmup 3 --no-cpu-baseline ${BENCH_ARGS:---no-latency} > $OUT/ab_$i.log 2>&1
  rc=$?; stop_if_fault $rc "bench [${c:-defaults}]"
  python - "$c" $OUT/ab_$i.log <<'PY'
import json, sys
l = [x for x in open(sys.argv[2]) if x.startswith('{')]
if l:
    d = json.loads(l[-1]); r = d.get('roofline', {}); inf = d.get('inference', {})
    print(f"[{sys.argv[1] or 'defaults'}] samples/s {d['value']:.2f} ms/step {d['ms_per_step']:.1f} gemm frac {r.get('frac', 0):.4f} gemm ms {r.get('gemm_ms_per_step', 0):.1f} loss {d['config'].get('final_loss')} p50 {inf.get('p50_ms')} {inf.get('stages_ms')}")
else:
    print(f"[{sys.argv[1]}] FAILED", open(sys.argv[2]).read()[-1500:])
PY
  i=$((i+1))
done
