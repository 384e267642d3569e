#!/bin/bash
# the whole -m gpu suite, smoke, the default bench line, a 1-rank RCCL dry run of the N > 1 bench path, the serve path's host share
# usage: bash tools/gpu_round.sh LOG_DIR   (from the repository root; logs go to LOG_DIR)
set -u
OUT="${1:?usage: bash tools/gpu_round.sh LOG_DIR}"; mkdir -p "$OUT"
# gpu NAME SECONDS LOG CMD...: one GPU step under its own time limit; a time-out (124) or a death by signal (abort 134, kill 137,
# segfault 139, ...) ends the script, so nothing more is started on a GPU that may have faulted
gpu() {
  local name=$1 limit=$2 log=$3; shift 3
  local t0=$(date +%s)
  timeout -k 10 "$limit" "$@" > "$log" 2>&1; local rc=$?
  echo "$name rc=$rc in $(( $(date +%s) - t0 )) s"
  if [ $rc = 124 ] || [ $rc -gt 128 ]; then echo "$name timed out or died by a signal: stopping"; exit $rc; fi
}
gpu pytest 3000 $OUT/pytest_gpu.log python -m pytest tests -m gpu -q --durations=10
grep -E "passed|failed" $OUT/pytest_gpu.log | tail -1; grep -E "^FAILED|^ERROR" $OUT/pytest_gpu.log | head
gpu smoke 300 $OUT/smoke.log python -c "import __graft_entry__ as g; g.smoke()"
tail -1 $OUT/smoke.log | cut -c1-200
gpu bench 900 $OUT/bench_default.log python bench.py --full
tail -1 $OUT/bench_default.log | python -c "
import json,sys
d=json.loads(sys.stdin.read()); r=d['roofline']; i=d['inference']; f=r['families']
print('samples/s', round(d['value'],2), 'ms/step', round(d['ms_per_step'],1), 'gemm frac', round(r['frac'],4), 'headline-schedule frac', round(r['headline_schedule']['frac'],4) if r.get('headline_schedule') else None, 'step frac', round(r['step_frac_of_mfma_peak'],4))
print('gemma_blocks', round(f['gemma_blocks']['frac'],3), 'vit_blocks', round(f['vit_blocks']['frac'],3), 'attention', round(f['attention']['frac'],3))
print('p50', round(i['p50_ms'],2), i.get('stages_ms'), 'trimmed', i.get('trimmed_prompt',{}).get('p50_ms'))
print('cpu', {k: d['cpu_baseline'][k] for k in ('value','cores','vocab','fwd_bwd_s_per_sample','optimizer_s')}, 'ranks', d['ranks']['rccl_ranks_seen'], d['ranks']['devices'][0]['device'][:40])"
gpu "1-rank RCCL bench" 600 $OUT/bench_rccl1.log env KAI0_FORCE_COLLECTIVES=1 KAI0_BENCH_FSDP=0 \
  python bench.py --full --steps 3 --warmup 1 --no-cpu-baseline --no-latency --no-trim-extra
tail -1 $OUT/bench_rccl1.log | cut -c1-300
gpu policy_latency 300 $OUT/policy_latency.log python tools/policy_latency.py 30
tail -1 $OUT/policy_latency.log | cut -c1-500
