#!/bin/bash
# configs[4] attention: long-range GQA K/V ring depth (TI_ATTN_RING_LONG 4 product | 6 | 8 in exp/).
set -e
export TMPDIR=/tmp
cd ${REPO_ROOT:-$PWD}
mkdir -p ${OUT_DIR:-bench_out}
: > ${OUT_DIR:-bench_out}/c4_ring_ab.txt
for v in 4 6 8 4; do
  if [ $v = 4 ]; then L=""; else L=${REPO_ROOT:-$PWD}/exp/l$v/libturboinfer_amd.so; fi
  TI_LIB=$L timeout -k 10 300 python3 -u bench.py --full --model llama3-8b --batch 32 --kv 8192 --steps 16 --warmup 3 --no-cpu-baseline > ${OUT_DIR:-bench_out}/c4_r$v.json 2>> ${OUT_DIR:-bench_out}/c4_ring_ab.err
  echo "$v $(python3 -c "import json;d=json.load(open('${OUT_DIR:-bench_out}/c4_r$v.json'));print(d['value'], d['ms_per_step'], d['kernels'].get('attention'))")" >> ${OUT_DIR:-bench_out}/c4_ring_ab.txt
done
TI_LIB=${REPO_ROOT:-$PWD}/exp/l6/libturboinfer_amd.so timeout -k 10 300 python3 -u -m pytest tests/test_gpu_engine.py -x -q -k "llama3 or 8192" --timeout 200 --timeout-method thread > ${OUT_DIR:-bench_out}/c4_ring_tests.log 2>&1
