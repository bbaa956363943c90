set -e
export TMPDIR=/tmp
cd ${REPO_ROOT:-$PWD}
mkdir -p ${OUT_DIR:-bench_out}
: > ${OUT_DIR:-bench_out}/kernarg_ab.txt
for v in unset 1 0 unset 1 0; do
  if [ $v = unset ]; then unset HIP_FORCE_DEV_KERNARG; else export HIP_FORCE_DEV_KERNARG=$v; fi
  timeout -k 10 300 python3 -u bench.py --full --steps 128 --warmup 8 --no-cpu-baseline > ${OUT_DIR:-bench_out}/ka.json 2>> ${OUT_DIR:-bench_out}/ka.err
  echo "$v $(python3 -c "import json;d=json.load(open('${OUT_DIR:-bench_out}/ka.json'));print(d['value'], d['ms_per_step'])")" >> ${OUT_DIR:-bench_out}/kernarg_ab.txt
done
