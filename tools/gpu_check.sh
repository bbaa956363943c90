set -e
export TMPDIR=/tmp
cd ${REPO_ROOT:-$PWD}
mkdir -p ${OUT_DIR:-bench_out}
timeout -k 10 500 python3 -u -m pytest tests -m gpu -x -q --timeout 120 --timeout-method thread --durations=15 > ${OUT_DIR:-bench_out}/gpu_tests.log 2>&1
timeout -k 10 300 python3 bench.py --full > ${OUT_DIR:-bench_out}/bench.json 2> ${OUT_DIR:-bench_out}/bench.err
