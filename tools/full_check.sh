set -e
export TMPDIR=/tmp
cd ${REPO_ROOT:-$PWD}
mkdir -p ${OUT_DIR:-bench_out}
timeout -k 10 900 python3 -u -m pytest tests -m gpu -x -q --timeout 300 --timeout-method thread > ${OUT_DIR:-bench_out}/full_gpu.log 2>&1
timeout -k 10 120 python3 -c "import __graft_entry__ as g; g.smoke(); print('smoke ok')" > ${OUT_DIR:-bench_out}/smoke.log 2>&1
timeout -k 10 300 python3 bench.py --full > ${OUT_DIR:-bench_out}/bench.json 2> ${OUT_DIR:-bench_out}/bench.err
