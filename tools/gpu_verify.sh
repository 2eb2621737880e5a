# GPU box: the full GPU suite, then the full bench line (each step under its own limit, chained).
# Usage: bash tools/gpu_verify.sh [tag]; logs and the JSON line go to $OUT (default bench_out/).
set -e
cd "$(dirname "$0")/.."
OUT=${OUT:-bench_out}
mkdir -p $OUT
T=${1:-r03}
timeout -k 10 480 python -u -m pytest tests -m gpu -x -q --timeout 120 --timeout-method thread > $OUT/${T}_gpu_tests.log 2>&1 || { tail -40 $OUT/${T}_gpu_tests.log; exit 1; }
tail -2 $OUT/${T}_gpu_tests.log
timeout -k 10 600 python bench.py --full > $OUT/${T}_bench.json 2> $OUT/${T}_bench.err
python -c "import json; d=json.load(open('$OUT/${T}_bench.json')); print(d['value'], d['ms_per_step'], d['kernels_us'], {k: (v.get('value'), v.get('roofline', {}).get('frac')) for k, v in d['secondary'].items()})"
