# GPU box: FC_small training / fold / parity GPU tests, then same-box A/B of the headline step (working tree vs
# build_exp/libhead.so): bench.py --full without sub-lines (for the per-kernel times), twice each. Logs and the JSON
# line of each run go to $OUT (default bench_out/).
set -e
cd "$(dirname "$0")/.."
OUT=${OUT:-bench_out}
mkdir -p $OUT
T=${1:-r03}
timeout -k 10 300 python -u -m pytest tests/test_gpu_train.py tests/test_gpu_fold.py tests/test_gpu_parity.py tests/test_gpu_dp.py -m gpu -x -q --timeout 120 --timeout-method thread > $OUT/${T}_step_tests.log 2>&1 || { tail -40 $OUT/${T}_step_tests.log; exit 1; }
tail -1 $OUT/${T}_step_tests.log
for r in 1 2; do
  for lib in default ${AB_LIBS:-build_exp/libhead.so}; do
    if [ "$lib" = default ]; then
      timeout -k 10 200 python bench.py --full --no-secondary --no-cpu-baseline > $OUT/ab_s.json 2>/dev/null
    else
      BCNF_AMD_LIB=$lib timeout -k 10 200 python bench.py --full --no-secondary --no-cpu-baseline > $OUT/ab_s.json 2>/dev/null
    fi
    python -c "import json; d=json.loads(open('$OUT/ab_s.json').read().strip().splitlines()[-1]); print('$lib', d['ms_per_step'], round(d['value']/1e6, 2), 'M samples/s', d['kernels_us'])"
  done
done 2>&1 | tee $OUT/${T}_ab_step.txt
