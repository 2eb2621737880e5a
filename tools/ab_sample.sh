# A/B of the sampling workload (GPU box): bash tools/ab_sample.sh build_exp/libA.so ...  (default library first)
# The JSON line of each run goes to $OUT (default bench_out/).
set -e
OUT=${OUT:-bench_out}
mkdir -p $OUT
for r in 1 2; do
  for lib in default "$@"; do
    if [ "$lib" = default ]; then
      timeout -k 10 200 python bench.py --workload sample --no-cpu-baseline > $OUT/ab_s.json 2>/dev/null
    else
      BCNF_AMD_LIB=$lib timeout -k 10 200 python bench.py --workload sample --no-cpu-baseline > $OUT/ab_s.json 2>/dev/null
    fi
    python -c "import json; d=json.loads(open('$OUT/ab_s.json').read().strip().splitlines()[-1]); print('$lib', d['ms_per_step'], round(d['value']/1e6, 1), 'M draws/s')"
  done
done
