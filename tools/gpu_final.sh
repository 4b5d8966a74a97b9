# the whole check of a tree, in one call: every GPU test, smoke(), the
# benchmark with every line (--full); logs and the result go to $OUT
set -e
TAG=${1:-final}
OUT=${OUT:-bench_out}
mkdir -p $OUT
timeout -k 10 900 python -u -m pytest tests -q -m gpu -x --timeout 300 --timeout-method thread > $OUT/pytest_gpu_$TAG.log 2>&1 || { tail -40 $OUT/pytest_gpu_$TAG.log; exit 1; }
echo tests-ok; tail -1 $OUT/pytest_gpu_$TAG.log
timeout -k 10 300 python -c "import __graft_entry__ as g; g.smoke(); print('smoke-ok')"
timeout -k 10 600 python bench.py --full > $OUT/bench_$TAG.json 2> $OUT/bench_$TAG.err || { tail $OUT/bench_$TAG.err; exit 1; }
python3 -c "import json; d=json.load(open('$OUT/bench_$TAG.json')); print('bench', d['value']/1e9, d['ms_per_step'], d['roofline']['frac'], d['cpu_baseline']['value'])"
