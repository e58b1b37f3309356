# One GPU-box call: the whole -m gpu suite, then the --full bench line.  Output under $OUT/<tag> (default out/<tag>).
set -e
cd /tmp && export TMPDIR=/tmp
cd $GRAFT_REPO_ROOT
R=${1:-r02}
O=${OUT:-out}/$R
mkdir -p $O
python -m pytest tests -m gpu -x -q --durations=15 > $O/gpu_tests.log 2>&1 || { tail -60 $O/gpu_tests.log; exit 1; }
tail -25 $O/gpu_tests.log
python bench.py --full > $O/bench_default.json 2> $O/bench_default.err || { tail -30 $O/bench_default.err; exit 1; }
python -c "
import json; d=json.load(open('$O/bench_default.json'))
print(d['value'], d['ms_per_step'], d['roofline'], d['accuracy'])
print('f32', d['f32'])
print('cpu', d['cpu_baseline'])
"
