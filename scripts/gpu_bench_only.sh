set -e
cd /tmp && export TMPDIR=/tmp
cd $GRAFT_REPO_ROOT
O=${OUT:-out}/$1     # where the outputs go: OUT (default out) / <tag>
mkdir -p $O
python bench.py --full > $O/bench_default.json 2> $O/bench_default.err || { tail -30 $O/bench_default.err; exit 1; }
python -c "
import json; d=json.load(open('$O/bench_default.json'))
print(d['value'], d['ms_per_step'], d['roofline']['frac'], d['roofline']['avg_launch_ms'])
print('f32', d['f32']['value'], d['f32']['roofline']['frac'])
print('c3', json.dumps(d['c3'], indent=1))
print('ingest', d['ingest'])
"
