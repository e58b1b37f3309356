set -e
cd /tmp && export TMPDIR=/tmp
cd $GRAFT_REPO_ROOT
R=r06
O=${OUT:-out}/$R
python tools/filebacked_timing.py 1440 1021 75 24 > $O/filebacked_timing.txt 2>&1 || { tail -20 $O/filebacked_timing.txt; exit 1; }
cat $O/filebacked_timing.txt
NF_STAGE_TRACE=1 NF_TIMING_LEGS=device python tools/filebacked_timing.py 1440 1021 75 24 2>&1 | grep -a 'staging:' | tail -18 > $O/stage_trace.txt || true
cat $O/stage_trace.txt
python bench.py --full --no-cpu --no-f32 --no-c3 --steps 5 > $O/bench_ingest.json 2> $O/bench_ingest.err || { tail -30 $O/bench_ingest.err; exit 1; }
python -c "
import json; d=json.load(open('$O/bench_ingest.json')); print(json.dumps(d['ingest'], indent=1))"
