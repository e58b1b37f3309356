# Full-size rehearsal of the N>1 path on the ONE GPU of a box (round-5 verdict W4a): the headline problem (3600 x 1800 x 75 x 12,
# float64, 65 transects) cut N ways, the N ranks started by bench.py's own launcher, all on device 0 (NF_FORCE_DEVICE=0), the
# reduce over gloo.  NOT a scaling measurement: the ranks share one GPU.  A box allows at most 6 processes on its card, so the
# 8-rank cut itself cannot be started here, and 6 ranks were ended by the box's process guard in round 6 (a seventh process --
# of the job before -- still had the card open); N = 5: cuts in the middle of time steps, 180 slabs = 2.4 steps per rank.  Checked: totals equal to the N = 1 line to 1e-13 relative, accuracy vs fluxexact, slab ranges.
set -e
cd /tmp && export TMPDIR=/tmp
cd $GRAFT_REPO_ROOT
R=$1
mkdir -p gpurun_out/$R
COMMON="--steps 3 --warmup 1 --full --no-cpu --dump-totals"
timeout -k 10 400 python bench.py --gpus 1 $COMMON --no-f32 --no-ingest --no-c3 > gpurun_out/$R/rehearsal_n1.json 2> gpurun_out/$R/rehearsal_n1.err || { tail -30 gpurun_out/$R/rehearsal_n1.err; exit 1; }
for N in 5; do
  NF_FORCE_DEVICE=0 NF_DIST_BACKEND=gloo timeout -k 10 500 python bench.py --gpus $N $COMMON > gpurun_out/$R/rehearsal_n$N.out 2> gpurun_out/$R/rehearsal_n$N.err || { tail -40 gpurun_out/$R/rehearsal_n$N.err; exit 1; }
  echo "N=$N done"
done
python - <<PY
import json, numpy
one = json.load(open('gpurun_out/$R/rehearsal_n1.json'))
b = numpy.array(one['totals'])
for N in (5,):
    d = json.loads([l for l in open('gpurun_out/$R/rehearsal_n%d.out' % N) if l.startswith('{')][0])
    a = numpy.array(d['totals'])
    rel = float(numpy.abs(a - b).max() / numpy.abs(b).max())
    want = [[(r * 900) // N, ((r + 1) * 900) // N] for r in range(N)]
    got = [r['slabs'] for r in d['ranks']]
    print(N, 'ranks on one GPU over', d['reduce']['backend'], ': n_gpus', d['n_gpus'], 'ms_per_step', round(d['ms_per_step'], 2),
          'max rel diff of the totals vs N=1', rel, 'max_abs_err_vs_fluxexact', d['accuracy']['max_abs_err_vs_fluxexact'],
          'slabs', got, 'steps touched', [r['steps_touched'] for r in d['ranks']], 'launches', [r['launches_per_pass'] for r in d['ranks']])
    assert rel <= 1e-13 and d['accuracy']['max_abs_err_vs_fluxexact'] <= 1e-11 and got == want and d['n_gpus'] == N
    d.pop('totals')
    head = {'what_this_is': f'{N} ranks SHARING ONE GPU over gloo (NF_FORCE_DEVICE=0 NF_DIST_BACKEND=gloo python bench.py --gpus {N} '
                            '--steps 3 --warmup 1 --full --no-cpu --dump-totals): a rehearsal of the launcher, the slab bookkeeping, the reduce '
                            'and the accuracy block at the headline size -- NOT a scaling measurement, the value is meaningless as a rate',
            'totals_max_rel_diff_vs_n1': rel, 'n1_ms_per_step': one['ms_per_step']}
    with open('gpurun_out/$R/rehearsal%d.json' % N, 'w') as f:
        f.write(json.dumps(head) + '\n' + json.dumps(d) + '\n')
print('full-size rehearsal OK')
PY
