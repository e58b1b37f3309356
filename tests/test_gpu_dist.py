"""GPU parity, part 3: the N>1 path with the REAL engine.  Two processes share the one GPU of the test box (RCCL needs
one GPU per rank, so the collective runs over gloo on host tensors here); each integrates its (t,z) slab range on
the GPU, one all_reduce combines the rows, and rank 0 compares with the single-rank result.  The RCCL/xGMI path itself is
exercised by the driver's multi-GPU bench."""
import os
import socket
import sys

import numpy
import pytest
import torch
import torch.multiprocessing as mp

from conftest import ROOT

pytestmark = pytest.mark.gpu

PSI = "(1+10*z)*(t+1)*(cos(2*pi*y/360) + sin(2*pi*x/360))"
TRANSECTS = [[(-100., -80., 0.), (100., -80., 0.), (0., 80., 0.)],
             [(-100., -80., 0.), (100., -80., 0.), (0., 80., 0.), (-100., -80., 0.)],
             [(-170., 10., 0.), (-20., -55., 0.), (135., 62., 0.)]]
NX, NY, NZ, NT = 180, 90, 7, 5     # 35 slabs over 2 ranks: rank 0 ends in the middle of time step 2


def _rows(rank, world, local_window):
    import contextlib
    import io
    from nemoflux_amd import dist as nfdist
    from nemoflux_amd._lib import DeviceArray
    from nemoflux_amd.datagen import DataGen
    from nemoflux_amd.field import Field
    dg = DataGen()
    dg.setSizes(NX, NY, NZ, NT)
    dg.setBoundingBox(-180., 180., -90., 90., 0., 1.)
    dg.build()
    dg.applyStreamFunction(PSI)
    sr = nfdist.slab_range(NT, NZ, rank, world)
    if local_window:   # hold only the touched time steps, address them through the virtual global base
        t0, t1 = nfdist.time_steps_touched(sr, NZ)
        u, v = dg.computeUVFromPotential(t0, t1)
        ug = DeviceArray(nfdist.virtual_base(u, t0 * NZ, NY * NX), (NT, NZ, NY, NX), 'float64', u)
        vg = DeviceArray(nfdist.virtual_base(v, t0 * NZ, NY * NX), (NT, NZ, NY, NX), 'float64', v)
    else:
        ug, vg = dg.computeUVFromPotential()
    with contextlib.redirect_stdout(io.StringIO()):
        fld = Field.fromArrays(dg.bounds_lon, dg.bounds_lat, dg.deptht_bounds, ug, vg,
                               [numpy.array(t) for t in TRANSECTS], slab_range=sr, readback=False)
    out = torch.zeros((NT, fld._rowlen), dtype=torch.float64, device='cuda')
    fld.computeAll(out=out)
    return out


def _worker(rank, world, port, out_path):
    sys.path.insert(0, ROOT)
    os.environ.update(MASTER_ADDR='127.0.0.1', MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world),
                      LOCAL_RANK='0')
    import torch.distributed as dist
    from nemoflux_amd import dist as nfdist
    nfdist.init_from_env(backend='gloo')
    rows = _rows(rank, world, local_window=True).cpu()
    nfdist.reduce_rows(rows)
    if rank == 0:
        numpy.save(out_path, rows.numpy())
    dist.destroy_process_group()


def test_two_ranks_one_gpu_gloo(tmp_path):
    s = socket.socket()
    s.bind(('127.0.0.1', 0))
    port = s.getsockname()[1]
    s.close()
    out = str(tmp_path / 'rows.npy')
    mp.spawn(_worker, args=(2, port, out), nprocs=2, join=True)
    got = numpy.load(out)
    full = _rows(0, 1, local_window=False).cpu().numpy()
    assert got.shape == full.shape
    assert numpy.allclose(got, full, rtol=1e-13, atol=1e-13 * numpy.abs(full).max())
    from nemoflux_amd.fluxexact import exactFlux
    nseg = sum(len(t) - 1 for t in TRANSECTS)
    ex = numpy.array(exactFlux(PSI, TRANSECTS[0], NZ, NT))
    assert numpy.abs(got[:, nseg + 0] - ex).max() <= 1e-12 * numpy.abs(ex).max()
    assert numpy.abs(got[:, nseg + 1]).max() <= 1e-12 * numpy.abs(ex).max()


def test_bench_contract_small_workload():
    """bench.py --full prints exactly one JSON line with the contract's keys (tiny workload, CPU leg included)."""
    import json
    import subprocess
    out = subprocess.run([sys.executable, os.path.join(ROOT, 'bench.py'), '--steps', '2', '--warmup', '1', '--nx', '144',
                          '--ny', '72', '--nz', '9', '--nt', '3', '--batch', '6', '--full'], capture_output=True, text=True,
                         timeout=600, cwd=ROOT)
    assert out.returncode == 0, out.stderr[-2000:]
    lines = [l for l in out.stdout.splitlines() if l.strip()]
    assert len(lines) == 1
    d = json.loads(lines[0])
    for k in ('metric', 'value', 'unit', 'n_gpus', 'steps', 'warmup', 'ms_per_step', 'higher_is_better', 'scaling',
              'vs_baseline', 'dtype', 'data', 'config', 'roofline', 'cpu_baseline'):
        assert k in d, k
    assert d['n_gpus'] == 1 and d['steps'] == 2 and d['warmup'] == 1 and d['higher_is_better'] is True
    assert d['vs_baseline'] is None and d['dtype'] == 'f64' and d['data'] == 'synthetic' and 'workload' in d['config']
    r = d['roofline']
    assert r['bound'] == 'hbm' and r['unit'] == 'GB/s' and r['peak'] == 8000.0
    assert abs(r['frac'] - r['achieved'] / r['peak']) < 1e-3 and r['achieved'] > 0
    c = d['cpu_baseline']
    assert c['kind'] == 'port' and c['value'] > 0 and c['cores'] >= 1 and c['unit'] == d['unit']
    assert d['accuracy']['max_abs_err_vs_fluxexact'] <= 1e-11 * max(1.0, d['accuracy']['max_abs_exact'])
    assert abs(d['value'] - 144 * 72 * 9 * 3 * 2 / (d['ms_per_step'] * 2e-3)) <= 1e-6 * d['value']
    assert d['scaling'] == 'strong' and 'legs' in c and c['legs']['a6_a7_all_cores_s'] > 0
    assert r['traffic'] is None and r['traffic_source'] is None       # no PMC pass exists for this toy workload
    f = d['f32']                                                      # float32 sub-record of the same workload
    assert f['dtype'] == 'f32' and f['value'] > 0 and f['roofline']['frac'] > 0
    assert abs(f['roofline']['algorithmic_bytes_per_unit'] - (8 + 64.0 / 9)) < 1e-3
    assert f['accuracy']['max_abs_err_vs_fluxexact'] <= 1e-5 * max(1.0, f['accuracy']['max_abs_exact'])
    g = d['ingest']                                                   # file-ingest sub-record: one launch of the device decoder
    assert g.get('bit_identical') is True and g['MB_per_s_per_stream'] > 10 and g['inflate_unshuffle_place_ms'] > 0, g


def test_bench_plain_run_is_lean(tmp_path):
    """A plain bench.py line carries the headline and the roofline of its own timed steps, none of what --full adds; with
    --dump-outputs a plain run writes the same arrays as a --full run (the float32 and C3 workloads run for it)."""
    import json
    import subprocess
    small = ['--steps', '2', '--warmup', '1', '--nx', '144', '--ny', '72', '--nz', '9', '--nt', '3', '--batch', '6']
    lines = {}
    for name, extra in (('plain', []), ('plain_dump', ['--dump-outputs', str(tmp_path / 'plain')]),
                        ('full_dump', ['--full', '--no-cpu', '--no-ingest', '--dump-outputs', str(tmp_path / 'full')])):
        out = subprocess.run([sys.executable, os.path.join(ROOT, 'bench.py')] + small + extra, capture_output=True,
                             text=True, timeout=600, cwd=ROOT)
        assert out.returncode == 0, out.stderr[-2000:]
        got = [l for l in out.stdout.splitlines() if l.strip()]
        assert len(got) == 1
        lines[name] = json.loads(got[0])
    d = lines['plain']
    assert d['metric'] == 'edge-flux integrals/sec' and d['unit'] == 'integrals/s' and d['higher_is_better'] is True
    assert d['dtype'] == 'f64' and d['steps'] == 2 and d['warmup'] == 1 and d['roofline']['launches'] >= 2
    assert abs(d['value'] - 144 * 72 * 9 * 3 * 2 / (d['ms_per_step'] * 2e-3)) <= 1e-6 * d['value']
    for k in ('accuracy', 'cpu_baseline', 'f32', 'ingest', 'c3', 'dumped_outputs'):
        assert k not in d, k
    assert 'weights_build_ms' not in d['config'] and 'accuracy' in lines['full_dump']
    assert lines['plain_dump']['dumped_outputs'] == lines['full_dump']['dumped_outputs']
    names = sorted(f.name for f in (tmp_path / 'full').iterdir())
    assert names == sorted(f.name for f in (tmp_path / 'plain').iterdir()) and 'f32_transect_totals.npy' in names
    assert 'c3_f64_segment_fluxes.npy' in names
    for f in names:
        a, b = numpy.load(tmp_path / 'plain' / f), numpy.load(tmp_path / 'full' / f)
        assert a.shape == b.shape and numpy.allclose(a, b, rtol=0, atol=1e-13 * max(1.0, float(numpy.abs(b).max()))), f


def test_readme_examples_script():
    """examples/readme_examples.py: every worked example of the reference's README within 1e-9 of its answer
    (the rotated closed loop carries the reference's own ~1e-11 arc-length conditioning error)."""
    import runpy
    mod = runpy.run_path(os.path.join(ROOT, 'examples', 'readme_examples.py'))
    assert mod['main']() <= 1e-9


def test_rccl_calls_of_the_bench_on_one_rank():
    """The exact RCCL calls bench.py / nemoflux_amd.dist make at N>1 (init bound to the GPU, all_reduce SUM and MAX,
    barrier with device_ids) on a one-rank communicator: all this box can run of the 'nccl' backend."""
    import subprocess
    with socket.socket() as s:
        s.bind(('127.0.0.1', 0))
        port = s.getsockname()[1]
    env = dict(os.environ, MASTER_ADDR='127.0.0.1', MASTER_PORT=str(port))
    r = subprocess.run([sys.executable, os.path.join(ROOT, 'tools', 'rccl_world1.py')], env=env, capture_output=True,
                       text=True, timeout=600)
    assert r.returncode == 0 and 'rccl world-1 OK' in r.stdout, r.stdout[-2000:] + r.stderr[-2000:]


def test_plain_c_client_of_the_abi(tmp_path):
    """examples/c_client.c (README case C1 through both ABI levels, from C): 360 twice, mint's error convention."""
    import subprocess
    from test_abi import build_c_client
    r = subprocess.run([build_c_client(tmp_path)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and 'C client OK' in r.stdout, r.stdout[-2000:] + r.stderr[-2000:]
    assert 'level 2: 5 segments, flux = 360.0000' in r.stdout and 'level 1: 648 cells, flux = 360.0000' in r.stdout
    assert 'ingest: decoded 1.0 (status 0)' in r.stdout
    assert 'reduce: 1 rank(s), rank 0 on device 0, row = 1.5 -2.0 360.0' in r.stdout      # nf_rows_allreduce from plain C


def _bench_json(extra, nproc=1, launcher='torchrun', env_extra=None, with_stderr=False):
    """Run bench.py on a small grid -- directly (N=1), under torch.distributed.run with `nproc` ranks (the driver's N>1
    command), or as plain `python bench.py --gpus N` (launcher='self': bench.py starts its own ranks); with N>1 all ranks
    use GPU 0 and reduce over gloo (NF_FORCE_DEVICE / NF_DIST_BACKEND: the rehearsal hook of nemoflux_amd.dist).
    Returns the parsed JSON line."""
    import json
    import subprocess
    small = ['--nx', '144', '--ny', '72', '--nz', '9', '--batch', '6', '--steps', '2', '--warmup', '1', '--full', '--no-cpu',
             '--no-f32', '--no-ingest', '--no-c3', '--dump-totals'] + extra
    env = dict(os.environ)
    if nproc == 1:
        cmd = [sys.executable, os.path.join(ROOT, 'bench.py'), '--gpus', '1'] + small
    else:
        with socket.socket() as s:
            s.bind(('127.0.0.1', 0))
            port = s.getsockname()[1]
        env.update(NF_FORCE_DEVICE='0', NF_DIST_BACKEND='gloo')
        env.pop('WORLD_SIZE', None)
        if launcher == 'self':
            cmd = [sys.executable, os.path.join(ROOT, 'bench.py'), '--gpus', str(nproc)] + small
        else:
            cmd = [sys.executable, '-m', 'torch.distributed.run', '--nnodes=1', f'--nproc-per-node={nproc}',
                   '--master-addr', '127.0.0.1', '--master-port', str(port), os.path.join(ROOT, 'bench.py'),
                   '--gpus', str(nproc)] + small
    env.update(env_extra or {})
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=900, cwd=ROOT, env=env)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-3000:]
    lines = [l for l in r.stdout.splitlines() if l.startswith('{')]
    assert len(lines) == 1, r.stdout[-2000:]
    return (json.loads(lines[0]), r.stderr) if with_stderr else json.loads(lines[0])


@pytest.mark.parametrize('scaling', ['strong', 'weak', 'default'])
def test_bench_two_ranks_rehearsal(scaling):
    """bench.py's own N>1 branch end to end (slab windows, virtual base, reduce, barrier, MAX of the elapsed time, the
    JSON line from rank 0) with 2 ranks on the one GPU of this box: the transect totals must equal the N=1 run of the
    same global problem to 1e-13 (the summation order differs), n_gpus == 2, and the default scaling is strong."""
    nt = 3
    args = [] if scaling == 'default' else ['--scaling', scaling]
    two = _bench_json(['--nt', str(nt)] + args, nproc=2)
    nt_global = 2 * nt if scaling == 'weak' else nt
    one = _bench_json(['--nt', str(nt_global)])
    assert two['n_gpus'] == 2 and one['n_gpus'] == 1
    assert two['scaling'] == ('weak' if scaling == 'weak' else 'strong') and one['scaling'] == 'strong'
    assert two['config']['nt_global'] == nt_global and ('strong' if scaling != 'weak' else 'weak') in two['config']['workload']
    a, b = numpy.array(two['totals']), numpy.array(one['totals'])
    assert a.shape == b.shape == (nt_global, 7)
    assert numpy.abs(a - b).max() <= 1e-13 * numpy.abs(b).max()
    assert two['accuracy']['max_abs_err_vs_fluxexact'] <= 1e-11 * max(1.0, two['accuracy']['max_abs_exact'])
    red = two['reduce']
    assert red['message_bytes'] == nt_global * (two['config']['target_segments'] + 7) * 8 and red['allreduce_ms'] > 0
    assert red['backend'] == 'gloo' and 'cpu_baseline' not in two and 'reduce' not in one
    units = 144 * 72 * 9 * nt_global
    assert abs(two['value'] - units * 2 / (two['ms_per_step'] * 2e-3)) <= 1e-6 * two['value']
    r = two['roofline']            # rank 0's kernel: half of the slabs
    assert r['frac'] > 0 and r['launches'] >= 2
    _check_rank_records(two, 2, nt_global * 9)


def test_bench_start_up_fails_soft_when_a_rank_cannot_join_rccl():
    """Round-3 verdict W6, on the GPU box: bench.py with two ranks whose native-communicator start-up is rehearsed
    (NF_NATIVE_REDUCE=rehearse) and rank 1's preflight made to fail (NF_TEST_FAIL_COMM=1): nobody enters ncclCommInitRank,
    both ranks fall back to torch.distributed together with the line on stderr, and the totals equal the N=1 run."""
    nt = 3
    two, err = _bench_json(['--nt', str(nt)], nproc=2, with_stderr=True,
                           env_extra={'NF_NATIVE_REDUCE': 'rehearse', 'NF_TEST_FAIL_COMM': '1', 'NF_DIST_TIMEOUT_S': '120'})
    one = _bench_json(['--nt', str(nt)])
    assert 'injected preflight failure on rank 1' in err and 'reducing through torch.distributed' in err
    assert two['reduce']['path'] == 'torch.distributed.all_reduce' and two['n_gpus'] == 2
    a, b = numpy.array(two['totals']), numpy.array(one['totals'])
    assert a.shape == b.shape and numpy.abs(a - b).max() <= 1e-13 * numpy.abs(b).max()
    # without the injected fault the rehearsal stops at the agreement (two ranks on one device cannot form a communicator)
    two, err = _bench_json(['--nt', str(nt)], nproc=2, with_stderr=True, env_extra={'NF_NATIVE_REDUCE': 'rehearse'})
    assert 'rehearsal on the gloo backend' in err and two['reduce']['path'] == 'torch.distributed.all_reduce'


def test_bench_emulates_one_rank_of_n():
    """`bench.py --emulate-rank r/N` (per-rank compute evidence for N > 1 on a one-GPU box): one process takes rank r's slab
    range of the strong-scaling cut, runs its launches without a reduce and says so in the line; the partial rows of all N
    emulated ranks add up to the N = 1 totals."""
    from nemoflux_amd.dist import slab_range
    nt, n = 3, 4
    one = _bench_json(['--nt', str(nt)])
    acc = None
    for r in range(n):
        d = _bench_json(['--nt', str(nt), '--emulate-rank', f'{r}/{n}'])
        e = d['emulated_rank']
        assert (e['rank'], e['of']) == (r, n) and tuple(e['slabs']) == slab_range(nt, 9, r, n)
        assert d['n_gpus'] == 1 and 'EMULATION of rank' in d['config']['workload'] and 'reduce' not in d and 'cpu_baseline' not in d
        assert e['ms_per_pass'] > 0 and e['launches_per_pass'] >= 1
        units = (e['slabs'][1] - e['slabs'][0]) * 144 * 72
        assert abs(d['value'] - units / (d['ms_per_step'] * 1e-3)) <= 1e-6 * d['value']
        t = numpy.array(d['totals'])
        acc = t if acc is None else acc + t
    b = numpy.array(one['totals'])
    assert numpy.abs(acc - b).max() <= 1e-13 * numpy.abs(b).max()


def test_rccl_preflight_is_not_collective():
    """nf_rccl_preflight: librccl resolves and this thread has a device -- answered by one rank on its own."""
    import ctypes
    import torch
    from nemoflux_amd._lib import lib, check
    dev = ctypes.c_int(-1)
    check(lib.nf_rccl_preflight(ctypes.byref(dev)))
    assert dev.value == torch.cuda.current_device()


def _check_rank_records(line, world, slabs):
    """one record per rank: the slab ranges tile [0, slabs), every rank timed its own kernels"""
    recs = line['ranks']
    assert [r['rank'] for r in recs] == list(range(world)) and line['reduce']['world_size'] == world
    assert recs[0]['slabs'][0] == 0 and recs[-1]['slabs'][1] == slabs
    for a, b in zip(recs[:-1], recs[1:]):
        assert a['slabs'][1] == b['slabs'][0]
    for r in recs:
        t0, t1 = r['steps_touched']
        assert r['device_name'] and t1 > t0 and r['launches_per_pass'] >= 1
        assert r['k_flux_ms'] > 0 and r['k3_ms'] > 0


def test_bench_starts_its_own_ranks():
    """plain `python bench.py --gpus 2` (no torchrun): the parent -- which makes no GPU call -- starts two ranks as a fresh
    child torch.distributed.run, relays rank 0's line and exits with the child's code.  Totals equal N=1 to 1e-13."""
    nt = 4
    two = _bench_json(['--nt', str(nt)], nproc=2, launcher='self')
    one = _bench_json(['--nt', str(nt)])
    assert two['n_gpus'] == 2 and two['scaling'] == 'strong' and one['n_gpus'] == 1
    a, b = numpy.array(two['totals']), numpy.array(one['totals'])
    assert a.shape == b.shape == (nt, 7)
    assert numpy.abs(a - b).max() <= 1e-13 * numpy.abs(b).max()
    _check_rank_records(two, 2, nt * 9)
    assert two['reduce']['backend'] == 'gloo' and two['reduce']['path'] == 'torch.distributed.all_reduce'
    assert 'ranks' not in one


def test_native_rccl_reduce_on_one_rank():
    """nf_rccl_unique_id / nf_rccl_comm_init / nf_rows_allreduce / nf_rccl_comm_info / nf_rccl_comm_destroy of the C ABI on
    a one-rank communicator (all this box can run of RCCL), through the same librccl the process already holds."""
    import ctypes
    import torch
    from nemoflux_amd._lib import lib, check
    ident = ctypes.create_string_buffer(128)
    check(lib.nf_rccl_unique_id(ident))
    comm = ctypes.c_void_p()
    check(lib.nf_rccl_comm_init(ctypes.byref(comm), 1, ident, 0))
    n, r, d = ctypes.c_int(-1), ctypes.c_int(-1), ctypes.c_int(-1)
    check(lib.nf_rccl_comm_info(comm, ctypes.byref(n), ctypes.byref(r), ctypes.byref(d)))
    assert (n.value, r.value, d.value) == (1, 0, torch.cuda.current_device())
    rows = torch.arange(24., dtype=torch.float64, device='cuda').reshape(3, 8)
    want = rows.clone()
    s = torch.cuda.Stream()
    with torch.cuda.stream(s):
        check(lib.nf_rows_allreduce(comm, ctypes.c_void_p(rows.data_ptr()), rows.numel(), ctypes.c_void_p(s.cuda_stream)))
    s.synchronize()
    assert torch.equal(rows, want)
    path = ctypes.create_string_buffer(512)
    check(lib.nf_rccl_library(path, 512))
    assert b'librccl' in path.value
    assert lib.nf_rows_allreduce(None, ctypes.c_void_p(rows.data_ptr()), 4, None) != 0     # null communicator: an error
    check(lib.nf_rccl_comm_destroy(comm))
