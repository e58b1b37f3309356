"""Cost of the gross (inflow / outflow) rows (nf_field_compute_gross_profile_async) against the net profiles, in one process.

For the bench workload (3600 x 1800 x 75, README singular transect + 64 seeded transects, nt = 2), float64 and float32, inputs
in HBM; ms per call, HIP events on the handle's stream, median with min and max of --reps repetitions after warm-up, the calls
of one comparison alternating:
  * the four gross forms -- volume or carried tracer, scalar or static per-cell thickness -- with every chunk length built
    for the dtype (the "gross_chunk" knob);
  * their yardsticks: the volume profile (scalar and cell thickness), the tracer profile (scalar) and the area profile with a
    cell thickness (the only net product with the carried form's 4 + 4 + 5 gathers), from --parent-lib, a libnemoflux_amd.so
    built from the parent commit and loaded beside this one, and from this build;
  * for scale, the host loop over getWeights() for one step (tests/gross_reference.py, the values gathered from HBM level by
    level, --threads host threads), float64 only, and the worst |err| / sum |c| of the device rows against it.
Both libraries are driven through the C ABI alone, each with a handle of its own on the same arrays.

    python tools/gross_timing.py [--reps N] [--dtype f64|f32] [--threads N] [--no-host] [--parent-lib FILE] [--out FILE]
"""
import argparse
import ctypes
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests'))

import numpy  # noqa: E402
import torch  # noqa: E402

import bench  # noqa: E402
from nemoflux_amd import _lib  # noqa: E402
from nemoflux_amd.datagen import DataGen  # noqa: E402

NX, NY, NZ, NT = 3600, 1800, 75, 2
CHUNKS = {'float64': (2, 4, 8), 'float32': (4, 8)}
REF = 10.0
FILL = 1.e20
CALLS = ('nf_last_error', 'nf_tuning_set', 'nf_field_new', 'nf_field_del', 'nf_field_set_stream', 'nf_field_set_bounds',
         'nf_field_set_thickness', 'nf_field_set_sverdrup', 'nf_field_set_uv', 'nf_field_add_transect', 'nf_field_build_weights', 'nf_field_row_length',
         'nf_field_set_tracer', 'nf_field_set_tracer_reference', 'nf_field_set_cell_thickness', 'nf_field_num_weights',
         'nf_field_get_weights', 'nf_field_get_arclengths', 'nf_field_compute_profile_async', 'nf_field_compute_tracer_profile_async',
         'nf_field_compute_area_profile_async')


def bind(path):
    """another libnemoflux_amd.so with the signatures of this build's binding for the calls used here"""
    L = ctypes.CDLL(path)
    for name in CALLS:
        fn, mine = getattr(L, name), getattr(_lib.lib, name)
        fn.argtypes, fn.restype = mine.argtypes, mine.restype
    return L


class Handle(object):
    """an nf_field of library L on the shared arrays"""

    def __init__(self, L, a):
        self.L, self.h = L, ctypes.c_void_p()
        self.call('new')
        self.call('set_stream', torch.cuda.current_stream().cuda_stream)
        code = _lib.NF_F32 if a['uo'].dtype == torch.float32 else _lib.NF_F64
        self.call('set_bounds', a['blon'].data_ptr(), a['blat'].data_ptr(), NY, NX, _lib.NF_F64, 1)
        self.call('set_sverdrup', 1)
        self.call('set_thickness', a['th'].ctypes.data_as(_lib.c_double_p), NZ)
        self.call('set_uv', a['uo'].data_ptr(), a['vo'].data_ptr(), NT, code, 1, FILL)
        for xyz in a['lines']:
            self.call('add_transect', xyz.ctypes.data_as(_lib.c_double_p), xyz.shape[0], 0, None)
        self.call('build_weights', 128, 360.)
        self.call('set_tracer', a['tracer'].data_ptr(), NT, code, 1, numpy.nan)
        self.call('set_tracer_reference', REF)
        n = ctypes.c_int()
        self.call('row_length', ctypes.byref(n))
        self.rowlen, self.code = n.value, code

    def call(self, name, *args):
        rc = getattr(self.L, 'nf_field_' + name)(ctypes.byref(self.h), *args)
        if rc != 0:
            raise RuntimeError(f'nf_field_{name}: {self.L.nf_last_error().decode()}')

    def cell_thickness(self, a, on):
        if on:
            self.call('set_cell_thickness', a['e3u'].data_ptr(), a['e3v'].data_ptr(), 1, self.code, 1, numpy.nan)
        else:
            self.call('set_cell_thickness', None, None, 0, _lib.NF_F64, 0, numpy.nan)

    def weights(self):
        n = ctypes.c_size_t()
        self.call('num_weights', ctypes.byref(n))
        ce, w, sg = numpy.empty(n.value, numpy.int64), numpy.empty(n.value, numpy.float64), numpy.empty(n.value, numpy.int32)
        self.call('get_weights', ce.ctypes.data_as(_lib.c_int64_p), w.ctypes.data_as(_lib.c_double_p), sg.ctypes.data_as(_lib.c_int_p))
        return ce, w, sg


def timed(calls, reps, warm=3):
    """median, min, max ms of every call of `calls`, their repetitions alternating"""
    stream = torch.cuda.current_stream()
    for _ in range(warm):
        for call in calls:
            call()
    torch.cuda.synchronize()
    ev = [[(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in calls] for _ in range(reps)]
    for row in ev:
        for (a, b), call in zip(row, calls):
            a.record(stream)
            call()
            b.record(stream)
    torch.cuda.synchronize()
    out = []
    for k in range(len(calls)):
        ms = sorted(row[k][0].elapsed_time(row[k][1]) for row in ev)
        out.append((ms[len(ms) // 2], ms[0], ms[-1]))
    return out


def fmt(t):
    return f'{t[0]:8.3f} ms ({t[1]:.3f} - {t[2]:.3f})'


def inputs(real):
    dg = DataGen(real=real)
    dg.setSizes(NX, NY, NZ, 1)
    dg.setBoundingBox(-180., 180., -90., 90., 0., 1.)
    dg.build()
    dt = torch.float32 if real == 'float32' else torch.float64
    gen = torch.Generator(device='cuda')
    gen.manual_seed(20261017)
    a = {}
    for name in ('uo', 'vo'):       # magnitudes in [0.01, 1], either sign, a tenth exactly 0, a land block
        x = torch.empty((NT, NZ, NY, NX), dtype=dt, device='cuda')
        for t in range(NT):
            mag = 0.0101 + (1. - 0.0101) * torch.rand((NZ, NY, NX), dtype=torch.float32, device='cuda', generator=gen)
            pick = torch.rand((NZ, NY, NX), dtype=torch.float32, device='cuda', generator=gen)
            x[t] = torch.where(pick < 0.1, torch.zeros_like(mag), torch.where(pick < 0.55, mag, -mag)).to(dt)
            del mag, pick
        x[:, 20:, 400:650, 2000:2901] = FILL
        a[name] = x
    db = numpy.asarray(dg.deptht_bounds, dtype=numpy.float64)
    a['th'] = numpy.ascontiguousarray(db[:, 1] - db[:, 0])
    th = torch.from_numpy(a['th']).cuda()[None, :, None, None]
    f = 0.5 + 0.5 * torch.rand((1, NZ, NY, NX), generator=gen, dtype=torch.float32, device='cuda')
    a['e3u'], a['e3v'] = (th * f).to(dt).contiguous(), (th * (1.5 - f)).to(dt).contiguous()
    del f
    lat = torch.linspace(-89.95, 89.95, NY, dtype=torch.float64, device='cuda')
    z = torch.arange(NZ, dtype=torch.float64, device='cuda')
    base = 2. + 26. * torch.cos(torch.deg2rad(lat))[None, :, None] * torch.exp(-z / 25.)[:, None, None]
    a['tracer'] = (base[None] + 1.5 * torch.rand((NT, NZ, NY, NX), generator=gen, dtype=torch.float32, device='cuda')).to(dt).contiguous()
    a['blon'] = torch.as_tensor(dg.bounds_lon, dtype=torch.float64, device='cuda').contiguous()
    a['blat'] = torch.as_tensor(dg.bounds_lat, dtype=torch.float64, device='cuda').contiguous()
    polys = bench.make_transects(NX, NY, -180., 180., -90., 90., 64)
    a['lines'] = [numpy.ascontiguousarray([(x, y, 0.) for x, y in p], dtype=numpy.float64) for p in polys]
    torch.cuda.synchronize()
    return a


def measure(real, args, say, parent):
    a = inputs(real)
    libs = [('this build', Handle(_lib.lib, a))] + ([('parent', Handle(parent, a))] if parent is not None else [])
    me = libs[0][1]
    nrec = me.weights()[0].size // 4
    say(f'== bench {NX} x {NY} x {NZ} {real}, nt = {NT}, {len(a["lines"])} transects, {nrec} records, row length {me.rowlen}; '
        f'medians of {args.reps} (min - max), ms per call')
    rows = torch.zeros((2, NZ, me.rowlen), dtype=torch.float64, device='cuda')
    p_rows = ctypes.c_void_p(rows.data_ptr())

    def net(h, name):
        return lambda: h.call(name + '_async', 0, p_rows)

    def gross(carry):
        return lambda: me.call('compute_gross_profile_async', 0, carry, p_rows)

    yard = {}
    for ct in (False, True):
        for _, h in libs:
            h.cell_thickness(a, ct)
        kinds = [('volume', 'compute_profile'), ('carried', 'compute_area_profile' if ct else 'compute_tracer_profile')]
        t = timed([net(h, name) for _, name in kinds for _, h in libs], args.reps)
        for k, (form, name) in enumerate(kinds):
            for j, (tag, _) in enumerate(libs):
                yard[form, ct, tag] = t[k * len(libs) + j]
                say(f'yardstick  nf_field_{name:<22s} {"cell thickness  " if ct else "scalar thickness"}  {tag:<10s} '
                    f'{fmt(yard[form, ct, tag])}')
        ytag = libs[-1][0]
        for carry, form in ((0, 'volume'), (1, 'carried')):
            y = yard[form, ct, ytag][0]
            for chunk in CHUNKS[real]:
                assert _lib.lib.nf_tuning_set(b'gross_chunk', chunk) == 0
                g, y2 = timed([gross(carry), net(libs[-1][1], dict(kinds)[form])], args.reps)
                say(f'gross      {form:<8s} {"cell thickness  " if ct else "scalar thickness"}  {chunk} levels per chunk   {fmt(g)}   = '
                    f'{g[0] / y2[0]:.2f} x its yardstick of the {ytag} alternating with it ({y2[0]:.3f} ms; bar 2.00)')
            assert _lib.lib.nf_tuning_set(b'gross_chunk', 0) == 0
            g, y2 = timed([gross(carry), net(libs[-1][1], dict(kinds)[form])], args.reps)
            say(f'gross      {form:<8s} {"cell thickness  " if ct else "scalar thickness"}  DEFAULT chunk        {fmt(g)}   = '
                f'{g[0] / y2[0]:.2f} x its yardstick ({y2[0]:.3f} ms; first pass {y:.3f} ms); bar 2.00: '
                f'{"met" if g[0] < 2. * y2[0] else "MISSED"}')
    for _, h in libs:
        h.cell_thickness(a, False)
    if real == 'float64' and not args.no_host:
        from gross_reference import GrossReference
        arc = numpy.zeros((NY * NX, 4))
        me.call('get_arclengths', arc.ctypes.data_as(_lib.c_double_p))
        ce, w, sg = me.weights()
        tr_off = numpy.concatenate([[0], numpy.cumsum([len(x) - 1 for x in a['lines']])])
        t0 = time.time()
        ref = GrossReference(ce, w, sg, arc, a['th'], tr_off, NX, NY, uv_markers=(FILL,), reference=REF, wrap=True, sverdrup=True)
        cells = torch.from_numpy(ref.cells).cuda()
        t1 = time.time()
        want = ref.gross_step(lambda name, zz, c: a[name][0, zz].reshape(-1)[cells].cpu().numpy(), threads=args.threads)
        t2 = time.time()
        worst = {}
        for carry, form in ((0, 'volume'), (1, 'carried')):
            gross(carry)()
            torch.cuda.synchronize()
            got = rows.cpu().numpy()
            worst[form] = float((numpy.abs(got - want[form][0]) / numpy.maximum(want[form][1], 1e-300)).max())
        one = timed([gross(0), gross(1)], args.reps)
        say(f'host loop over getWeights() for one step, both forms (numpy, {args.threads} threads): setup {t1 - t0:.1f} s + step '
            f'{t2 - t1:.1f} s = {(t2 - t0) * 1e3 / (one[0][0] + one[1][0]):.0f} x the two gross calls ({one[0][0] + one[1][0]:.3f} ms); '
            f'worst |err| / sum |c| against it: volume {worst["volume"]:.3g}, carried {worst["carried"]:.3g}; '
            f'smallest non-zero |q| {want["min_abs_q"]:.3g}')
    for _, h in libs:
        h.call('del')
    del a
    torch.cuda.empty_cache()


def main():
    ap = argparse.ArgumentParser(description=__doc__.split('\n')[0])
    ap.add_argument('--reps', type=int, default=10)
    ap.add_argument('--dtype', choices=['f64', 'f32'], default=None)
    ap.add_argument('--threads', type=int, default=12)
    ap.add_argument('--no-host', dest='no_host', action='store_true', help='skip the host loop')
    ap.add_argument('--parent-lib', dest='parent_lib', default='', help='libnemoflux_amd.so built from the parent commit')
    ap.add_argument('--out', default='', help='also append the lines to this file')
    args = ap.parse_args()
    parent = bind(args.parent_lib) if args.parent_lib else None

    def say(line):
        print(line, flush=True)
        if args.out:
            with open(args.out, 'a') as fh:
                fh.write(line + '\n')
    if parent is None:
        say('no --parent-lib: the yardsticks are the net profiles of this build')
    for dt, real in (('f64', 'float64'), ('f32', 'float32')):
        if args.dtype and dt != args.dtype:
            continue
        measure(real, args, say, parent)


if __name__ == '__main__':
    main()
