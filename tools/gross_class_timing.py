"""Cost of a gross class step (nf_field_compute_gross_class_transport_async) against the net class step beside it.

For the bench workload (3600 x 1800 x 75, README singular transect + 64 seeded transects), float64 and float32, with 16 and
256 class edges: ms per step (HIP events on the field's stream, medians of --reps with min - max, everything in one process)
of every form -- volume, carried tracer that is the class field, carried tracer with a class field of its own, each with the
scalar and with a per-cell thickness -- and of the yardstick measured in the same process: computeClassTransport (volume) /
computeClassTracerTransport (carried) at the same edges and dtype.  The bar is 2 x the yardstick, the two sign-masked class
passes that a gross class step replaces; the cell-thickness forms have no net form to compare with, so their ratio to the
scalar form is printed next to the ratio of the bytes gathered per level.

Stage split: the call is one gather launch (stage 1) and one binning launch plus the finalize per window of 32 rows (stage 2);
with the block skip off every window costs the same, so the two edge counts (2 and 17 windows) give stage 1 and the per-window
cost as the intercept and the slope of a line -- an estimate, printed as such.  Also printed: the size of the term table, and
the worst error of one step against tests/gross_class_reference.py relative to sum |c| of the value (bar 1e-12), for the
volume form with the scalar thickness and for the widest form (--no-check leaves it out).

    python tools/gross_class_timing.py [--reps N] [--dtype f64|f32] [--classes 16,256] [--no-check] [--json OUT]
"""
import argparse
import ctypes
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tools'))
sys.path.insert(0, os.path.join(ROOT, 'tests'))

import numpy  # noqa: E402
import torch  # noqa: E402

import bench  # noqa: E402
import class_timing  # noqa: E402
from joint_class_timing import make_salinity, stats, timed  # noqa: E402
from nemoflux_amd._lib import lib, check  # noqa: E402
from nemoflux_amd.datagen import DataGen, STREAM_FUNCTIONS  # noqa: E402

BAR = 1e-12
WINDOW = 32     # nf_tuning_set("joint_window") default
FORMS = ('volume', 'carried-one', 'carried-two')
GATHERS = {'volume': 4 + 5, 'carried-one': 4 + 5, 'carried-two': 4 + 5 + 5}      # per level, scalar thickness; + 4 with cells


def make_thickness(u, thickness):
    """e3u, e3v of the dtype of uo: the level's thickness times a factor in [0.8, 1.2) per cell"""
    gen = torch.Generator(device='cuda')
    gen.manual_seed(20261018)
    th = torch.from_numpy(numpy.asarray(thickness, dtype=numpy.float64)).cuda()[None, :, None, None]
    return [(th * (0.8 + 0.4 * torch.rand(tuple(u.shape), generator=gen, dtype=torch.float64, device='cuda'))).to(u.dtype).contiguous()
            for _ in range(2)]


def worst_error(fld, arrays, edges, carry, cell, rows):
    """max |rows - reference| / sum |c| of one step, and the smallest non-zero |q|"""
    from gross_class_reference import GrossClassReference
    ce, w, sg = fld.getWeights()
    ref = GrossClassReference(ce, w, sg, fld.arcLengths, fld.thickness, fld._tr_off, fld.nx, fld.ny, reference=0.0, wrap=True,
                              sverdrup=fld.sverdrup, cell_thickness=cell)
    cells = torch.from_numpy(ref.cells).cuda()

    def values(name, z, _cells):
        return arrays[name][0, z].reshape(-1)[cells].cpu().numpy()

    want = ref.gross_class_step(values, edges, tracer=carry, threads=16)
    w_, m_ = want['carried' if carry else 'volume']
    return float((numpy.abs(rows - w_) / numpy.where(m_ > 0, m_, 1.0)).max()), want['min_abs_q']


def measure(name, mk_field, u, v, A, B, args):
    res = []
    fld = mk_field(u, v)
    e3 = make_thickness(u, fld.thickness)
    nrec = fld.getWeights()[0].size // 4
    base = dict(case=name, records=int(nrec), row_length=fld._rowlen, table_GB=40 * nrec * fld.nz / 1e9, reps=args.reps)
    print(json.dumps(base), flush=True)
    for n in args.classes:
        edges = numpy.linspace(1., 29., n)
        nrows = n + 2
        out = torch.zeros((2 * nrows, fld._rowlen), dtype=torch.float64, device='cuda')
        net = torch.zeros((nrows, fld._rowlen), dtype=torch.float64, device='cuda')
        for form in FORMS:
            # the class field is temperature-like A throughout; carried-two carries the salinity-like B through its classes
            fld.setCellThickness(None, None)
            if form == 'carried-two':
                fld.setTracer(B)
                fld.setClassTracer(A)
            else:
                fld.setClassTracer(None)
                fld.setTracer(A)
            fld.setClassEdges(edges)
            carry = form != 'volume'
            arrays = {'uo': u, 'vo': v, 'class': A, 'tracer': B if form == 'carried-two' else A, 'e3u': e3[0], 'e3v': e3[1]}

            def gross():
                check(lib.nf_field_compute_gross_class_transport_async(ctypes.byref(fld._h), 0, int(carry),
                                                                       ctypes.c_void_p(out.data_ptr())))

            def yardstick():
                fn = lib.nf_field_compute_class_tracer_transport_async if carry else lib.nf_field_compute_class_transport_async
                check(fn(ctypes.byref(fld._h), 0, ctypes.c_void_p(net.data_ptr())))

            r = dict(base, edges=n, rows=2 * nrows, windows=-(-2 * nrows // WINDOW), form=form)
            yard = stats(timed(yardstick, args.reps))
            net_rows = net.cpu().numpy().copy()
            scalar = stats(timed(gross, args.reps))
            rows = out.cpu().numpy().reshape(2, nrows, -1).copy()
            mag = rows[0] - rows[1] if not carry else None
            if mag is not None:     # volume form: P - N is sum |c| of both parts
                r['p_plus_n_vs_net'] = float((numpy.abs(rows[0] + rows[1] - net_rows) / numpy.where(mag > 0, mag, 1.0)).max())
            check(lib.nf_tuning_set(b'joint_skip', 0))
            r['ms_skip_off'] = stats(timed(gross, args.reps))
            check(lib.nf_tuning_set(b'joint_skip', 1))
            r.update(ms=scalar, yardstick_ms=yard, ratio_to_yardstick=scalar['median'] / yard['median'],
                     within_two_yardsticks=bool(scalar['median'] <= 2. * yard['median']))
            if not args.no_check and form == 'volume' and n == args.classes[0]:
                r['worst_error'], r['min_abs_q'] = worst_error(fld, arrays, edges, carry, False, rows)
            fld.setCellThickness(*e3)
            cell = stats(timed(gross, args.reps))
            r.update(cell_ms=cell, cell_to_scalar=cell['median'] / scalar['median'],
                     cell_to_scalar_gathers=(GATHERS[form] + 4) / GATHERS[form])
            if not args.no_check and form == 'carried-two' and n == args.classes[0]:
                rows = out.cpu().numpy().reshape(2, nrows, -1)
                r['cell_worst_error'], r['cell_min_abs_q'] = worst_error(fld, arrays, edges, carry, True, rows)
            print(json.dumps(r), flush=True)
            res.append(r)
        del out, net
    vol = [x for x in res if x['form'] == 'volume']
    if len(vol) == 2:   # stage 1 and the per-window cost of stage 2, skip off: the intercept and the slope over the windows
        (w0, t0), (w1, t1) = [(x['windows'], x['ms_skip_off']['median']) for x in vol]
        per_window = (t1 - t0) / (w1 - w0)
        est = dict(case=name, estimate='volume form, skip off: T = stage1 + windows * stage2', stage2_ms_per_window=per_window,
                   stage1_ms=t0 - w0 * per_window)
        print(json.dumps(est), flush=True)
        res.append(est)
    return res


def bench_case(real, args):
    nx, ny, nz = 3600, 1800, 75
    dg = DataGen(real=real)
    dg.setSizes(nx, ny, nz, 1)
    dg.setBoundingBox(-180., 180., -90., 90., 0., 1.)
    dg.build()
    dg.applyStreamFunction(STREAM_FUNCTIONS[5])
    u, v = dg.computeUVFromPotential()
    polys = bench.make_transects(nx, ny, -180., 180., -90., 90., 64)
    xyzs = [numpy.array([(x, y, 0.) for x, y in p]) for p in polys]
    A = class_timing.make_tracer(u, ny, nz, -89.95, 89.95)
    B = make_salinity(u, nx, nz)
    r = measure(f'bench {nx}x{ny}x{nz} {real}, {len(xyzs)} transects', class_timing.field_maker(dg, xyzs), u, v, A, B, args)
    del u, v, A, B, dg
    torch.cuda.empty_cache()
    return r


def main():
    ap = argparse.ArgumentParser(description=__doc__.split('\n')[0])
    ap.add_argument('--reps', type=int, default=10)
    ap.add_argument('--dtype', choices=['f64', 'f32'], default=None)
    ap.add_argument('--classes', default='16,256')
    ap.add_argument('--json', default='')
    ap.add_argument('--no-check', dest='no_check', action='store_true', help='leave the comparison with the reference out')
    args = ap.parse_args()
    args.classes = [int(x) for x in args.classes.split(',') if x]
    out = []
    for dt, real in (('f64', 'float64'), ('f32', 'float32')):
        if args.dtype and dt != args.dtype:
            continue
        out += bench_case(real, args)
        if args.json:       # written as it goes: a later case that runs out of time keeps the earlier ones
            with open(args.json, 'w') as f:
                json.dump(out, f, indent=1)
    errs = [x[k] for x in out for k in ('worst_error', 'cell_worst_error', 'p_plus_n_vs_net') if k in x]
    big = [x for x in out if x.get('edges', 0) >= 256 and not x['within_two_yardsticks']]
    if big or any(e > BAR for e in errs):
        sys.exit('gross_class_timing: a form at 256 edges costs more than two net class steps, or a check misses its bar (see '
                 'the lines above)')


if __name__ == '__main__':
    main()
