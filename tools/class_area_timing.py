"""Cost of a class area step (nf_field_compute_class_area_async) against the two gross class steps it replaces.

Before this call the section area in classes took uo / vo replaced by 1 and two calls of computeGrossClassTransport, carry=False
and carry=True, with P - N of each as the area rows and the tracer rows.  For the bench workload (3600 x 1800 x 75, README
singular transect + 64 seeded transects), float64 and float32, with 16 and 256 class edges: ms per step (HIP events on the
field's stream, medians of --reps with min - max, everything in one process) of every form -- the tracer binned by itself, a
class field of its own, each with the scalar and with a per-cell thickness -- and of the yardstick measured in the same
process: the sum of the medians of the two gross class calls at the same edges, dtype, tracers and thickness form.  The bar is
1 x the yardstick, no margin.

Stage split: the call is one gather launch (stage 1) and one binning launch plus the finalize per window of 32 rows (stage 2);
with the block skip off every window costs the same, so the two edge counts (2 and 17 windows) give stage 1 and the per-window
cost as the intercept and the slope of a line -- an estimate, printed as such.  Also printed: the size of the term table, and
the worst error of one step against tests/class_area_reference.py relative to the sum of |terms| of the value (bar 1e-12), for
the one-tracer form with the scalar thickness and for the widest form (--no-check leaves it out).

    python tools/class_area_timing.py [--reps N] [--dtype f64|f32] [--classes 16,256] [--no-check] [--json OUT]
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
from gross_class_timing import make_thickness  # noqa: E402
from joint_class_timing import make_salinity, stats, timed  # noqa: E402
from nemoflux_amd._lib import lib, check  # noqa: E402
from nemoflux_amd.datagen import DataGen, STREAM_FUNCTIONS  # noqa: E402

BAR = 1e-12
WINDOW = 32     # nf_tuning_set("joint_window") default
FORMS = ('one-tracer', 'class-tracer')


def worst_error(fld, arrays, edges, cell, rows):
    """max |rows - reference| / sum |terms| of one step"""
    from class_area_reference import ClassAreaReference
    ce, w, sg = fld.getWeights()
    ref = ClassAreaReference(ce, w, sg, fld.arcLengths, fld.thickness, fld._tr_off, fld.nx, fld.ny, reference=0.0, wrap=True,
                             cell_thickness=cell)
    cells = torch.from_numpy(ref.cells).cuda()

    def values(name, z, _cells):
        return arrays[name][0, z].reshape(-1)[cells].cpu().numpy()

    want, mag = ref.class_area_step(values, edges, threads=16)
    return float((numpy.abs(rows - want) / numpy.where(mag > 0, mag, 1.0)).max())


def measure(name, mk_field, u, v, A, B, args):
    res = []
    fld = mk_field(u, v)
    e3 = make_thickness(u, fld.thickness)
    nrec = fld.getWeights()[0].size // 4
    base = dict(case=name, records=int(nrec), row_length=fld._rowlen, table_GB=80 * nrec * fld.nz / 1e9, reps=args.reps)
    print(json.dumps(base), flush=True)
    for n in args.classes:
        edges = numpy.linspace(1., 29., n)
        nrows = n + 2
        out = torch.zeros((2 * nrows, fld._rowlen), dtype=torch.float64, device='cuda')
        pn = torch.zeros((2 * nrows, fld._rowlen), dtype=torch.float64, device='cuda')
        for form in FORMS:
            # the class field is temperature-like A throughout; class-tracer carries the salinity-like B through its classes
            if form == 'class-tracer':
                fld.setTracer(B)
                fld.setClassTracer(A)
            else:
                fld.setClassTracer(None)
                fld.setTracer(A)
            fld.setClassEdges(edges)
            arrays = {'uo': u, 'vo': v, 'class': A, 'tracer': B if form == 'class-tracer' else A, 'e3u': e3[0], 'e3v': e3[1]}

            def area():
                check(lib.nf_field_compute_class_area_async(ctypes.byref(fld._h), 0, ctypes.c_void_p(out.data_ptr())))

            def gross(carry):
                def call():
                    check(lib.nf_field_compute_gross_class_transport_async(ctypes.byref(fld._h), 0, carry,
                                                                           ctypes.c_void_p(pn.data_ptr())))
                return call

            r = dict(base, edges=n, rows=2 * nrows, windows=-(-2 * nrows // WINDOW), form=form)
            for cell in (False, True):
                fld.setCellThickness(*(e3 if cell else (None, None)))
                key = 'cell_' if cell else ''
                vol, car = stats(timed(gross(0), args.reps)), stats(timed(gross(1), args.reps))
                mine = stats(timed(area, args.reps))
                yard = vol['median'] + car['median']
                r.update({key + 'ms': mine, key + 'gross_volume_ms': vol, key + 'gross_carried_ms': car,
                          key + 'yardstick_ms': yard, key + 'ratio_to_yardstick': mine['median'] / yard,
                          key + 'within_yardstick': bool(mine['median'] <= yard)})
                if not cell:
                    check(lib.nf_tuning_set(b'joint_skip', 0))
                    r['ms_skip_off'] = stats(timed(area, args.reps))
                    check(lib.nf_tuning_set(b'joint_skip', 1))
                    area()
                checked = (form == 'one-tracer' and not cell) or (form == 'class-tracer' and cell)
                if not args.no_check and checked and n == args.classes[0]:
                    torch.cuda.synchronize()
                    rows = out.cpu().numpy().reshape(2, nrows, -1)
                    r[key + 'worst_error'] = worst_error(fld, arrays, edges, cell, rows)
            fld.setCellThickness(None, None)
            print(json.dumps(r), flush=True)
            res.append(r)
        del out, pn
    one = [x for x in res if x['form'] == 'one-tracer']
    if len(one) == 2:   # stage 1 and the per-window cost of stage 2, skip off: the intercept and the slope over the windows
        (w0, t0), (w1, t1) = [(x['windows'], x['ms_skip_off']['median']) for x in one]
        per_window = (t1 - t0) / (w1 - w0)
        est = dict(case=name, estimate='one-tracer form, skip off: T = stage1 + windows * stage2', stage2_ms_per_window=per_window,
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
    errs = [x[k] for x in out for k in ('worst_error', 'cell_worst_error') if k in x]
    slow = [x for x in out if x.get('within_yardstick') is False or x.get('cell_within_yardstick') is False]
    if slow or any(e > BAR for e in errs):
        sys.exit('class_area_timing: a form costs more than the two gross class steps it replaces, or a check misses its bar '
                 '(see the lines above)')


if __name__ == '__main__':
    main()
