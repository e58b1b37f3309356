"""Cost of a remapped gross class step (nf_field_compute_gross_class_remap_async) against the net remapped step beside it.

For the bench workload (3600 x 1800 x 75, README singular transect + 64 seeded transects), float64 and float32, with 16 and
256 class edges: ms per step (HIP events on the field's stream, medians of --reps with min - max, everything in one process)
of every form -- volume, carried tracer that is the class field, carried tracer with a class field of its own, each with the
scalar and with a per-cell thickness -- and, measured in the same process at the same edges and dtype: the yardstick,
computeClassRemap (one pass over the fields per window of rows, where the gross form makes one per part and window: about 2 x
is what to expect), and computeGrossClassTransport, the step rule's gross form, with both thicknesses.  The ratio to the yardstick
is printed next to the spread of the yardstick's own repeats, (max - min) / median: that spread is the margin of the ratio.  The
cell-thickness forms have no net remap to compare with: their ratio to the scalar form is printed beside the same ratio of
computeGrossClassTransport.

Also printed: the worst error of one step against tests/gross_remap_reference.py relative to sum |share| of the value (bar
1e-12), every value of P and N, for the volume form with the scalar thickness and for the widest form with the cell thickness
(--no-check leaves it out).

    python tools/gross_remap_timing.py [--reps N] [--dtype f64|f32] [--classes 16,256] [--no-check] [--json OUT]
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
from gross_class_timing import FORMS, make_thickness  # noqa: E402
from joint_class_timing import make_salinity, stats, timed  # noqa: E402
from nemoflux_amd._lib import lib, check  # noqa: E402
from nemoflux_amd.datagen import DataGen, STREAM_FUNCTIONS  # noqa: E402

BAR = 1e-12


def worst_error(fld, arrays, edges, carry, cell, rows):
    """max |rows - reference| / sum |share| of one step over every value of P and N, and the smallest non-zero |q|"""
    from gross_remap_reference import GrossRemapReference
    ce, w, sg = fld.getWeights()
    ref = GrossRemapReference(ce, w, sg, fld.arcLengths, fld.thickness, fld._tr_off, fld.nx, fld.ny, reference=0.0, wrap=True,
                              sverdrup=fld.sverdrup, cell_thickness=cell)
    cells = torch.from_numpy(ref.cells).cuda()
    cache = {}

    def values(name, z, _cells):
        if (name, z) not in cache:      # a level of the class field is asked for by three levels
            cache[name, z] = arrays[name][0, z].reshape(-1)[cells].cpu().numpy()
        return cache[name, z]

    want = ref.gross_remap_step(values, edges, tracer=carry, threads=16)
    w_, m_ = want['carried' if carry else 'volume']
    return float((numpy.abs(rows - w_) / numpy.where(m_ > 0, m_, 1.0)).max()), want['min_abs_q'], want['spread_terms']


def measure(name, mk_field, u, v, A, B, args):
    res = []
    fld = mk_field(u, v)
    e3 = make_thickness(u, fld.thickness)
    nrec = fld.getWeights()[0].size // 4
    base = dict(case=name, records=int(nrec), row_length=fld._rowlen, reps=args.reps)
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
            dst = ctypes.c_void_p(out.data_ptr())

            def remap():
                check(lib.nf_field_compute_gross_class_remap_async(ctypes.byref(fld._h), 0, int(carry), dst))

            def step_rule():
                check(lib.nf_field_compute_gross_class_transport_async(ctypes.byref(fld._h), 0, int(carry), dst))

            def yardstick():
                check(lib.nf_field_compute_class_remap_async(ctypes.byref(fld._h), 0, int(carry), ctypes.c_void_p(net.data_ptr())))

            r = dict(base, edges=n, rows=2 * nrows, form=form)
            yard = stats(timed(yardstick, args.reps))
            net_rows = net.cpu().numpy().copy()
            step = stats(timed(step_rule, args.reps))
            scalar = stats(timed(remap, args.reps))
            rows = out.cpu().numpy().reshape(2, nrows, -1).copy()
            if not carry:       # volume form: P - N is sum |share| of both parts
                mag = rows[0] - rows[1]
                r['p_plus_n_vs_net'] = float((numpy.abs(rows[0] + rows[1] - net_rows) / numpy.where(mag > 0, mag, 1.0)).max())
            r.update(ms=scalar, yardstick_ms=yard, ratio_to_yardstick=scalar['median'] / yard['median'],
                     yardstick_spread=(yard['max'] - yard['min']) / yard['median'], step_rule_ms=step)
            if not args.no_check and form == 'volume' and n == args.classes[0]:
                r['worst_error'], r['min_abs_q'], r['spread_terms'] = worst_error(fld, arrays, edges, carry, False, rows)
            fld.setCellThickness(*e3)
            cell = stats(timed(remap, args.reps))
            rows = out.cpu().numpy().reshape(2, nrows, -1).copy()
            step_cell = stats(timed(step_rule, args.reps))
            r.update(cell_ms=cell, cell_to_scalar=cell['median'] / scalar['median'], step_rule_cell_ms=step_cell,
                     step_rule_cell_to_scalar=step_cell['median'] / step['median'])
            if not args.no_check and form == 'carried-two' and n == args.classes[0]:
                r['cell_worst_error'], r['cell_min_abs_q'], r['cell_spread_terms'] = worst_error(fld, arrays, edges, carry, True, rows)
            print(json.dumps(r), flush=True)
            res.append(r)
        del out, net
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
    if any(e > BAR for e in errs):
        sys.exit('gross_remap_timing: a check misses its bar (see the lines above)')


if __name__ == '__main__':
    main()
