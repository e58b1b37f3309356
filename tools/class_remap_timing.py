"""Cost of a remapped class step (nf_field_compute_class_remap_async) against the step-rule class step beside it.

For the bench workload (3600 x 1800 x 75, README singular transect + 64 seeded transects), float64 and float32, with 16 and
256 class edges: ms per step (HIP events on the field's stream, medians of --reps with min - max, the two calls alternating in
one process) of every form -- volume, carried tracer that is the class field, carried tracer with a class field of its own --
and of the yardstick: computeClassTransport (volume) / computeClassTracerTransport (carried) at the same edges, window and
dtype, the product the library had before.  The remapping issues the same gathers per level plus two halo levels, so the ratio
is near 1 while a layer stays inside a few classes; with many edges it is set by how many rows a term reaches, which the
reference counts (rows_per_term: the mean over the classed terms with a non-zero volume value).  No bar is set on the ratio.

Also printed: the worst error of one step against tests/class_remap_reference.py relative to sum |share| of the value (bar
1e-12), for the volume form at the first edge count and the widest form at the last (--no-check leaves it out).

    python tools/class_remap_timing.py [--reps N] [--dtype f64|f32] [--classes 16,256] [--no-check] [--json OUT]
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
from gross_timing import timed  # noqa: E402
from joint_class_timing import make_salinity  # noqa: E402
from nemoflux_amd._lib import lib, check  # noqa: E402
from nemoflux_amd.datagen import DataGen, STREAM_FUNCTIONS  # noqa: E402

BAR = 1e-12
FORMS = ('volume', 'carried-one', 'carried-two')


def reference_step(fld, arrays, edges, carry):
    """the reference's rows of step 0, its sum |share| and the mean number of rows a term reaches"""
    from class_remap_reference import ClassRemapReference
    ce, w, sg = fld.getWeights()
    ref = ClassRemapReference(ce, w, sg, fld.arcLengths, fld.thickness, fld._tr_off, fld.nx, fld.ny, reference=0.0, wrap=True,
                              sverdrup=fld.sverdrup)
    cells = torch.from_numpy(ref.cells).cuda()

    def values(name, z, _cells):
        return arrays[name][0, z].reshape(-1)[cells].cpu().numpy()

    want = ref.remap_step(values, edges, tracer=carry, threads=16)
    return want['carried' if carry else 'volume'], want['rows_per_term']


def measure(name, mk_field, u, v, A, B, args):
    res = []
    fld = mk_field(u, v)
    nrec = fld.getWeights()[0].size // 4
    base = dict(case=name, records=int(nrec), row_length=fld._rowlen, reps=args.reps)
    print(json.dumps(base), flush=True)
    for n in args.classes:
        edges = numpy.linspace(1., 29., n)
        out = torch.zeros((n + 2, fld._rowlen), dtype=torch.float64, device='cuda')
        net = torch.zeros((n + 2, fld._rowlen), dtype=torch.float64, device='cuda')
        for form in FORMS:
            # the class field is temperature-like A throughout; carried-two carries the salinity-like B through its classes
            if form == 'carried-two':
                fld.setTracer(B)
                fld.setClassTracer(A)
            else:
                fld.setClassTracer(None)
                fld.setTracer(A)
            fld.setClassEdges(edges)
            carry = form != 'volume'
            arrays = {'uo': u, 'vo': v, 'class': A, 'tracer': B if form == 'carried-two' else A}

            def remap():
                check(lib.nf_field_compute_class_remap_async(ctypes.byref(fld._h), 0, int(carry), ctypes.c_void_p(out.data_ptr())))

            def yardstick():
                fn = lib.nf_field_compute_class_tracer_transport_async if carry else lib.nf_field_compute_class_transport_async
                check(fn(ctypes.byref(fld._h), 0, ctypes.c_void_p(net.data_ptr())))

            keys = ('median', 'min', 'max')
            t_remap, t_yard = (dict(zip(keys, t)) for t in timed([remap, yardstick], args.reps))
            r = dict(base, edges=n, form=form, ms=t_remap, yardstick_ms=t_yard, ratio_to_yardstick=t_remap['median'] / t_yard['median'])
            rows, step = out.cpu().numpy(), net.cpu().numpy()
            total = numpy.abs(step).sum(axis=0)
            r['sum_over_rows_vs_step_rule'] = float((numpy.abs(rows.sum(axis=0) - step.sum(axis=0)) / numpy.where(total > 0, total, 1.)).max())
            if not args.no_check and ((form == 'volume' and n == args.classes[0]) or (form == 'carried-two' and n == args.classes[-1])):
                (w_, m_), r['rows_per_term'] = reference_step(fld, arrays, edges, carry)
                r['worst_error'] = float((numpy.abs(rows - w_) / numpy.where(m_ > 0, m_, 1.0)).max())
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
    if any(x.get('worst_error', 0.) > BAR for x in out):
        sys.exit('class_remap_timing: a check misses its bar (see the lines above)')


if __name__ == '__main__':
    main()
