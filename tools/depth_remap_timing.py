"""Cost of a step of the transports in depth bins (nf_field_compute_depth_transport_async) against the profile step beside it.

For the bench workload (3600 x 1800 x 75, README singular transect + 64 seeded transects), float64 and float32, with 16 and 75
depth edges, with the per-level thickness and with a per-cell thickness (the nominal one times a partial-cell factor in
[0.5, 1]): ms per step (HIP events on the field's stream, medians of --reps with min - max, the calls alternating in one
process) of the volume and the carried form, and of the yardstick: computeFluxProfile under the same thickness at the same
dtype, the product the library had before.  The depth kernel makes one pass over the fields per window of 32 rows and every
pass issues the profile's gathers, so the yardstick is multiplied by the number of passes, ceil((n + 2) / 32); the target is
at most 1.5 x that product (the margin is for the spread into the LDS rows).  `ratio_to_target_base` is ms / (passes x
yardstick): <= 1.5 meets the target.  The carried form has the tracer profile as its yardstick where that call exists (no
cell thickness); with a cell thickness it is reported without one.  `sum_over_rows_vs_profile` is the largest difference
between the sum over the rows and the sum over z of the yardstick's rows, relative to the sum over z of |yardstick row| -- not
to sum |terms|: where the rows of a closed transect are rounding noise (the volume form of a flow with a stream function under
the per-level thickness) it means nothing.

Also printed: the worst error of one step against tests/depth_remap_reference.py relative to sum |share| of the value (bar
1e-12), for the volume form at the first edge count and the carried form at the last, both with the per-cell thickness
(--no-check leaves it out).

    python tools/depth_remap_timing.py [--reps N] [--dtype f64|f32] [--edges 16,75] [--no-check] [--json OUT]
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
from nemoflux_amd._lib import lib, check  # noqa: E402
from nemoflux_amd.datagen import DataGen, STREAM_FUNCTIONS  # noqa: E402

BAR = 1e-12
TARGET = 1.5
WINDOW = 32


def reference_step(fld, arrays, edges, carry, cell):
    """the reference's rows of step 0 and their sum |share|, and how many terms were spread over more than one row"""
    from depth_remap_reference import DepthRemapReference
    ce, w, sg = fld.getWeights()
    ref = DepthRemapReference(ce, w, sg, fld.arcLengths, fld.thickness, fld._tr_off, fld.nx, fld.ny, reference=0.0, wrap=True,
                              sverdrup=fld.sverdrup, cell_thickness=cell)
    cells = torch.from_numpy(ref.cells).cuda()

    def values(name, z, _cells):
        return arrays[name][0, z].reshape(-1)[cells].cpu().numpy()

    want = ref.depth_step(values, edges, tracer=carry, threads=16)
    return want['carried' if carry else 'volume'], want['spread_terms']


def measure(name, mk_field, u, v, A, e3, zmax, args):
    res = []
    fld = mk_field(u, v)
    fld.setTracer(A)
    nrec = fld.getWeights()[0].size // 4
    base = dict(case=name, records=int(nrec), row_length=fld._rowlen, reps=args.reps)
    print(json.dumps(base), flush=True)
    prof = torch.zeros((fld.nz, fld._rowlen), dtype=torch.float64, device='cuda')
    keys = ('median', 'min', 'max')
    for cell in (False, True):
        fld.setCellThickness(*(e3 if cell else (None, None)))
        arrays = {'uo': u, 'vo': v, 'tracer': A, 'e3u': e3[0], 'e3v': e3[1]}
        for n in args.edges:
            edges = numpy.linspace(0., zmax, n)
            fld.setDepthEdges(edges)
            passes = -(-(n + 2) // WINDOW)
            out = torch.zeros((n + 2, fld._rowlen), dtype=torch.float64, device='cuda')
            for carry in (False, True):
                def depth():
                    check(lib.nf_field_compute_depth_transport_async(ctypes.byref(fld._h), 0, int(carry), ctypes.c_void_p(out.data_ptr())))

                def yardstick():
                    fn = lib.nf_field_compute_tracer_profile_async if carry else lib.nf_field_compute_profile_async
                    check(fn(ctypes.byref(fld._h), 0, ctypes.c_void_p(prof.data_ptr())))

                has_yard = not (carry and cell)            # the tracer profile takes no cell thickness
                t = [dict(zip(keys, x)) for x in timed([depth, yardstick] if has_yard else [depth], args.reps)]
                r = dict(base, edges=n, passes=passes, thickness='cell' if cell else 'scalar', form='carried' if carry else 'volume',
                         ms=t[0])
                rows = out.cpu().numpy()
                if has_yard:
                    r['yardstick_ms'] = t[1]
                    r['ratio_to_target_base'] = t[0]['median'] / (passes * t[1]['median'])
                    r['meets_target'] = bool(r['ratio_to_target_base'] <= TARGET)
                    level = prof.cpu().numpy()
                    total = numpy.abs(level).sum(axis=0)
                    r['sum_over_rows_vs_profile'] = float((numpy.abs(rows.sum(axis=0) - level.sum(axis=0)) /
                                                           numpy.where(total > 0, total, 1.)).max())
                if not args.no_check and cell and ((not carry and n == args.edges[0]) or (carry and n == args.edges[-1])):
                    (w_, m_), r['spread_terms'] = reference_step(fld, arrays, edges, carry, cell)
                    r['worst_error'] = float((numpy.abs(rows - w_) / numpy.where(m_ > 0, m_, 1.0)).max())
                print(json.dumps(r), flush=True)
                res.append(r)
            del out
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
    gen = torch.Generator(device='cuda')
    gen.manual_seed(20261019)
    db = numpy.asarray(dg.deptht_bounds.cpu().numpy() if hasattr(dg.deptht_bounds, 'cpu') else dg.deptht_bounds, dtype=numpy.float64)
    th = torch.from_numpy(db[:, 1] - db[:, 0]).cuda()[None, :, None, None]

    def thickness():      # the nominal thickness times a partial-cell factor in [0.5, 1]
        f = 0.5 + 0.5 * torch.rand((1, nz, ny, nx), generator=gen, dtype=torch.float32, device='cuda')
        return (th * f).to(u.dtype).contiguous()

    e3 = (thickness(), thickness())
    r = measure(f'bench {nx}x{ny}x{nz} {real}, {len(xyzs)} transects', class_timing.field_maker(dg, xyzs), u, v, A, e3,
                float(db[-1, 1]), args)
    del u, v, A, e3, dg
    torch.cuda.empty_cache()
    return r


def main():
    ap = argparse.ArgumentParser(description=__doc__.split('\n')[0])
    ap.add_argument('--reps', type=int, default=10)
    ap.add_argument('--dtype', choices=['f64', 'f32'], default=None)
    ap.add_argument('--edges', default='16,75')
    ap.add_argument('--json', default='')
    ap.add_argument('--no-check', dest='no_check', action='store_true', help='leave the comparison with the reference out')
    args = ap.parse_args()
    args.edges = [int(x) for x in args.edges.split(',') if x]
    out = []
    for dt, real in (('f64', 'float64'), ('f32', 'float32')):
        if args.dtype and dt != args.dtype:
            continue
        out += bench_case(real, args)
        if args.json:       # written as it goes: a later case that runs out of time keeps the earlier ones
            with open(args.json, 'w') as f:
                json.dump(out, f, indent=1)
    if any(x.get('worst_error', 0.) > BAR for x in out):
        sys.exit('depth_remap_timing: a check misses its bar (see the lines above)')


if __name__ == '__main__':
    main()
