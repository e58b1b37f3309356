"""Cost of a step of the transports between surfaces (nf_field_compute_surface_transport_async) against the depth bins beside it.

For the bench workload (3600 x 1800 x 75, README singular transect + 64 seeded transects), float64 and float32, with m = 2 and 8
surfaces in HBM, with the per-level thickness and with a per-cell thickness (the nominal one times a partial-cell factor in
[0.5, 1]): ms per step (HIP events on the field's stream, medians of --reps with min - max, the calls alternating in one
process) of the volume and the carried form, and of the yardstick: computeDepthTransport WITH THE CELL THICKNESS at
n = max(m, 2) edges, the same form (volume or carried) at the same dtype -- the form that also carries four spans per level.
Both thickness forms of the surface kernel are held against that one yardstick.  The target is at most 1.25 x the yardstick:
the margin is for the one-time 5 m surface gathers and for the per-lane edges in LDS.  `ratio` is ms / yardstick ms: <= 1.25
meets the target; a miss is reported as a miss.

Also printed: the worst error of one step against tests/surface_transport_reference.py relative to sum |share| of the value
(bar 1e-12), for the volume form at the first m and the carried form at the last, both with the per-cell thickness (--no-check
leaves it out).

    python tools/surface_transport_timing.py [--reps N] [--dtype f64|f32] [--surfaces 2,8] [--no-check] [--json OUT]
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
TARGET = 1.25


def reference_step(fld, arrays, surfaces, carry, cell):
    """the reference's rows of step 0 and their sum |share|, and how many terms were spread over more than one row"""
    from surface_transport_reference import SurfaceReference
    ce, w, sg = fld.getWeights()
    ref = SurfaceReference(ce, w, sg, fld.arcLengths, fld.thickness, fld._tr_off, fld.nx, fld.ny, reference=0.0, wrap=True,
                           sverdrup=fld.sverdrup, cell_thickness=cell)
    cells = torch.from_numpy(ref.cells).cuda()

    def values(name, z, _cells):
        if name == 'surface':
            return surfaces[z].reshape(-1)[cells].cpu().numpy()
        return arrays[name][0, z].reshape(-1)[cells].cpu().numpy()

    want = ref.surface_step(values, len(surfaces), tracer=carry)
    return want['carried' if carry else 'volume'], want['spread_terms']


def measure(name, mk_field, u, v, A, e3, zmax, gen, args):
    res = []
    plain, thick = mk_field(u, v), mk_field(u, v)
    thick.setCellThickness(*e3)
    for fld in (plain, thick):
        fld.setTracer(A)
    nrec = plain.getWeights()[0].size // 4
    base = dict(case=name, records=int(nrec), row_length=plain._rowlen, reps=args.reps)
    print(json.dumps(base), flush=True)
    keys = ('median', 'min', 'max')
    arrays = {'uo': u, 'vo': v, 'tracer': A, 'e3u': e3[0], 'e3v': e3[1]}
    for m in args.surfaces:
        # surface k around the depth (k + 1/2) zmax / m, moved by up to a band's width: neighbours cross here and there
        surfaces = [((k + 0.5 + (torch.rand((plain.ny, plain.nx), generator=gen, dtype=torch.float32, device='cuda') - 0.5) * 1.2)
                     * (zmax / m)).to(u.dtype).contiguous() for k in range(m)]
        n = max(m, 2)
        thick.setDepthEdges(numpy.linspace(0., zmax, n + 2)[1:-1])
        yard_out = torch.zeros((n + 2, plain._rowlen), dtype=torch.float64, device='cuda')
        out = torch.zeros((m + 2, plain._rowlen), dtype=torch.float64, device='cuda')
        for fld in (plain, thick):
            fld.setDepthSurfaces(surfaces)
        for cell, fld in ((False, plain), (True, thick)):
            for carry in (False, True):
                def surface():
                    check(lib.nf_field_compute_surface_transport_async(ctypes.byref(fld._h), 0, int(carry), ctypes.c_void_p(out.data_ptr())))

                def yardstick():
                    check(lib.nf_field_compute_depth_transport_async(ctypes.byref(thick._h), 0, int(carry),
                                                                     ctypes.c_void_p(yard_out.data_ptr())))

                t = [dict(zip(keys, x)) for x in timed([surface, yardstick], args.reps)]
                r = dict(base, surfaces=m, yardstick_edges=n, thickness='cell' if cell else 'scalar',
                         form='carried' if carry else 'volume', ms=t[0], yardstick_ms=t[1], ratio=t[0]['median'] / t[1]['median'])
                r['meets_target'] = bool(r['ratio'] <= TARGET)
                surface()
                torch.cuda.synchronize()
                rows = out.cpu().numpy()
                if not args.no_check and cell and ((not carry and m == args.surfaces[0]) or (carry and m == args.surfaces[-1])):
                    (w_, m_), r['spread_terms'] = reference_step(fld, arrays, surfaces, carry, cell)
                    r['worst_error'] = float((numpy.abs(rows - w_) / numpy.where(m_ > 0, m_, 1.0)).max())
                print(json.dumps(r), flush=True)
                res.append(r)
        del out, yard_out, surfaces
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
    gen.manual_seed(20261020)
    db = numpy.asarray(dg.deptht_bounds.cpu().numpy() if hasattr(dg.deptht_bounds, 'cpu') else dg.deptht_bounds, dtype=numpy.float64)
    th = torch.from_numpy(db[:, 1] - db[:, 0]).cuda()[None, :, None, None]

    def thickness():      # the nominal thickness times a partial-cell factor in [0.5, 1]
        f = 0.5 + 0.5 * torch.rand((1, nz, ny, nx), generator=gen, dtype=torch.float32, device='cuda')
        return (th * f).to(u.dtype).contiguous()

    e3 = (thickness(), thickness())
    r = measure(f'bench {nx}x{ny}x{nz} {real}, {len(xyzs)} transects', class_timing.field_maker(dg, xyzs), u, v, A, e3,
                float(db[-1, 1]), gen, args)
    del u, v, A, e3, dg
    torch.cuda.empty_cache()
    return r


def main():
    ap = argparse.ArgumentParser(description=__doc__.split('\n')[0])
    ap.add_argument('--reps', type=int, default=10)
    ap.add_argument('--dtype', choices=['f64', 'f32'], default=None)
    ap.add_argument('--surfaces', default='2,8')
    ap.add_argument('--json', default='')
    ap.add_argument('--no-check', dest='no_check', action='store_true', help='leave the comparison with the reference out')
    args = ap.parse_args()
    args.surfaces = [int(x) for x in args.surfaces.split(',') if x]
    out = []
    for dt, real in (('f64', 'float64'), ('f32', 'float32')):
        if args.dtype and dt != args.dtype:
            continue
        out += bench_case(real, args)
        if args.json:       # written as it goes: a later case that runs out of time keeps the earlier ones
            with open(args.json, 'w') as f:
                json.dump(out, f, indent=1)
    if any(x.get('worst_error', 0.) > BAR for x in out):
        sys.exit('surface_transport_timing: a check misses its bar (see the lines above)')


if __name__ == '__main__':
    main()
