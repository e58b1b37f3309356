"""Cost of a tracer-transport step (nf_field_compute_tracer_all_async, one time step: K1tau + K3) against the volume step
(nf_field_compute_all_async: K1 + K3) on the bench workload, measured in the same process, alternating.

The workload is bench.py's: 3600 x 1800 x 75, README singular transect + 64 seeded transects, uo / vo from nf_datagen_uv
(stream function 5), float64 and float32.  The tracer is filled on the device by a seeded torch generator (5 .. 25).
Per round the two steps run back to back in alternating order, each bracketed by HIP events on the field's stream; the
medians over the rounds are reported with their ratio.  Algorithmic bytes of K1tau: 3*sizeof(T) per (t,z,j,i) plus
(16 arc + 16 planes) per cell; K1's: 2*sizeof(T) plus (16 arc + 32 iV + 16 abs) (nf_flux.hip).  For the kernels' own
times (and so their share of 8 TB/s) run it under rocprofv3 --kernel-trace --stats.

    python tools/tracer_timing.py [--reps N] [--dtype f64|f32] [--json OUT]
"""
import argparse
import contextlib
import ctypes
import io
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy  # noqa: E402
import torch  # noqa: E402

import bench  # noqa: E402
from nemoflux_amd._lib import lib, check  # noqa: E402
from nemoflux_amd.datagen import DataGen, STREAM_FUNCTIONS  # noqa: E402
from nemoflux_amd.field import Field  # noqa: E402

PEAK = 8.0e12


def run(real, reps):
    nx, ny, nz = 3600, 1800, 75
    es = 8 if real == 'float64' else 4
    dg = DataGen(real=real)
    dg.setSizes(nx, ny, nz, 1)
    dg.setBoundingBox(-180., 180., -90., 90., 0., 1.)
    dg.build()
    dg.applyStreamFunction(STREAM_FUNCTIONS[5])
    u, v = dg.computeUVFromPotential()
    gen = torch.Generator(device='cuda')
    gen.manual_seed(20261015)
    tau = torch.rand(tuple(u.shape), generator=gen, dtype=u.dtype, device='cuda') * 20 + 5
    polys = bench.make_transects(nx, ny, -180., 180., -90., 90., 64)
    xyzs = [numpy.array([(x, y, 0.) for x, y in p]) for p in polys]
    stream = torch.cuda.current_stream()
    with contextlib.redirect_stdout(io.StringIO()):
        fld = Field.fromArrays(dg.bounds_lon, dg.bounds_lat, dg.deptht_bounds, u, v, xyzs, readback=False,
                               stream=stream.cuda_stream)
    fld.setTracer(tau, reference=0.0)
    rows_v = torch.zeros((1, fld._rowlen), dtype=torch.float64, device='cuda')
    rows_t = torch.zeros((1, fld._rowlen), dtype=torch.float64, device='cuda')

    def volume():
        check(lib.nf_field_compute_all_async(ctypes.byref(fld._h), ctypes.c_void_p(rows_v.data_ptr())))

    def tracer():
        check(lib.nf_field_compute_tracer_all_async(ctypes.byref(fld._h), ctypes.c_void_p(rows_t.data_ptr())))

    for _ in range(3):
        volume()
        tracer()
    torch.cuda.synchronize()
    ms = {'volume': [], 'tracer': []}
    for r in range(reps):
        order = (('volume', volume), ('tracer', tracer)) if r % 2 == 0 else (('tracer', tracer), ('volume', volume))
        for name, fn in order:
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record(stream)
            fn()
            b.record(stream)
            b.synchronize()
            ms[name].append(a.elapsed_time(b))
    ncell = nx * ny
    bytes_tracer = 3 * es * ncell * nz + (16 + 16) * ncell
    bytes_k1 = 2 * es * ncell * nz + (16 + 32 + 16) * ncell
    med = {k: float(numpy.median(x)) for k, x in ms.items()}
    res = dict(case=f'bench {nx}x{ny}x{nz} {real}, {len(xyzs)} transects', reps=reps,
               volume_step_ms_median=med['volume'], tracer_step_ms_median=med['tracer'],
               volume_step_ms_min=min(ms['volume']), tracer_step_ms_min=min(ms['tracer']),
               tracer_over_volume=med['tracer'] / med['volume'],
               algorithmic_bytes_k1tau=bytes_tracer, algorithmic_bytes_k1=bytes_k1,
               tracer_step_fraction_of_8TBps=bytes_tracer / (med['tracer'] * 1e-3) / PEAK,
               volume_step_fraction_of_8TBps=bytes_k1 / (med['volume'] * 1e-3) / PEAK,
               tracer_row_finite=bool(torch.isfinite(rows_t).all().item()),
               tracer_total_transect0=float(rows_t[0, fld._nseg].item()))
    print(json.dumps(res), flush=True)
    del fld, u, v, tau, dg
    torch.cuda.empty_cache()
    return res


def main():
    ap = argparse.ArgumentParser(description=__doc__.split('\n')[0])
    ap.add_argument('--reps', type=int, default=20)
    ap.add_argument('--dtype', choices=['f64', 'f32'], default=None)
    ap.add_argument('--json', default='')
    args = ap.parse_args()
    out = []
    for dt, real in (('f64', 'float64'), ('f32', 'float32')):
        if args.dtype and dt != args.dtype:
            continue
        out.append(run(real, args.reps))
    if args.json:
        with open(args.json, 'w') as f:
            json.dump(out, f, indent=1)


if __name__ == '__main__':
    main()
