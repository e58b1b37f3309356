"""Cost of a depth-resolved step (nf_field_compute_profile_async) against the one-hot emulation it replaces.

For the bench workload (3600 x 1800 x 75, README singular transect + 64 seeded transects) and BASELINE config C3 (1440 x 1021
x 75, the 50-station transect), float64 and float32: ms per profile step (HIP events on the field's stream), the one-hot
emulation measured in the same process (nz computeFlux calls, the thickness set to level z alone before each: K1 + K3 per
level) and whether its rows equal the profile's bit for bit, and the kernel's algorithmic bytes -- the records (40 B) and
the four arc lengths they read (32 B) once per chunk of levels, the DISTINCT uo / vo elements the records touch per level
(counted on the host from the weights), the rows -- with their fraction of 8 TB/s.

    python tools/profile_timing.py [--reps N] [--only bench|c3] [--dtype f64|f32] [--no-onehot] [--json OUT]
"""
import argparse
import contextlib
import ctypes
import io
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy  # noqa: E402
import torch  # noqa: E402

import bench  # noqa: E402
from nemoflux_amd import _lib  # noqa: E402
from nemoflux_amd._lib import lib, check  # noqa: E402
from nemoflux_amd.datagen import DataGen, STREAM_FUNCTIONS  # noqa: E402
from nemoflux_amd.field import Field  # noqa: E402

PEAK = 8.0e12
CHUNK = 8          # nf::kProfileChunk


def algorithmic_bytes(fld, es):
    """records + arc lengths once per chunk, distinct u / v elements per level, rows"""
    ce, _, _ = fld.getWeights()
    nrec = ce.size // 4
    cells = numpy.unique(ce // 4)
    nx = fld.nx
    j, i = cells // nx, cells % nx
    west = numpy.where(i > 0, cells - 1, cells - 1 + nx)
    south = cells[j > 0] - nx
    nu = numpy.unique(numpy.concatenate([cells, west])).size
    nv = numpy.unique(numpy.concatenate([cells, south])).size
    nchunks = -(-fld.nz // CHUNK)
    rec = nchunks * nrec * (40 + 32)
    gathered = fld.nz * (nu + nv) * es
    rows = fld.nz * fld._rowlen * 8
    return dict(nrec=int(nrec), distinct_u=int(nu), distinct_v=int(nv), record_bytes=int(rec), gathered_bytes=int(gathered),
                row_bytes=int(rows), total=int(rec + gathered + rows))


def measure(name, fld, es, reps, onehot=True):
    stream = torch.cuda.current_stream()
    out = torch.zeros((fld.nz, fld._rowlen), dtype=torch.float64, device='cuda')

    def prof():
        check(lib.nf_field_compute_profile_async(ctypes.byref(fld._h), 0, ctypes.c_void_p(out.data_ptr())))
    for _ in range(3):
        prof()
    torch.cuda.synchronize()
    ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(reps)]
    for a, b in ev:
        a.record(stream)
        prof()
        b.record(stream)
    torch.cuda.synchronize()
    ms = sorted(a.elapsed_time(b) for a, b in ev)
    profile_rows = out.cpu().numpy()

    # one-hot emulation: one field, its thickness set to level z alone before each computeFlux (K1 + K3 of a full step)
    th = fld.thickness.copy()
    emu_rows = numpy.zeros_like(profile_rows)
    emu_ms, emu_dev_ms = [float('nan')], [float('nan')]
    for r in range(2 if onehot else 0):
        if r == 0:
            emu_ms, emu_dev_ms = [], []
        fld.enableKernelTiming(True, reserve=fld.nz + 1)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for z in range(fld.nz):
            one = numpy.zeros_like(th)
            one[z] = th[z]
            check(lib.nf_field_set_thickness(ctypes.byref(fld._h), _lib.dptr(one), fld.nz))
            fld.computeFlux(0)
            emu_rows[z] = fld._row[:fld._rowlen]
        torch.cuda.synchronize()
        emu_ms.append((time.perf_counter() - t0) * 1e3)
        n, kms = fld.readKernelTiming()
        emu_dev_ms.append(kms + fld.readTransectTiming())
        fld.enableKernelTiming(False)
    check(lib.nf_field_set_thickness(ctypes.byref(fld._h), _lib.dptr(th), fld.nz))
    b = algorithmic_bytes(fld, es)
    med = ms[len(ms) // 2]
    res = dict(case=name, nz=fld.nz, row_length=fld._rowlen, profile_ms_median=med, profile_ms_min=ms[0],
               profile_ms_max=ms[-1], reps=reps, onehot_wall_ms=min(emu_ms), onehot_device_ms=min(emu_dev_ms),
               speedup_vs_onehot_device=min(emu_dev_ms) / med, speedup_vs_onehot_wall=min(emu_ms) / med,
               onehot_rows_bit_identical=bool(numpy.array_equal(emu_rows, profile_rows)) if onehot else None,
               bytes=b, algorithmic_TBps=b['total'] / (med * 1e-3) / 1e12, fraction_of_8TBps=b['total'] / (med * 1e-3) / PEAK)
    print(json.dumps(res), flush=True)
    return res


def bench_case(real, reps, onehot):
    nx, ny, nz = 3600, 1800, 75
    dg = DataGen(real=real)
    dg.setSizes(nx, ny, nz, 1)
    dg.setBoundingBox(-180., 180., -90., 90., 0., 1.)
    dg.build()
    dg.applyStreamFunction(STREAM_FUNCTIONS[5])
    u, v = dg.computeUVFromPotential()
    polys = bench.make_transects(nx, ny, -180., 180., -90., 90., 64)
    xyzs = [numpy.array([(x, y, 0.) for x, y in p]) for p in polys]
    with contextlib.redirect_stdout(io.StringIO()):
        fld = Field.fromArrays(dg.bounds_lon, dg.bounds_lat, dg.deptht_bounds, u, v, xyzs, readback=False,
                               stream=torch.cuda.current_stream().cuda_stream)
    r = measure(f'bench {nx}x{ny}x{nz} {real}, {len(xyzs)} transects', fld, 8 if real == 'float64' else 4, reps, onehot)
    del fld, u, v, dg
    torch.cuda.empty_cache()
    return r


def c3_case(real, reps, onehot):
    nx, ny, nz = 1440, 1021, 75
    with open(os.path.join(ROOT, 'tests', 'golden', 'stations.json')) as f:
        st = json.load(f)['S3_sta_bdep.txt']
    xyz = numpy.array([(lon, lat, 0.) for lon, lat in st])
    dg = DataGen(real=real)
    dg.setSizes(nx, ny, nz, 1)
    dg.setBoundingBox(-180., 180., -90., 90., 0., 1.)
    dg.build()
    dg.applyStreamFunction(STREAM_FUNCTIONS[2])
    u, v = dg.computeUVFromPotential()
    with contextlib.redirect_stdout(io.StringIO()):
        fld = Field.fromArrays(dg.bounds_lon, dg.bounds_lat, dg.deptht_bounds, u, v, [xyz], readback=False,
                               stream=torch.cuda.current_stream().cuda_stream)
    r = measure(f'C3 {nx}x{ny}x{nz} {real}, {len(st)} stations', fld, 8 if real == 'float64' else 4, reps, onehot)
    del fld, u, v, dg
    torch.cuda.empty_cache()
    return r


def main():
    ap = argparse.ArgumentParser(description=__doc__.split('\n')[0])
    ap.add_argument('--reps', type=int, default=20)
    ap.add_argument('--only', choices=['bench', 'c3'], default=None)
    ap.add_argument('--dtype', choices=['f64', 'f32'], default=None)
    ap.add_argument('--json', default='')
    ap.add_argument('--no-onehot', action='store_true', help='profile launches only (for rocprofv3 runs)')
    args = ap.parse_args()
    out = []
    for case, fn in (('bench', bench_case), ('c3', c3_case)):
        if args.only and case != args.only:
            continue
        for dt, real in (('f64', 'float64'), ('f32', 'float32')):
            if args.dtype and dt != args.dtype:
                continue
            out.append(fn(real, args.reps, not args.no_onehot))
    if args.json:
        with open(args.json, 'w') as f:
            json.dump(out, f, indent=1)


if __name__ == '__main__':
    main()
