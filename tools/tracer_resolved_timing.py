"""Cost of the depth- and class-resolved tracer transports (nf_field_compute_tracer_profile_async,
nf_field_compute_class_tracer_transport_async) against the emulations they replace and against the volume forms.

For the bench workload (3600 x 1800 x 75, README singular transect + 64 seeded transects), float64 and float32: ms per step
(HIP events on the field's stream, median with min and max of --reps repetitions after warm-up) of
  * the volume profile and the tracer profile (4 and 4 + 5 gathers per record and level),
  * the volume class transport, the class-tracer transport with the carried tracer as its own class field (9 gathers) and
    with a class field of its own (14), for 16 and 256 edges,
and the emulations, measured in the same process, kernel time only (k_tracer_flux + K3: nf_field_compute_tracer_all_async of
the one step between events): for the profile nz tracer passes with the thickness set to one level at a time, for the
classes nedges + 2 tracer passes over uo / vo masked by the class of each U / V face (the masking is not timed).  The largest
difference of the emulated rows from the new rows is reported relative to the largest |row value|.  The bytes model: records
(40 B) and arc lengths (32 B) once per chunk of levels or window of rows, the DISTINCT elements of uo, vo and of each tracer
that the records touch per level, the rows.

The carried tracer is temperature-like (2 + 26 cos(lat) exp(-z / 25) + noise), the class field density-like (the same shape
from another seed); edges evenly spaced over [1, 29].  Only the timed step is generated (nt = 1).  For the kernels' own times
run it under rocprofv3 --kernel-trace --stats (--no-emulation).

    python tools/tracer_resolved_timing.py [--reps N] [--dtype f64|f32] [--classes 16,256] [--no-emulation] [--json OUT]
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
from nemoflux_amd import _lib  # noqa: E402
from nemoflux_amd._lib import lib, check  # noqa: E402
from nemoflux_amd.datagen import DataGen, STREAM_FUNCTIONS  # noqa: E402
from nemoflux_amd.field import Field  # noqa: E402

PEAK = 8.0e12
PROFILE_CHUNK, WINDOW = 8, 32      # nf::kProfileChunk, "class_window"
TRACER_PROFILE_CHUNK = {8: 4, 4: 8}   # nf::tracer_profile_chunk by element size
REF = 10.0


def make_tracer(u, ny, nz, seed):
    gen = torch.Generator(device='cuda')
    gen.manual_seed(seed)
    lat = torch.linspace(-89.95, 89.95, ny, dtype=torch.float64, device='cuda')
    z = torch.arange(nz, dtype=torch.float64, device='cuda')
    base = 2. + 26. * torch.cos(torch.deg2rad(lat))[None, :, None] * torch.exp(-z / 25.)[:, None, None]
    noise = torch.rand(tuple(u.shape), generator=gen, dtype=torch.float64, device='cuda') * 1.5
    return (base[None] + noise).to(u.dtype).contiguous()


def face_rows(sig, edges):
    """class row (int16) of the east and the north face of every cell: sig (1, nz, ny, nx) without markers, wrap on"""
    e = torch.from_numpy(edges).cuda()
    t = sig[0].double()
    xe = 0.5 * (t + torch.roll(t, -1, dims=2))
    xn = 0.5 * (t + torch.roll(t, -1, dims=1))
    xn[:, -1, :] = t[:, -1, :]                              # last row: no north neighbour
    return torch.bucketize(xe, e, right=True).to(torch.int16)[None], torch.bucketize(xn, e, right=True).to(torch.int16)[None]


def distinct_elements(fld):
    """number of records and of distinct uo, vo and tracer elements they touch per level"""
    ce, _, _ = fld.getWeights()
    cells = numpy.unique(ce // 4)
    nx, ncell = fld.nx, fld.nx * fld.ny
    j, i = cells // nx, cells % nx
    west = numpy.where(i > 0, cells - 1, cells - 1 + nx)
    east = numpy.where(i + 1 < nx, cells + 1, cells + 1 - nx)
    south = cells[j > 0] - nx
    north = cells[cells + nx < ncell] + nx
    return dict(nrec=int(ce.size // 4), u=int(numpy.unique(numpy.concatenate([cells, west])).size),
                v=int(numpy.unique(numpy.concatenate([cells, south])).size),
                tracer=int(numpy.unique(numpy.concatenate([cells, west, east, south, north])).size))


def model_bytes(d, fld, es, record_passes, field_passes, ntracers, nrows):
    """records + arc lengths once per pass over the records, the distinct elements of every level once per pass over the
    fields, the rows"""
    rec = record_passes * d['nrec'] * (40 + 32)
    gathered = field_passes * fld.nz * (d['u'] + d['v'] + ntracers * d['tracer']) * es
    return int(rec + gathered + nrows * fld._rowlen * 8)


def timed(call, reps, warm=3):
    stream = torch.cuda.current_stream()
    for _ in range(warm):
        call()
    torch.cuda.synchronize()
    ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(reps)]
    for a, b in ev:
        a.record(stream)
        call()
        b.record(stream)
    torch.cuda.synchronize()
    ms = sorted(a.elapsed_time(b) for a, b in ev)
    return dict(median=ms[len(ms) // 2], min=ms[0], max=ms[-1])


def with_model(t, nbytes):
    t.update(model_bytes=nbytes, fraction_of_8TBps=nbytes / (t['median'] * 1e-3) / PEAK)
    return t


def tracer_pass(fld, row):
    """k_tracer_flux + K3 of the one step, asynchronous on the field's stream"""
    check(lib.nf_field_compute_tracer_all_async(ctypes.byref(fld._h), ctypes.c_void_p(row.data_ptr())))


def emulate(fld, nrows, prepare, reps_emu):
    """`nrows` tracer passes, prepare(k) before each outside the events: (rows, sorted totals of kernel ms)"""
    stream = torch.cuda.current_stream()
    row = torch.zeros((1, fld._rowlen), dtype=torch.float64, device='cuda')
    rows = numpy.zeros((nrows, fld._rowlen))
    totals = []
    for r in range(reps_emu):
        tot = 0.0
        for k in range(nrows):
            prepare(k)
            torch.cuda.synchronize()
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record(stream)
            tracer_pass(fld, row)
            b.record(stream)
            torch.cuda.synchronize()
            tot += a.elapsed_time(b)
            rows[k] = row.cpu().numpy()[0]
        totals.append(tot)
    return rows, sorted(totals)


def spread(ms):
    return dict(median=ms[len(ms) // 2], min=ms[0], max=ms[-1], reps=len(ms))


def measure(real, args):
    nx, ny, nz = 3600, 1800, 75
    es = 8 if real == 'float64' else 4
    dg = DataGen(real=real)
    dg.setSizes(nx, ny, nz, 1)
    dg.setBoundingBox(-180., 180., -90., 90., 0., 1.)
    dg.build()
    dg.applyStreamFunction(STREAM_FUNCTIONS[5])
    u, v = dg.computeUVFromPotential()
    polys = bench.make_transects(nx, ny, -180., 180., -90., 90., 64)
    xyzs = [numpy.array([(x, y, 0.) for x, y in p]) for p in polys]
    tau, sig = make_tracer(u, ny, nz, 20261016), make_tracer(u, ny, nz, 20261017)

    def mk(u, v):
        with contextlib.redirect_stdout(io.StringIO()):
            return Field.fromArrays(dg.bounds_lon, dg.bounds_lat, dg.deptht_bounds, u, v, xyzs, readback=False,
                                    stream=torch.cuda.current_stream().cuda_stream)
    fld = mk(u, v)
    fld.setTracer(tau, reference=REF)
    h = ctypes.byref(fld._h)
    d = distinct_elements(fld)
    res = dict(case=f'bench {nx}x{ny}x{nz} {real}, {len(xyzs)} transects', reps=args.reps, nz=nz, row_length=fld._rowlen,
               distinct=d, gathers_per_level=dict(volume_profile=4, tracer_profile=9, class_volume=9, class_tracer_one=9,
                                                  class_tracer_two=14))

    # ---- profile
    out = torch.zeros((nz, fld._rowlen), dtype=torch.float64, device='cuda')
    vol = timed(lambda: check(lib.nf_field_compute_profile_async(h, 0, ctypes.c_void_p(out.data_ptr()))), args.reps)
    tra = timed(lambda: check(lib.nf_field_compute_tracer_profile_async(h, 0, ctypes.c_void_p(out.data_ptr()))), args.reps)
    prof = out.cpu().numpy()
    p = dict(volume_ms=with_model(vol, model_bytes(d, fld, es, -(-nz // PROFILE_CHUNK), 1, 0, nz)),
             tracer_ms=with_model(tra, model_bytes(d, fld, es, -(-nz // TRACER_PROFILE_CHUNK[es]), 1, 1, nz)),
             tracer_over_volume=tra['median'] / vol['median'], gather_ratio=9 / 4)
    if not args.no_emulation:
        th = fld.thickness.copy()

        def one_hot(z):
            one = numpy.zeros_like(th)
            one[z] = th[z]
            check(lib.nf_field_set_thickness(h, _lib.dptr(one), nz))
        rows, tot = emulate(fld, nz, one_hot, args.reps_emulation)
        check(lib.nf_field_set_thickness(h, _lib.dptr(th), nz))
        p.update(emulation_kernel_ms=spread(tot), speedup_vs_emulation=tot[len(tot) // 2] / tra['median'],
                 spreads_overlap=bool(tot[0] <= tra['max']),
                 emulation_rows_bit_identical=bool(numpy.array_equal(rows, prof)))
    res['profile'] = p
    print(json.dumps(dict(case=res['case'], profile=p)), flush=True)

    # ---- classes
    res['classes'] = []
    emu = None
    if not args.no_emulation:
        um, vm = torch.empty_like(u), torch.empty_like(v)
        emu = mk(um, vm)
        emu.setTracer(tau, reference=REF)
    for nedges in args.classes:
        edges = numpy.linspace(1., 29., nedges)
        fld.setClassEdges(edges)
        nrow = nedges + 2
        nwin = -(-nrow // WINDOW)
        out = torch.zeros((nrow, fld._rowlen), dtype=torch.float64, device='cuda')
        ptr = ctypes.c_void_p(out.data_ptr())
        fld.setClassTracer(None)
        cvol = timed(lambda: check(lib.nf_field_compute_class_transport_async(h, 0, ptr)), args.reps, 2)
        one = timed(lambda: check(lib.nf_field_compute_class_tracer_transport_async(h, 0, ptr)), args.reps, 2)
        fld.setClassTracer(sig)
        two = timed(lambda: check(lib.nf_field_compute_class_tracer_transport_async(h, 0, ptr)), args.reps, 2)
        rows = out.cpu().numpy()
        c = dict(nedges=nedges, rows=nrow, window=WINDOW, rows_nonzero=int((numpy.abs(rows).max(axis=1) > 0).sum()),
                 class_volume_ms=with_model(cvol, model_bytes(d, fld, es, nwin, nwin, 1, nrow)),
                 class_tracer_one_ms=with_model(one, model_bytes(d, fld, es, nwin, nwin, 1, nrow)),
                 class_tracer_two_ms=with_model(two, model_bytes(d, fld, es, nwin, nwin, 2, nrow)),
                 one_over_volume=one['median'] / cvol['median'], two_over_volume=two['median'] / cvol['median'],
                 gather_ratio_one=9 / 9, gather_ratio_two=14 / 9)
        if emu is not None:
            rE, rN = face_rows(sig, edges)

            def mask(k):
                torch.where(rE == k, u, torch.zeros_like(u), out=um)
                torch.where(rN == k, v, torch.zeros_like(v), out=vm)
            erows, tot = emulate(emu, nrow, mask, args.reps_emulation)
            c.update(emulation_kernel_ms=spread(tot), speedup_vs_emulation=tot[len(tot) // 2] / two['median'],
                     spreads_overlap=bool(tot[0] <= two['max']),
                     emulation_max_diff_over_max_abs=float(numpy.abs(erows - rows).max() / numpy.abs(rows).max()))
            del rE, rN
        print(json.dumps(dict(case=res['case'], classes=c)), flush=True)
        res['classes'].append(c)
    del fld, emu
    torch.cuda.empty_cache()
    return res


def main():
    ap = argparse.ArgumentParser(description=__doc__.split('\n')[0])
    ap.add_argument('--reps', type=int, default=10)
    ap.add_argument('--reps-emulation', dest='reps_emulation', type=int, default=3,
                    help='repetitions of an emulation (each is nz or nedges + 2 tracer passes)')
    ap.add_argument('--dtype', choices=['f64', 'f32'], default=None)
    ap.add_argument('--classes', default='16,256')
    ap.add_argument('--json', default='')
    ap.add_argument('--no-emulation', action='store_true', help='the new launches only (for rocprofv3 runs)')
    args = ap.parse_args()
    args.classes = [int(x) for x in args.classes.split(',') if x]
    out = []
    for dt, real in (('f64', 'float64'), ('f32', 'float32')):
        if args.dtype and dt != args.dtype:
            continue
        out.append(measure(real, args))
        if args.json:       # written as it goes: a later case that runs out of time keeps the earlier one
            with open(args.json, 'w') as f:
                json.dump(out, f, indent=1)


if __name__ == '__main__':
    main()
