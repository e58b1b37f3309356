"""Cost of a class-transport step (nf_field_compute_class_transport_async) against the masked emulation it replaces.

For the bench workload (3600 x 1800 x 75, README singular transect + 64 seeded transects) and BASELINE config C3 (1440 x 1021
x 75, the 50-station transect), float64 and float32, with 16, 64 and 256 class edges (nedges + 2 rows): ms per class step
(HIP events on the field's stream, medians) for the class windows 8, 16 and 32 (nf_tuning_set "class_window": rows per pass
over the fields), and the emulation measured in the same process -- nedges + 2 computeFlux calls over uo / vo masked by the
class of each U / V face, counting their kernel time only (K1 + K3; the masking is excluded) -- with the largest difference
of its rows from the class rows relative to sum |terms| of the value (a torch restatement of the terms on the device).  The
algorithmic bytes of one class step: the records (40 B) and the four arc lengths they read (32 B), and the DISTINCT u / v /
tau elements the records touch per level, once per window; the rows -- with their fraction of 8 TB/s.

The tracer is temperature-like, generated on the device from a seeded generator: 2 + 26 cos(lat) exp(-z / 25) plus uniform
noise of 1.5 degrees, so that the faces spread over the classes (edges evenly spaced over [1, 29]).  Only the timed step is
generated (nt = 1).  For the kernels' own times run it under rocprofv3 --kernel-trace --stats (--no-emulation).

    python tools/class_timing.py [--reps N] [--only bench|c3] [--dtype f64|f32] [--classes 16,64,256] [--windows 8,16,32]
                                 [--no-emulation] [--json OUT]
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
DEFAULT_WINDOW = 32     # nf_tuning_set("class_window") default


def make_tracer(u, ny, nz, lat0, lat1):
    gen = torch.Generator(device='cuda')
    gen.manual_seed(20261016)
    lat = torch.linspace(lat0, lat1, ny, dtype=torch.float64, device='cuda')
    z = torch.arange(nz, dtype=torch.float64, device='cuda')
    base = 2. + 26. * torch.cos(torch.deg2rad(lat))[None, :, None] * torch.exp(-z / 25.)[:, None, None]
    noise = torch.rand(tuple(u.shape), generator=gen, dtype=torch.float64, device='cuda') * 1.5
    return (base[None] + noise).to(u.dtype).contiguous()


def face_rows(tau, edges):
    """class row (int16) of the east and the north face of every cell: tau (1, nz, ny, nx) without markers, wrap on"""
    e = torch.from_numpy(edges).cuda()
    t = tau[0].double()
    xe = 0.5 * (t + torch.roll(t, -1, dims=2))
    xn = 0.5 * (t + torch.roll(t, -1, dims=1))
    xn[:, -1, :] = t[:, -1, :]                              # last row: no north neighbour
    rE = torch.bucketize(xe, e, right=True).to(torch.int16)  # number of edges <= x
    rN = torch.bucketize(xn, e, right=True).to(torch.int16)
    return rE[None], rN[None]


def abs_terms(fld, u, v, rE, rN, nrow):
    """sum |terms| per (row, value) of one class step, restated with torch on the device from the weights"""
    ce, w, sg = fld.getWeights()
    ce, w, sg = (torch.from_numpy(x).cuda() for x in (ce, w, sg))
    nx, ncell = fld.nx, fld.nx * fld.ny
    c, slot = ce // 4, ce % 4
    j, i = c // nx, c % nx
    cell = torch.where(slot == 0, torch.where(j > 0, c - nx, c), torch.where(slot == 3, torch.where(i > 0, c - 1, c - 1 + nx), c))
    ew = (slot == 1) | (slot == 3)
    keep = (slot != 0) | (j > 0)
    arc = torch.from_numpy(fld.arcLengths).cuda()
    a = torch.where(ew, arc[cell, 1], arc[cell, 2])
    th = fld.thickness
    scale = 6371000.0 / 1.e6 if fld.sverdrup else 1.0
    mag = torch.zeros(nrow * fld._nseg, dtype=torch.float64, device='cuda')
    for z in range(fld.nz):
        uz, vz = u[0, z].reshape(-1).double(), v[0, z].reshape(-1).double()
        d = torch.where(ew, uz[cell], vz[cell]) * th[z] * a * scale
        row = torch.where(ew, rE[0, z].reshape(-1)[cell], rN[0, z].reshape(-1)[cell]).long()
        mag.index_add_(0, row * fld._nseg + sg, torch.where(keep, (w * d).abs(), torch.zeros_like(d)))
    mag = mag.reshape(nrow, fld._nseg).cpu().numpy()
    o = fld._tr_off
    tot = numpy.stack([mag[:, o[p]:o[p + 1]].sum(axis=1) for p in range(len(o) - 1)], axis=1)
    del ce, w, sg, c, slot, cell, a
    return numpy.concatenate([mag, tot], axis=1), int(ncell)


def algorithmic_bytes(fld, es, nedges, window):
    """records + arc lengths and the distinct u / v / tau elements per level, once per window; the rows"""
    ce, _, _ = fld.getWeights()
    nrec = ce.size // 4
    cells = numpy.unique(ce // 4)
    nx, ncell = fld.nx, fld.nx * fld.ny
    j, i = cells // nx, cells % nx
    west = numpy.where(i > 0, cells - 1, cells - 1 + nx)
    east = numpy.where(i + 1 < nx, cells + 1, cells + 1 - nx)
    south = cells[j > 0] - nx
    north = cells[cells + nx < ncell] + nx
    nu = numpy.unique(numpy.concatenate([cells, west])).size
    nv = numpy.unique(numpy.concatenate([cells, south])).size
    nt = numpy.unique(numpy.concatenate([cells, west, east, south, north])).size
    nwin = -(-(nedges + 2) // window)
    rec = nwin * nrec * (40 + 32)
    gathered = nwin * fld.nz * (nu + nv + nt) * es
    rows = (nedges + 2) * fld._rowlen * 8
    return dict(nrec=int(nrec), windows=int(nwin), distinct_u=int(nu), distinct_v=int(nv), distinct_tau=int(nt),
                record_bytes=int(rec), gathered_bytes=int(gathered), row_bytes=int(rows), total=int(rec + gathered + rows))


def time_class(fld, out, reps):
    stream = torch.cuda.current_stream()

    def step():
        check(lib.nf_field_compute_class_transport_async(ctypes.byref(fld._h), 0, ctypes.c_void_p(out.data_ptr())))
    for _ in range(2):
        step()
    torch.cuda.synchronize()
    ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(reps)]
    for a, b in ev:
        a.record(stream)
        step()
        b.record(stream)
    torch.cuda.synchronize()
    return sorted(a.elapsed_time(b) for a, b in ev)


def measure(name, mk_field, u, v, tau, es, lat, reps, classes, windows, emulation):
    res = []
    fld = mk_field(u, v)
    fld.setTracer(tau)
    emu = None
    if emulation:
        um, vm = torch.empty_like(u), torch.empty_like(v)
        emu = mk_field(um, vm)
    for nedges in classes:
        edges = numpy.linspace(1., 29., nedges)
        fld.setClassEdges(edges)
        nrow = nedges + 2
        out = torch.zeros((nrow, fld._rowlen), dtype=torch.float64, device='cuda')
        per_window = {}
        for w in windows:
            check(lib.nf_tuning_set(b'class_window', int(w)))
            try:
                ms = time_class(fld, out, reps)
                per_window[str(w)] = dict(median=ms[len(ms) // 2], min=ms[0], max=ms[-1])
            except RuntimeError as err:      # a launch the runtime refuses is a finding, not the end of the run
                per_window[str(w)] = dict(error=str(err))
        check(lib.nf_tuning_set(b'class_window', DEFAULT_WINDOW))
        ms = time_class(fld, out, reps)
        med = ms[len(ms) // 2]
        rows = out.cpu().numpy()
        r = dict(case=name, nedges=nedges, rows=nrow, row_length=fld._rowlen, reps=reps, window=DEFAULT_WINDOW,
                 class_ms_median=med, class_ms_min=ms[0], class_ms_max=ms[-1], by_window=per_window,
                 rows_nonzero=int((numpy.abs(rows).max(axis=1) > 0).sum()))
        b = algorithmic_bytes(fld, es, nedges, DEFAULT_WINDOW)
        r.update(bytes=b, algorithmic_TBps=b['total'] / (med * 1e-3) / 1e12, fraction_of_8TBps=b['total'] / (med * 1e-3) / PEAK)
        if emu is not None:
            rE, rN = face_rows(tau, edges)
            emu_rows = numpy.zeros_like(rows)
            emu.enableKernelTiming(True, reserve=nrow + 1)
            kms = 0.0
            for k in range(nrow):
                torch.where(rE == k, u, torch.zeros_like(u), out=um)
                torch.where(rN == k, v, torch.zeros_like(v), out=vm)
                torch.cuda.synchronize()
                emu.computeFlux(0)
                n, t_ms = emu.readKernelTiming()
                kms += t_ms + emu.readTransectTiming()
                emu_rows[k] = emu._row[:emu._rowlen]
            emu.enableKernelTiming(False)
            mag, _ = abs_terms(fld, u, v, rE, rN, nrow)
            vol = emu_rows.sum(axis=0)
            rel = numpy.abs(emu_rows - rows) / numpy.where(mag > 0, mag, 1.0)
            r.update(emulation_device_ms=kms, speedup_vs_emulation=kms / med,
                     emulation_max_diff_over_sum_abs_terms=float(rel.max()),
                     emulation_rows_exactly_equal=int(numpy.sum(numpy.all(emu_rows == rows, axis=1))),
                     conservation_max_diff_over_sum_abs_terms=float(
                         (numpy.abs(rows.sum(axis=0) - vol) / numpy.maximum(mag.sum(axis=0), 1e-300)).max()))
            del rE, rN
        print(json.dumps(r), flush=True)
        res.append(r)
    del fld, emu
    torch.cuda.empty_cache()
    return res


def field_maker(dg, xyzs):
    def mk(u, v):
        with contextlib.redirect_stdout(io.StringIO()):
            return Field.fromArrays(dg.bounds_lon, dg.bounds_lat, dg.deptht_bounds, u, v, xyzs, readback=False,
                                    stream=torch.cuda.current_stream().cuda_stream)
    return mk


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
    tau = make_tracer(u, ny, nz, -89.95, 89.95)
    r = measure(f'bench {nx}x{ny}x{nz} {real}, {len(xyzs)} transects', field_maker(dg, xyzs), u, v, tau,
                8 if real == 'float64' else 4, None, args.reps, args.classes, args.windows, not args.no_emulation)
    del u, v, tau, dg
    torch.cuda.empty_cache()
    return r


def c3_case(real, args):
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
    tau = make_tracer(u, ny, nz, -89.9, 89.9)
    r = measure(f'C3 {nx}x{ny}x{nz} {real}, {len(st)} stations', field_maker(dg, [xyz]), u, v, tau,
                8 if real == 'float64' else 4, None, args.reps, args.classes, args.windows, not args.no_emulation)
    del u, v, tau, dg
    torch.cuda.empty_cache()
    return r


def main():
    ap = argparse.ArgumentParser(description=__doc__.split('\n')[0])
    ap.add_argument('--reps', type=int, default=10)
    ap.add_argument('--only', choices=['bench', 'c3'], default=None)
    ap.add_argument('--dtype', choices=['f64', 'f32'], default=None)
    ap.add_argument('--classes', default='16,64,256')
    ap.add_argument('--windows', default='8,16,32')
    ap.add_argument('--json', default='')
    ap.add_argument('--no-emulation', action='store_true', help='class launches only (for rocprofv3 runs)')
    args = ap.parse_args()
    args.classes = [int(x) for x in args.classes.split(',') if x]
    args.windows = [int(x) for x in args.windows.split(',') if x]
    out = []
    for case, fn in (('bench', bench_case), ('c3', c3_case)):
        if args.only and case != args.only:
            continue
        for dt, real in (('f64', 'float64'), ('f32', 'float32')):
            if args.dtype and dt != args.dtype:
                continue
            out += fn(real, args)
            if args.json:       # written as it goes: a later case that runs out of time keeps the earlier ones
                with open(args.json, 'w') as f:
                    json.dump(out, f, indent=1)


if __name__ == '__main__':
    main()
