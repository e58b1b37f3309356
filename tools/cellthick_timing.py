"""Cost of the transports with per-cell layer thicknesses (nf_field_set_cell_thickness) against the per-level forms and against
what a user could do without them, all in one process on one build.

For the bench workload (3600 x 1800 x 75, README singular transect + 64 seeded transects, nt = 2), float64 and float32, with
a static (1, nz, ny, nx) and a time-varying (nt, nz, ny, nx) thickness in HBM; ms per time step, HIP events on the field's
stream, median with min and max of --reps repetitions after warm-up:
  * the volume step (flux kernel + expansion + K3: nf_field_compute_all_async / nt) with and without a cell thickness, and
    from the library's own per-launch events the flux kernel alone (K1 against the cell-thickness kernel), with the bytes
    model of each -- K1 2 sizeof(T) per (t, z, cell) plus arcs and six planes, the new kernel 4 sizeof(T) plus arcs and two
    planes -- as a fraction of 8 TB/s;
  * the route without the feature: torch premultiplies uo * e3u / th[z] and vo * e3v / th[z] into new arrays (timed), then
    the per-level step runs on them.  Its rows carry one more rounding per term, so they are compared with the fused rows
    at 1e-12 x sum |w f| over the weight entries of the resident planes, not in bits;
  * the depth profile (4 against 4 + 4 gathers per record and level) and the tracer row (3 against 5 streams, plus the tracer's
    neighbours) with and without a cell thickness.

    python tools/cellthick_timing.py [--reps N] [--dtype f64|f32] [--json OUT]
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
NX, NY, NZ, NT = 3600, 1800, 75, 2


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
    return dict(median=ms[len(ms) // 2], min=ms[0], max=ms[-1], reps=reps)


def per_step(t):
    return dict(median=t['median'] / NT, min=t['min'] / NT, max=t['max'] / NT, reps=t['reps'])


def with_model(t, nbytes):
    t.update(model_bytes=int(nbytes), fraction_of_8TBps=nbytes / (t['median'] * 1e-3) / PEAK)
    return t


def kernel_split(fld, rows, reps):
    """ms per step of the flux kernel, the expansion behind it and K3, from the library's events around every launch"""
    h = ctypes.byref(fld._h)
    fld.enableKernelTiming(True, reserve=NT)
    flux, expand, k3 = [], [], []
    for r in range(reps + 2):
        check(lib.nf_field_compute_all_async(h, ctypes.c_void_p(rows.data_ptr())))
        n, total, f, e = fld.readKernelTiming(split=True)
        if r >= 2:
            flux.append(f / NT), expand.append(e / NT), k3.append(fld.readTransectTiming() / NT)
    fld.enableKernelTiming(False)

    def spread(x):
        x = sorted(x)
        return dict(median=x[len(x) // 2], min=x[0], max=x[-1], reps=len(x))
    return dict(flux=spread(flux), expand=spread(expand), k3=spread(k3))


def entry_magnitudes(fld):
    """sum |w f| per [segment | transect] over the weight entries, f the resident planes (the last step computed)"""
    n = fld.ny * fld.nx
    iV = numpy.zeros((n, 4))
    check(lib.nf_field_read_step(ctypes.byref(fld._h), _lib.dptr(iV), None, None, None))
    ce, w, sg = fld.getWeights()
    seg = numpy.bincount(sg, weights=numpy.abs(w * iV.reshape(-1)[ce]), minlength=fld._nseg)
    o = fld._tr_off
    return numpy.concatenate([seg, [seg[o[i]:o[i + 1]].sum() for i in range(len(o) - 1)]])


def measure(real, args):
    es = 8 if real == 'float64' else 4
    ncell = NX * NY
    dg = DataGen(real=real)
    dg.setSizes(NX, NY, NZ, NT)
    dg.setBoundingBox(-180., 180., -90., 90., 0., 1.)
    dg.build()
    dg.applyStreamFunction(STREAM_FUNCTIONS[5])
    u, v = dg.computeUVFromPotential()
    polys = bench.make_transects(NX, NY, -180., 180., -90., 90., 64)
    xyzs = [numpy.array([(x, y, 0.) for x, y in p]) for p in polys]
    gen = torch.Generator(device='cuda')
    gen.manual_seed(20261017)
    th = torch.from_numpy(dg.deptht_bounds[:, 1] - dg.deptht_bounds[:, 0]).cuda()[None, :, None, None]

    def thickness():      # the nominal thickness times a partial-cell factor in [0.5, 1]
        f = 0.5 + 0.5 * torch.rand((NT, NZ, NY, NX), generator=gen, dtype=torch.float32, device='cuda')
        return (th * f).to(u.dtype).contiguous()
    e3u, e3v = thickness(), thickness()
    th = th.to(u.dtype)
    tau = (2. + 26. * torch.rand(tuple(u.shape), generator=gen, dtype=torch.float32, device='cuda')).to(u.dtype)
    stream = torch.cuda.current_stream().cuda_stream

    def mk(u, v):
        with contextlib.redirect_stdout(io.StringIO()):
            return Field.fromArrays(dg.bounds_lon, dg.bounds_lat, dg.deptht_bounds, u, v, xyzs, readback=False, stream=stream)
    fld = mk(u, v)
    fld.setTracer(tau, reference=10.)
    h = ctypes.byref(fld._h)
    rows = torch.zeros((NT, fld._rowlen), dtype=torch.float64, device='cuda')
    prof = torch.zeros((NZ, fld._rowlen), dtype=torch.float64, device='cuda')

    def step_pass(f=fld, out=rows):
        check(lib.nf_field_compute_all_async(ctypes.byref(f._h), ctypes.c_void_p(out.data_ptr())))

    k1_bytes = 2 * es * ncell * NZ + (16 + 32 + 16) * ncell
    ct_bytes = 4 * es * ncell * NZ + (16 + 16) * ncell
    res = dict(case=f'bench {NX}x{NY}x{NZ} {real}, nt = {NT}, {len(xyzs)} transects', reps=args.reps)
    # ---- the per-level forms
    plain = dict(step_ms=per_step(timed(step_pass, args.reps)), kernels_ms=kernel_split(fld, rows, args.reps),
                 profile_ms=timed(lambda: check(lib.nf_field_compute_profile_async(h, NT - 1, ctypes.c_void_p(prof.data_ptr()))),
                                  args.reps),
                 tracer_ms=per_step(timed(lambda: check(lib.nf_field_compute_tracer_all_async(h, ctypes.c_void_p(rows.data_ptr()))),
                                          args.reps)))
    with_model(plain['kernels_ms']['flux'], k1_bytes)
    res['per_level'] = plain
    print(json.dumps(dict(case=res['case'], per_level=plain)), flush=True)
    # ---- with a cell thickness; the premultiplied route beside it
    um, vm = torch.empty_like(u), torch.empty_like(v)
    pre = mk(um, vm)
    rows_pre = torch.zeros_like(rows)
    for form in ('static', 'time-varying'):
        a, b = (e3u[:1], e3v[:1]) if form == 'static' else (e3u, e3v)
        fld.setCellThickness(a.contiguous(), b.contiguous())
        c = dict(step_ms=per_step(timed(step_pass, args.reps)), kernels_ms=kernel_split(fld, rows, args.reps))
        with_model(c['kernels_ms']['flux'], ct_bytes)
        step_pass()
        fused = rows.cpu().numpy()
        mag = entry_magnitudes(fld)
        c['profile_ms'] = timed(lambda: check(lib.nf_field_compute_profile_async(h, NT - 1, ctypes.c_void_p(prof.data_ptr()))),
                                args.reps)
        c['tracer_ms'] = per_step(timed(lambda: check(lib.nf_field_compute_tracer_all_async(h, ctypes.c_void_p(rows.data_ptr()))),
                                        args.reps))

        def premultiplied():
            torch.mul(u, a, out=um)
            um.div_(th)
            torch.mul(v, b, out=vm)
            vm.div_(th)
            step_pass(pre, rows_pre)
        c['premultiplied_step_ms'] = per_step(timed(premultiplied, args.reps))
        diff = numpy.abs(rows_pre.cpu().numpy()[NT - 1] - fused[NT - 1])
        c.update(step_over_per_level=c['step_ms']['median'] / plain['step_ms']['median'],
                 kernel_over_k1=c['kernels_ms']['flux']['median'] / plain['kernels_ms']['flux']['median'], kernel_byte_ratio=ct_bytes / k1_bytes,
                 premultiplied_over_fused=c['premultiplied_step_ms']['median'] / c['step_ms']['median'],
                 fused_faster_than_premultiplied=bool(c['step_ms']['max'] < c['premultiplied_step_ms']['min']),
                 premultiplied_max_diff_over_entry_magnitude=float((diff / numpy.maximum(mag, 1e-300)).max()),
                 premultiplied_rows_within_1e12=bool(numpy.all(diff <= 1e-12 * mag)),
                 profile_over_per_level=c['profile_ms']['median'] / plain['profile_ms']['median'], profile_gather_ratio=8 / 4,
                 tracer_over_per_level=c['tracer_ms']['median'] / plain['tracer_ms']['median'], tracer_stream_ratio=5 / 3)
        res[form] = c
        print(json.dumps({'case': res['case'], form: c}), flush=True)
        fld.setCellThickness(None, None)
    del fld, pre
    torch.cuda.empty_cache()
    return res


def main():
    ap = argparse.ArgumentParser(description=__doc__.split('\n')[0])
    ap.add_argument('--reps', type=int, default=10)
    ap.add_argument('--dtype', choices=['f64', 'f32'], default=None)
    ap.add_argument('--json', default='')
    args = ap.parse_args()
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
