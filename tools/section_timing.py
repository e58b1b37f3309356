"""Cost of the section-area rows (nf_field_compute_area_profile_async) and of the whole throughflow / overturning / gyre split,
all in one process on one build.

For the bench workload (3600 x 1800 x 75, README singular transect + 64 seeded transects, nt = 2), float64 and float32, inputs
in HBM; ms per call, HIP events on the field's stream, median with min and max of --reps repetitions after warm-up:
  * the area profile with each of the two chunk lengths built for the dtype (the "area_chunk" knob), with the scalar thickness
    and with a static cell thickness (4 + 5 and 4 + 4 + 5 gathers per record and level);
  * its yardstick, the tracer profile of the same run (4 + 5 gathers per record and level, one value per level instead of
    two), and for the cell-thickness form that figure times the gather ratio 13 / 9;
  * the whole decomposition of a step: volume profile + area profile + tracer row;
  * for scale, the host restatement of the same two blocks of rows (tests/section_reference.py over Field.getWeights(), the
    values gathered from HBM level by level, --threads host threads), float64 only.

    python tools/section_timing.py [--reps N] [--dtype f64|f32] [--threads N] [--no-host] [--out FILE]
"""
import argparse
import contextlib
import ctypes
import io
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests'))

import numpy  # noqa: E402
import torch  # noqa: E402

import bench  # noqa: E402
from nemoflux_amd._lib import lib, check  # noqa: E402
from nemoflux_amd.datagen import DataGen, STREAM_FUNCTIONS  # noqa: E402
from nemoflux_amd.field import Field  # noqa: E402

NX, NY, NZ, NT = 3600, 1800, 75, 2
CHUNKS = {'float64': (4, 2), 'float32': (8, 4)}     # the default first
REF = 10.0


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
    return ms[len(ms) // 2], ms[0], ms[-1]


def fmt(t):
    return f'{t[0]:8.3f} ms ({t[1]:.3f} - {t[2]:.3f})'


def measure(real, args, say):
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
    f = 0.5 + 0.5 * torch.rand((1, NZ, NY, NX), generator=gen, dtype=torch.float32, device='cuda')
    e3u = (th * f).to(u.dtype).contiguous()
    e3v = (th * (1.5 - f)).to(u.dtype).contiguous()
    del f
    lat = torch.linspace(-89.95, 89.95, NY, dtype=torch.float64, device='cuda')
    z = torch.arange(NZ, dtype=torch.float64, device='cuda')
    base = 2. + 26. * torch.cos(torch.deg2rad(lat))[None, :, None] * torch.exp(-z / 25.)[:, None, None]
    tau = (base[None] + 1.5 * torch.rand(tuple(u.shape), generator=gen, dtype=torch.float32, device='cuda')).to(u.dtype).contiguous()
    stream = torch.cuda.current_stream().cuda_stream
    with contextlib.redirect_stdout(io.StringIO()):
        fld = Field.fromArrays(dg.bounds_lon, dg.bounds_lat, dg.deptht_bounds, u, v, xyzs, readback=False, stream=stream)
    fld.setTracer(tau, reference=REF)
    h = ctypes.byref(fld._h)
    nrec = fld.getWeights()[0].size // 4
    say(f'== bench {NX} x {NY} x {NZ} {real}, nt = {NT}, {len(xyzs)} transects, {nrec} records, row length {fld._rowlen}; '
        f'medians of {args.reps} (min - max)')
    prof = torch.zeros((NZ, fld._rowlen), dtype=torch.float64, device='cuda')
    row = torch.zeros((NT, fld._rowlen), dtype=torch.float64, device='cuda')
    area = torch.zeros((2, NZ, fld._rowlen), dtype=torch.float64, device='cuda')
    p_prof, p_area = ctypes.c_void_p(prof.data_ptr()), ctypes.c_void_p(area.data_ptr())

    def volume_profile():
        check(lib.nf_field_compute_profile_async(h, 0, p_prof))

    def tracer_profile():
        check(lib.nf_field_compute_tracer_profile_async(h, 0, p_prof))

    def area_profile():
        check(lib.nf_field_compute_area_profile_async(h, 0, p_area))

    def tracer_rows():      # nt steps: halved below
        check(lib.nf_field_compute_tracer_all_async(h, ctypes.c_void_p(row.data_ptr())))

    yard = timed(tracer_profile, args.reps)
    say(f'tracer profile (yardstick, 9 gathers per level)          {fmt(yard)}')
    vol = timed(volume_profile, args.reps)
    say(f'volume profile                                           {fmt(vol)}')
    trow = tuple(x / NT for x in timed(tracer_rows, args.reps))
    say(f'tracer row, per step                                     {fmt(trow)}')
    default = {}
    for ct in (False, True):
        if ct:
            fld.setCellThickness(e3u, e3v)
        for chunk in CHUNKS[real]:
            check(lib.nf_tuning_set(b'area_chunk', chunk))
            t = timed(area_profile, args.reps)
            scale = 13. / 9. if ct else 1.
            tag = ' (default)' if chunk == CHUNKS[real][0] else ''
            say(f'area profile, {"static cell thickness, 13" if ct else "scalar thickness, 9"} gathers, {chunk} levels per chunk{tag}'
                f'   {fmt(t)}   = {t[0] / (yard[0] * scale):.2f} x yardstick' + (' x 13/9' if ct else ''))
            if tag:
                default[ct] = t
        check(lib.nf_tuning_set(b'area_chunk', 0))
        if ct:
            volc, trowc = timed(volume_profile, args.reps), tuple(x / NT for x in timed(tracer_rows, args.reps))
            say(f'decomposition of a step with the cell thickness: volume profile {volc[0]:.3f} + area profile {default[ct][0]:.3f} + '
                f'tracer row {trowc[0]:.3f} = {volc[0] + default[ct][0] + trowc[0]:.3f} ms')
            fld.setCellThickness(None, None)
        else:
            say(f'decomposition of a step: volume profile {vol[0]:.3f} + area profile {default[ct][0]:.3f} + tracer row '
                f'{trow[0]:.3f} = {vol[0] + default[ct][0] + trow[0]:.3f} ms')
    if real == 'float64' and not args.no_host:
        from section_reference import SectionReference
        ce, w, sg = fld.getWeights()
        t0 = time.time()
        ref = SectionReference(ce, w, sg, fld.arcLengths, fld.thickness, fld._tr_off, NX, NY, reference=REF, wrap=True)
        cells = torch.from_numpy(ref.cells).cuda()
        arrays = {'uo': u, 'vo': v, 'tracer': tau}
        t1 = time.time()
        want = ref.area_step(lambda name, zz, c: arrays[name][0, zz].reshape(-1)[cells].cpu().numpy(), threads=args.threads)
        t2 = time.time()
        area_profile()
        got = area.cpu().numpy()
        worst = max(float((numpy.abs(got[k] - want[key][0]) / numpy.maximum(want[key][1], 1e-300)).max())
                    for k, key in enumerate(('area_profile', 'tracer_area_profile')))
        say(f'host restatement of the same rows (numpy over getWeights(), {args.threads} threads): setup {t1 - t0:.1f} s + step '
            f'{t2 - t1:.1f} s = {(t2 - t0) * 1e3 / default[False][0]:.0f} x the area profile; worst |err| / mag against it {worst:.3g}')
    del fld
    torch.cuda.empty_cache()


def main():
    ap = argparse.ArgumentParser(description=__doc__.split('\n')[0])
    ap.add_argument('--reps', type=int, default=10)
    ap.add_argument('--dtype', choices=['f64', 'f32'], default=None)
    ap.add_argument('--threads', type=int, default=12)
    ap.add_argument('--no-host', dest='no_host', action='store_true', help='skip the host restatement')
    ap.add_argument('--out', default='', help='also append the lines to this file')
    args = ap.parse_args()

    def say(line):
        print(line, flush=True)
        if args.out:
            with open(args.out, 'a') as fh:
                fh.write(line + '\n')
    for dt, real in (('f64', 'float64'), ('f32', 'float32')):
        if args.dtype and dt != args.dtype:
            continue
        measure(real, args, say)


if __name__ == '__main__':
    main()
