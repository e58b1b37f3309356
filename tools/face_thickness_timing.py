"""Cost of the face thicknesses derived from e3t (nf_face_thickness, the kernel behind nemoflux_amd.thickness.FaceThickness), all in
one process on one build.

One time step of the bench shape, 3600 x 1800 x 75, everything in HBM, float64 and float32, the three rules; ms per call, HIP
events on the stream of the launches, median with min and max of --reps repetitions after warm-up:
  * nf_face_thickness; GB/s over the bytes the definition moves -- 3 * n * sizeof(T) for min and mean, 6 * n * sizeof(T) for
    anomaly -- and that rate as a fraction of the 8 TB/s HBM peak;
  * nf_sigma_eos80 at pref = 0 on arrays of the same size in the same process, which moves 3 * n * sizeof(T) bytes too: the
    yardstick.  The aim is 0.9 x its fraction for min and mean (the row j + 1 is read a second time); the ratio for anomaly is
    recorded without an aim;
  * the same rule written with torch on the same tensors: what a user can do today without the kernel, compared with
    torch.equal;
  * the count of values that differ from the numpy restatement (tests/face_thickness_reference.py), 100 rows at a time;
  * Field.computeFluxProfile per step with a FaceThickness over a two-step e3t in HBM (the kernel runs at every call, the steps
    alternate) beside the same call with the resulting e3u / e3v as HBM arrays: host clock around the call, which ends with the
    rows on the host.
About a third of the columns are land (e3t's _FillValue); NaN and exact zeros are sprinkled over the rest.

    python tools/face_thickness_timing.py [--reps N] [--dtype f64|f32] [--no-field] [--no-check] [--out FILE]
"""
import argparse
import contextlib
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
import face_thickness_reference as ref  # noqa: E402
from nemoflux_amd._lib import lib, check, NF_F64, NF_F32  # noqa: E402
from nemoflux_amd.datagen import DataGen, STREAM_FUNCTIONS  # noqa: E402
from nemoflux_amd.field import Field  # noqa: E402
from nemoflux_amd.thickness import FaceThickness, face_thickness  # noqa: E402
from timemean_timing import timed  # noqa: E402

NX, NY, NZ = 3600, 1800, 75
FILL, FILL0 = 1.e20, -1.e30
HBM_PEAK = 8.0e12
RULES = ('min', 'mean', 'anomaly')
NAN = float('nan')


def thickness(dtype, nt, seed, fill, land=None):
    """(nt, NZ, NY, NX) thicknesses in HBM on the lattice of 1/8 in [0.25, 4]: land columns, NaN and exact zeros"""
    gen = torch.Generator(device='cuda')
    gen.manual_seed(seed)
    a = torch.empty((nt, NZ, NY, NX), dtype=dtype, device='cuda')
    if land is None:
        land = torch.rand((NY, NX), generator=gen, device='cuda') < 0.33
    for t in range(nt):
        for z in range(NZ):
            x = torch.randint(2, 33, (NY, NX), generator=gen, device='cuda').to(torch.float64) / 8.
            r = torch.rand((NY, NX), generator=gen, device='cuda')
            x[r < 0.01] = NAN
            x[(r >= 0.01) & (r < 0.02)] = 0.0
            x[land] = fill
            a[t, z] = x.to(dtype)
    return a, land


def torch_face(e3t, rule, e3t0, e3u0, e3v0, fill, fill0):
    """the rule with torch (wrapX on): float64 throughout, the presence rule, the final rounding"""
    def present(x, m):
        return ~(torch.isnan(x) | (x == m))

    def neighbours(a):
        return torch.roll(a, -1, dims=-1), torch.cat([a[..., 1:, :], a[..., -1:, :]], dim=-2)

    out = []
    pa = present(e3t, fill)
    A = e3t.to(torch.float64)
    zero = torch.zeros((), dtype=torch.float64, device='cuda')
    nbs = neighbours(e3t)
    nbs0 = neighbours(e3t0) if rule == 'anomaly' else (None, None)
    for b, b0, f0 in zip(nbs, nbs0, (e3u0, e3v0)):
        both = pa & present(b, fill)
        B = b.to(torch.float64)
        if rule == 'min':
            r = torch.where(both, torch.where(B < A, B, A), zero)
        elif rule == 'mean':
            r = torch.where(both, 0.5 * (A + B), zero)
        else:
            every = both & present(e3t0, fill0) & present(b0, fill0)
            F0 = f0.to(torch.float64)
            val = F0 + 0.5 * ((A - e3t0.to(torch.float64)) + (B - b0.to(torch.float64)))
            r = torch.where(present(f0, fill0), torch.where(every, val, F0), zero)
        out.append(r.to(e3t.dtype))
    return out


def differing(got, e3t, rule, statics, markers, static_markers, rows=100):
    """the number of values of (e3u, e3v) on the host that differ from the numpy restatement, `rows` rows at a time"""
    bad = 0
    for j0 in range(0, NY, rows):
        j1 = min(NY, j0 + rows)
        j2 = min(NY, j1 + 1)              # one more row: the north neighbour of the slab's last row
        want = ref.face_thickness(e3t[:, j0:j2], rule, *[None if s is None else s[:, j0:j2] for s in statics], wrap=True,
                                  markers=markers, static_markers=static_markers)
        for g, w in zip(got, want):
            a, b = g[:, j0:j1], w[:, :j1 - j0]
            same = ((a == b) & (numpy.signbit(a) == numpy.signbit(b))) | (numpy.isnan(a) & numpy.isnan(b))
            bad += int((~same).sum())
    return bad


def measure(real, args, say):
    dtype = torch.float64 if real == 'float64' else torch.float32
    code, itemsize = (NF_F64, 8) if real == 'float64' else (NF_F32, 4)
    n = NZ * NY * NX
    e3t2, land = thickness(dtype, 2, 20261020, FILL)
    e3t = e3t2[0]
    statics = [thickness(dtype, 1, 20261021 + k, FILL0, land)[0][0] for k in range(3)]
    outs = (torch.empty_like(e3t), torch.empty_like(e3t))
    stream = torch.cuda.current_stream().cuda_stream
    say(f'== one step {NX} x {NY} x {NZ} {real} in HBM; medians of {args.reps} (min - max)')

    def line(label, t, nbytes, note=''):
        say(f'{label:<58s}{t[0]:9.3f} ms ({t[1]:.3f} - {t[2]:.3f})  {nbytes / t[0] / 1e6:8.1f} GB/s = '
            f'{nbytes / (t[0] * 1e-3) / HBM_PEAK:.3f} of 8 TB/s{note}')
        return nbytes / (t[0] * 1e-3) / HBM_PEAK

    def sigma():
        check(lib.nf_sigma_eos80(outs[0].data_ptr(), e3t.data_ptr(), statics[0].data_ptr(), n, code, 0.0, FILL, NAN, FILL0, NAN,
                                 NAN, stream))

    fs = line(f'nf_sigma_eos80, pref = 0, on two of the arrays ({3 * n * itemsize / 1e9:.2f} GB)', timed(sigma, args.reps),
              3 * n * itemsize)
    host = None
    if not args.no_check:
        host = [e3t.cpu().numpy()] + [s.cpu().numpy() for s in statics]
    for rule in RULES:
        st = statics if rule == 'anomaly' else [None, None, None]

        def kernel():
            face_thickness(e3t, rule, *st, wrapX=True, markers=(FILL, NAN), static_markers=(FILL0, NAN), out=outs, stream=stream)

        nbytes = (6 if rule == 'anomaly' else 3) * n * itemsize
        best = timed(kernel, args.reps)
        fk = line(f'nf_face_thickness, rule {rule} ({nbytes / 1e9:.2f} GB)', best, nbytes)
        aim = '' if rule == 'anomaly' else f' (the aim: 0.9; {"met" if fk / fs >= 0.9 else "MISSED"})'
        say(f'    fraction of the peak: {fk:.3f}, nf_sigma_eos80 {fs:.3f}, ratio {fk / fs:.3f}{aim}')
        kernel()
        torch.cuda.synchronize()
        box = {}

        def formulas():
            box['r'] = torch_face(e3t, rule, *st, FILL, FILL0)

        t = timed(formulas, max(3, args.reps // 3), warm=1)
        line('    the same rule with torch', t, nbytes, f'   = {t[0] / best[0]:.1f} x the kernel')
        say(f'    torch.equal with the kernel: e3u {torch.equal(box["r"][0], outs[0])}, e3v {torch.equal(box["r"][1], outs[1])}')
        del box
        torch.cuda.empty_cache()
        if host is not None:
            got = [o.cpu().numpy() for o in outs]
            t0 = time.perf_counter()
            bad = differing(got, host[0], rule, host[1:] if rule == 'anomaly' else [None] * 3, (FILL,), (FILL0,))
            say(f'    values that differ from the numpy restatement, 100 rows at a time: {bad} of {2 * n} '
                f'({time.perf_counter() - t0:.0f} s on the host)')
            del got
    del host
    if not args.no_field:
        field_step(real, e3t2, args, say)
    del e3t2, e3t, statics, outs
    torch.cuda.empty_cache()


def field_step(real, e3t2, args, say):
    """computeFluxProfile whose cell thickness is a FaceThickness against the same step on the resident e3u / e3v arrays"""
    dg = DataGen(real=real)
    dg.setSizes(NX, NY, NZ, 2)
    dg.setBoundingBox(-180., 180., -90., 90., 0., 1.)
    dg.build()
    dg.applyStreamFunction(STREAM_FUNCTIONS[5])
    u, v = dg.computeUVFromPotential()
    polys = bench.make_transects(NX, NY, -180., 180., -90., 90., 64)
    xyzs = [numpy.array([(x, y, 0.) for x, y in p]) for p in polys]
    with contextlib.redirect_stdout(io.StringIO()):
        fld = Field.fromArrays(dg.bounds_lon, dg.bounds_lat, dg.deptht_bounds, u, v, xyzs, readback=False,
                               stream=torch.cuda.current_stream().cuda_stream)

    def clock():
        ms, rows = [], []
        for k in range(args.reps + 2):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            rows.append(fld.computeFluxProfile(k % 2)[0])
            ms.append((time.perf_counter() - t0) * 1e3)
        ms = sorted(ms[2:])
        return (ms[len(ms) // 2], ms[0], ms[-1]), rows[-2:]

    for rule in ('min', 'mean'):
        fld.setCellThickness(FaceThickness(e3t2, rule, fill_value=FILL))
        a, rows_a = clock()
        e3u, e3v = torch.empty_like(e3t2), torch.empty_like(e3t2)
        for t in range(2):
            face_thickness(e3t2[t], rule, markers=(FILL, NAN), out=(e3u[t], e3v[t]))
        torch.cuda.synchronize()
        fld.setCellThickness(e3u, e3v)
        b, rows_b = clock()
        same = all(numpy.array_equal(x, y) for x, y in zip(rows_a, rows_b))
        say(f'computeFluxProfile, 64 transects, rule {rule}: from a FaceThickness {a[0]:.3f} ms ({a[1]:.3f} - {a[2]:.3f}), from the '
            f'resident e3u / e3v arrays {b[0]:.3f} ms ({b[1]:.3f} - {b[2]:.3f}); the same rows: {same}, levels with water: '
            f'{int((numpy.abs(rows_b[0]).max(axis=1) > 0).sum())}')
        fld.setCellThickness(None, None)
        del e3u, e3v
    del fld, u, v, dg
    torch.cuda.empty_cache()


def main():
    ap = argparse.ArgumentParser(description=__doc__.split('\n')[0])
    ap.add_argument('--reps', type=int, default=10)
    ap.add_argument('--dtype', choices=['f64', 'f32'], default=None)
    ap.add_argument('--no-field', action='store_true', help='the kernel, nf_sigma_eos80 and the torch rule only')
    ap.add_argument('--no-check', action='store_true', help='without the count against the numpy restatement')
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
