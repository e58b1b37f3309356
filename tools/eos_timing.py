"""Cost of potential density from theta and S (nf_sigma_eos80, the kernel behind nemoflux_amd.eos.Sigma), all in one process on
one build.

One time step of the bench shape, 3600 x 1800 x 75, theta and S in HBM, float64 and float32, pref 0 (sigma0) and 2000 dbar
(sigma2); ms per call, HIP events on the stream of the launches, median with min and max of --reps repetitions after warm-up:
  * nf_sigma_eos80; GB/s over the bytes the definition moves, 3 * n * sizeof(T), and that rate as a fraction of the 8 TB/s HBM
    peak;
  * nf_time_mean of one step of theta alone (n * sizeof(T) in, 8 n out) in the same process: the project's yardstick for a
    streaming pass;
  * the same formulas written with torch on the same tensors (tests/eos_reference.py's expressions, which take tensors as they
    are): what a user can do today without the kernel, with the largest difference from the kernel (torch divides by a Python
    number through its reciprocal, so the last bits may differ);
  * Field.computeClassTransport of that step with 16 class edges and the bench transects, the class field a Sigma (the kernel
    runs at every call) against the same call on the resident sigma array the kernel wrote: host clock around the call, which
    ends with the rows on the host.
About a third of the values are land (theta's _FillValue); NaN is sprinkled over the rest.

    python tools/eos_timing.py [--reps N] [--dtype f64|f32] [--no-field] [--out FILE]
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
import eos_reference as eos  # noqa: E402
from nemoflux_amd._lib import lib, check, NF_F64, NF_F32, NF_MEAN_OVER_PRESENT  # noqa: E402
from nemoflux_amd.datagen import DataGen, STREAM_FUNCTIONS  # noqa: E402
from nemoflux_amd.eos import Sigma  # noqa: E402
from nemoflux_amd.field import Field  # noqa: E402
from timemean_timing import timed  # noqa: E402

NX, NY, NZ = 3600, 1800, 75
FILL = 1.e20
HBM_PEAK = 8.0e12
PREFS = (0., 2000.)


def theta_salt(dtype):
    """(1, NZ, NY, NX) theta and S in HBM: a warm surface and a cold abyss, S around 35; land columns, NaN"""
    gen = torch.Generator(device='cuda')
    gen.manual_seed(20261018)
    th = torch.empty((1, NZ, NY, NX), dtype=dtype, device='cuda')
    sa = torch.empty((1, NZ, NY, NX), dtype=dtype, device='cuda')
    land = torch.rand((NY, NX), generator=gen, device='cuda') < 0.33
    lat = torch.linspace(-89.95, 89.95, NY, dtype=torch.float64, device='cuda')
    for z in range(NZ):
        x = 2. + 26. * torch.cos(torch.deg2rad(lat))[:, None] * float(numpy.exp(-z / 25.)) + \
            1.5 * torch.rand((NY, NX), generator=gen, dtype=torch.float64, device='cuda')
        r = torch.rand((NY, NX), generator=gen, device='cuda')
        x[r < 0.01] = float('nan')
        x[land] = FILL
        th[0, z] = x.to(dtype)
        sa[0, z] = (33. + 3. * torch.rand((NY, NX), generator=gen, dtype=torch.float64, device='cuda')).to(dtype)
    return th, sa


def torch_sigma(th, sa, pref, fill):
    """the formulas with torch: float64 throughout, the presence rule, the final rounding"""
    ok = ~(torch.isnan(th) | (th == fill) | torch.isnan(sa))
    T, S = th.to(torch.float64), sa.to(torch.float64)
    r = torch.sqrt(S)
    if pref == 0.0:
        s = eos.rho0(S, T, r) - 1000.0
    else:
        s = eos.rho(S, eos.ptmp(S, T, 0.0, pref), pref, r) - 1000.0
    return torch.where(ok, s.to(th.dtype), torch.full((), float('nan'), dtype=th.dtype, device='cuda'))


def measure(real, args, say):
    dtype = torch.float64 if real == 'float64' else torch.float32
    code, itemsize = (NF_F64, 8) if real == 'float64' else (NF_F32, 4)
    n = NZ * NY * NX
    th, sa = theta_salt(dtype)
    out = torch.empty_like(th)
    acc = torch.empty(n, dtype=torch.float64, device='cuda')
    stream = torch.cuda.current_stream().cuda_stream
    fill = float(numpy.dtype(real).type(FILL))
    say(f'== one step {NX} x {NY} x {NZ} {real} in HBM; medians of {args.reps} (min - max)')

    def line(label, t, nbytes, note=''):
        say(f'{label:<58s}{t[0]:9.3f} ms ({t[1]:.3f} - {t[2]:.3f})  {nbytes / t[0] / 1e6:8.1f} GB/s = '
            f'{nbytes / (t[0] * 1e-3) / HBM_PEAK:.3f} of 8 TB/s{note}')
        return nbytes / (t[0] * 1e-3) / HBM_PEAK

    def mean():
        check(lib.nf_time_mean(acc.data_ptr(), None, th.data_ptr(), 1, n, n, code, FILL, float('nan'), 1, 1,
                               NF_MEAN_OVER_PRESENT, 1, fill, stream))

    fm = line(f'nf_time_mean of one step of theta ({(n * itemsize + 8 * n) / 1e9:.2f} GB)', timed(mean, args.reps),
              n * itemsize + 8 * n)
    for pref in PREFS:
        def kernel():
            check(lib.nf_sigma_eos80(out.data_ptr(), th.data_ptr(), sa.data_ptr(), n, code, pref, FILL, float('nan'),
                                     float('nan'), float('nan'), float('nan'), stream))

        nbytes = 3 * n * itemsize
        best = timed(kernel, args.reps)
        fk = line(f'nf_sigma_eos80, pref = {pref:g} dbar ({nbytes / 1e9:.2f} GB)', best, nbytes)
        say(f'    fraction of the peak: {fk:.3f}, nf_time_mean {fm:.3f}, ratio {fk / fm:.3f}')
        kernel()
        torch.cuda.synchronize()
        box = {}

        def formulas():
            box['s'] = torch_sigma(th, sa, pref, fill)

        t = timed(formulas, max(3, args.reps // 3), warm=1)
        line('    the same formulas with torch', t, nbytes, f'   = {t[0] / best[0]:.1f} x the kernel')
        d = (box['s'].double() - out.double()).abs()
        both = torch.isnan(box['s']) == torch.isnan(out)
        say(f'    largest |difference| from the kernel {float(d[torch.isfinite(d)].max()):.3g} kg m-3, NaNs in the same places: '
            f'{bool(both.all())}')
        del box, d, both
        torch.cuda.empty_cache()
    del acc
    if not args.no_field:
        field_step(real, th, sa, out, args, say)
    del th, sa, out
    torch.cuda.empty_cache()


def field_step(real, th, sa, sig, args, say):
    """a class step whose class field is a Sigma against the same step on the resident sigma array (pref 0 and 2000)"""
    dg = DataGen(real=real)
    dg.setSizes(NX, NY, NZ, 1)
    dg.setBoundingBox(-180., 180., -90., 90., 0., 1.)
    dg.build()
    dg.applyStreamFunction(STREAM_FUNCTIONS[5])
    u, v = dg.computeUVFromPotential()
    polys = bench.make_transects(NX, NY, -180., 180., -90., 90., 64)
    xyzs = [numpy.array([(x, y, 0.) for x, y in p]) for p in polys]
    with contextlib.redirect_stdout(io.StringIO()):
        fld = Field.fromArrays(dg.bounds_lon, dg.bounds_lat, dg.deptht_bounds, u, v, xyzs, readback=False,
                               stream=torch.cuda.current_stream().cuda_stream)

    def clock(reset):
        ms = []
        for k in range(args.reps + 2):
            if reset:
                fld._tracer['step'] = -1          # compute sigma again, as a new time step would
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            rows = fld.computeClassTransport(0)[0]
            ms.append((time.perf_counter() - t0) * 1e3)
        ms = sorted(ms[2:])
        return (ms[len(ms) // 2], ms[0], ms[-1]), rows

    for pref in PREFS:
        edges = numpy.linspace(20., 29., 16) + (9. if pref else 0.)
        fld.setClassEdges(edges)
        fld.setTracer(Sigma(th, sa, pref, fill_value=FILL))
        a, rows_a = clock(True)
        check(lib.nf_sigma_eos80(sig.data_ptr(), th.data_ptr(), sa.data_ptr(), th.numel(), NF_F32 if real == 'float32' else NF_F64,
                                 pref, FILL, float('nan'), float('nan'), float('nan'), float('nan'), None))
        torch.cuda.synchronize()
        fld.setTracer(sig)
        b, rows_b = clock(False)
        say(f'computeClassTransport, 16 edges, 64 transects, pref = {pref:g}: from a Sigma {a[0]:.3f} ms ({a[1]:.3f} - {a[2]:.3f}), '
            f'from the resident sigma array {b[0]:.3f} ms ({b[1]:.3f} - {b[2]:.3f}); the same rows: '
            f'{bool(numpy.array_equal(rows_a, rows_b))}, classes with water: {int((numpy.abs(rows_b).max(axis=1) > 0).sum())}')
    del fld, u, v, dg
    torch.cuda.empty_cache()


def main():
    ap = argparse.ArgumentParser(description=__doc__.split('\n')[0])
    ap.add_argument('--reps', type=int, default=10)
    ap.add_argument('--dtype', choices=['f64', 'f32'], default=None)
    ap.add_argument('--no-field', action='store_true', help='the kernel, nf_time_mean and the torch formulas only')
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
