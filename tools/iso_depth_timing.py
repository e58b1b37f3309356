"""Cost of the isosurface depth search (nf_iso_depth, the kernel behind nemoflux_amd.surfaces.IsoDepth / MixedLayerDepth), all
in one process on one build.

One time step of the bench shape, 3600 x 1800 x 75, the tracer in HBM, float64 and float32, the thicknesses as the level
vector; ms per call, HIP events on the stream of the launches, median with min and max of --reps repetitions after warm-up:
  (a) a value that is reached nowhere: every column is read to the bed.  GB/s over the bytes the definition moves,
      nz * n * sizeof(T) in and m * n * sizeof(T) out, and that rate as a fraction of the 8 TB/s HBM peak, next to nf_time_mean
      of the same array (n * nz * sizeof(T) in, 8 n nz out) in the same process: the project's yardstick for a streaming pass.
      Target: at least 0.9 x that fraction.  The e3t form (twice the bytes in) is listed too.
  (b) a value crossed inside the top 10 levels everywhere: the wave-wide vote ends the level loop there.  Target: at most
      0.5 x the time of (a).
  (c) m = 8 values in one call against eight calls of one value each.
  (d) the search of (b) written with torch on the same tensor: only the speed-up is reported.
Every output is compared with the numpy restatement of tests/iso_depth_reference.py, 100 rows of the grid at a time so that the
host memory stays small; the count of differing values is printed and is expected to be 0.  --check-stride K compares every
K-th row only (the restatement of all 6.5 million columns takes minutes per output); the line says how many values were
compared.

    python tools/iso_depth_timing.py [--reps N] [--dtype f64|f32] [--check-stride K] [--out FILE]
"""
import argparse
import ctypes
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests'))

import numpy  # noqa: E402
import torch  # noqa: E402

import iso_depth_reference as ref  # noqa: E402
from nemoflux_amd._lib import lib, check, NF_F64, NF_F32, NF_MEAN_OVER_PRESENT  # noqa: E402
from timemean_timing import timed  # noqa: E402

NX, NY, NZ = 3600, 1800, 75
HBM_PEAK = 8.0e12
NAN = float('nan')
THICKNESS = 1.0 + 0.125 * numpy.arange(NZ)          # 1 m at the surface to 10.25 m at the bed
NOWHERE = 1.0e9
SHALLOW = 5.3125                                    # crossed between levels 5 and 6 (or 4 and 5) everywhere
EIGHT = [5.3125 + 9.0 * j for j in range(8)]        # spread from level 5 to level 68
_DP = ctypes.POINTER(ctypes.c_double)


def tracer(dtype):
    """(NZ, NY, NX) in HBM, every level wet: level k holds k + a random number in [0, 0.5) on the lattice of 1 / 64"""
    gen = torch.Generator(device='cuda')
    gen.manual_seed(20261020)
    a = torch.empty((NZ, NY, NX), dtype=dtype, device='cuda')
    for z in range(NZ):
        a[z] = (z + torch.floor(32. * torch.rand((NY, NX), generator=gen, dtype=torch.float64, device='cuda')) / 64.).to(dtype)
    return a


def torch_search(tau, value, c):
    """absolute mode, sense +1, every level wet, with torch: first level that has reached the value, linear between centres"""
    reached = tau >= value
    has = reached.any(dim=0)
    ks = reached.to(torch.uint8).argmax(dim=0)
    a = (ks - 1).clamp(min=0)
    tk = torch.gather(tau, 0, ks[None])[0].double()
    ta = torch.gather(tau, 0, a[None])[0].double()
    ck, ca = c[ks], c[a]
    z = ca + (ck - ca) * ((value - ta) / (tk - ta))
    bed = float(THICKNESS.sum())
    return torch.where(has, torch.where(ks == 0, torch.zeros_like(z), z), torch.full_like(z, bed)).to(tau.dtype)


def measure(real, args, say):
    dtype = torch.float64 if real == 'float64' else torch.float32
    code, itemsize = (NF_F64, 8) if real == 'float64' else (NF_F32, 4)
    n = NY * NX
    tau = tracer(dtype)
    stream = torch.cuda.current_stream().cuda_stream
    hp = numpy.ascontiguousarray(THICKNESS).ctypes.data_as(_DP)
    say(f'== one step {NX} x {NY} x {NZ} {real} in HBM, level vector; medians of {args.reps} (min - max)')

    def line(label, t, nbytes, note=''):
        say(f'{label:<62s}{t[0]:9.3f} ms ({t[1]:.3f} - {t[2]:.3f})  {nbytes / t[0] / 1e6:8.1f} GB/s = '
            f'{nbytes / (t[0] * 1e-3) / HBM_PEAK:.3f} of 8 TB/s{note}')
        return nbytes / (t[0] * 1e-3) / HBM_PEAK

    def search(values, out, e3t=None):
        v = (ctypes.c_double * len(values))(*values)
        check(lib.nf_iso_depth(out.data_ptr(), tau.data_ptr(), None if e3t is not None else hp,
                               None if e3t is None else e3t.data_ptr(), NZ, NY, NX, code, NAN, NAN, NAN, NAN, 0.0,
                               ctypes.cast(v, _DP), len(values), 1, 0, 10.0, NAN, stream))

    def differing(values, out, e3t=None):
        picked = torch.arange(0, NY, args.check_stride, device='cuda')
        nbad = ncompared = 0
        for lo in range(0, picked.numel(), 100):
            rows = picked[lo:lo + 100]
            host = tau[:, rows].cpu().numpy()
            kw = dict(thickness=THICKNESS) if e3t is None else dict(e3t=e3t[:, rows].cpu().numpy())
            want = ref.iso_depth(host, values, 1, **kw)
            got = out[:, rows].cpu().numpy()
            nbad += int((~((got == want) | (numpy.isnan(got) & numpy.isnan(want)))).sum())
            ncompared += got.size
        return f'{nbad} of {ncompared} compared values (of {out.numel()}) differ from the restatement'

    acc = torch.empty(NZ * n, dtype=torch.float64, device='cuda')

    def mean():
        check(lib.nf_time_mean(acc.data_ptr(), None, tau.data_ptr(), 1, NZ * n, NZ * n, code, NAN, NAN, 1, 1, NF_MEAN_OVER_PRESENT,
                               1, NAN, stream))

    fm = line(f'nf_time_mean of the step ({(NZ * n * (itemsize + 8)) / 1e9:.2f} GB)', timed(mean, args.reps), NZ * n * (itemsize + 8))
    del acc
    torch.cuda.empty_cache()

    out1 = torch.empty((1, NY, NX), dtype=dtype, device='cuda')
    bytes_a = (NZ + 1) * n * itemsize
    ta = timed(lambda: search([NOWHERE], out1), args.reps)
    fa = line(f'(a) a value reached nowhere, m = 1 ({bytes_a / 1e9:.2f} GB)', ta, bytes_a)
    say(f'    fraction of the peak: {fa:.3f}, nf_time_mean {fm:.3f}, ratio {fa / fm:.3f} (target >= 0.9: '
        f'{"met" if fa / fm >= 0.9 else "MISSED"}); {differing([NOWHERE], out1)}')
    e3t = torch.from_numpy(THICKNESS.astype(real)).cuda()[:, None, None].expand(NZ, NY, NX).contiguous()
    te = timed(lambda: search([NOWHERE], out1, e3t), args.reps)
    line(f'    the same with e3t ({(2 * NZ + 1) * n * itemsize / 1e9:.2f} GB)', te, (2 * NZ + 1) * n * itemsize)
    search([NOWHERE], out1, e3t)
    torch.cuda.synchronize()
    say(f'    {differing([NOWHERE], out1, e3t)}')
    del e3t
    torch.cuda.empty_cache()

    tb = timed(lambda: search([SHALLOW], out1), args.reps)
    say(f'(b) a value crossed inside the top 10 levels everywhere, m = 1   {tb[0]:9.3f} ms ({tb[1]:.3f} - {tb[2]:.3f})  = '
        f'{tb[0] / ta[0]:.3f} x (a) (target <= 0.5: {"met" if tb[0] / ta[0] <= 0.5 else "MISSED"}); {differing([SHALLOW], out1)}')

    out8 = torch.empty((8, NY, NX), dtype=dtype, device='cuda')
    t8 = timed(lambda: search(EIGHT, out8), args.reps)

    def one_by_one():
        for j, v in enumerate(EIGHT):
            search([v], out8[j:j + 1])

    t1 = timed(one_by_one, args.reps)
    search(EIGHT, out8)
    torch.cuda.synchronize()
    say(f'(c) m = 8 in one call {t8[0]:9.3f} ms ({t8[1]:.3f} - {t8[2]:.3f}), eight calls of m = 1 {t1[0]:9.3f} ms '
        f'({t1[1]:.3f} - {t1[2]:.3f}) = {t1[0] / t8[0]:.2f} x; {differing(EIGHT, out8)}')
    del out8

    D = numpy.concatenate([[0.0], numpy.cumsum(THICKNESS)])
    c = torch.from_numpy(0.5 * (D[:-1] + D[1:])).cuda()
    box = {}

    def formulas():
        box['z'] = torch_search(tau, SHALLOW, c)

    tt = timed(formulas, max(3, args.reps // 3), warm=1)
    search([SHALLOW], out1)
    torch.cuda.synchronize()
    d = (box['z'].double() - out1[0].double()).abs().max()
    say(f'(d) the search of (b) with torch: {tt[0] / tb[0]:.1f} x the kernel\'s time (largest |difference| {float(d):.3g})')
    del box, tau, out1
    torch.cuda.empty_cache()


def main():
    ap = argparse.ArgumentParser(description=__doc__.split('\n')[0])
    ap.add_argument('--reps', type=int, default=10)
    ap.add_argument('--dtype', choices=['f64', 'f32'], default=None)
    ap.add_argument('--check-stride', type=int, default=1, help='compare every K-th row of the grid with the restatement')
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
