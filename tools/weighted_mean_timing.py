"""Cost of the thickness-weighted time mean (nf_time_mean_weighted, the kernel behind Field.timeMean(thicknessWeighted=True)),
all in one process on one build.

Bench shape 3600 x 1800 x 75 x 12: one velocity series and one thickness series in HBM (93 GB at float64), float64 and float32,
one call with first && last (nothing carried); ms per call, HIP events on the stream of the launches, median with min and max
of --reps repetitions after warm-up:
  * nf_time_mean_weighted; GB/s over the bytes the definition moves, 2 * nsteps * n * sizeof(T) in and 16 n out, and that rate
    as a fraction of the 8 TB/s HBM peak;
  * nf_time_mean on the velocity series alone (nsteps * n * sizeof(T) in, 8 n out), in the same process: the yardstick.  The
    weighted call moves twice its bytes, so the expectation is the same fraction of the peak, and the ratio of the two
    fractions is written down;
  * the same masked float64 sums written with torch on the same tensors, step by step (the same order of operations, so the
    same bits, which is checked).
About a third of the values are land (_FillValue at every step in the velocity, 0 in the thickness); NaN and a second marker
are sprinkled over the rest of both.

    python tools/weighted_mean_timing.py [--reps N] [--dtype f64|f32] [--nt N] [--no-torch] [--out FILE]
"""
import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy  # noqa: E402
import torch  # noqa: E402

from nemoflux_amd._lib import lib, check, NF_F64, NF_F32, NF_MEAN_OVER_STEPS  # noqa: E402

NX, NY, NZ, NT = 3600, 1800, 75, 12
FILL, MISSING = 1.e20, -999.
THFILL, THMISSING = -1.e30, 9999.
HBM_PEAK = 8.0e12


def timed(call, reps, warm=2):
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


def series(dtype, nt):
    """the velocity and the thickness, (nt, NZ, NY, NX) each in HBM, filled plane by plane: velocities of O(1), thicknesses in
    [0.2, 3], land columns, NaN and the second marker of each"""
    gen = torch.Generator(device='cuda')
    gen.manual_seed(20261018)
    a = torch.empty((nt, NZ, NY, NX), dtype=dtype, device='cuda')
    h = torch.empty((nt, NZ, NY, NX), dtype=dtype, device='cuda')
    land = torch.rand((NY, NX), generator=gen, device='cuda') < 0.33
    for t in range(nt):
        for z in range(NZ):
            x = torch.randn((NY, NX), generator=gen, dtype=torch.float32, device='cuda')
            r = torch.rand((NY, NX), generator=gen, device='cuda')
            x[r < 0.01] = float('nan')
            x[r > 0.99] = MISSING
            x[land] = FILL
            a[t, z] = x.to(dtype)
            e = 0.2 + 2.8 * torch.rand((NY, NX), generator=gen, dtype=torch.float32, device='cuda')
            r = torch.rand((NY, NX), generator=gen, device='cuda')
            e[r < 0.01] = float('nan')
            e[r > 0.99] = THMISSING
            e[(r > 0.98) & (r <= 0.99)] = THFILL
            e[land] = 0.0
            h[t, z] = e.to(dtype)
    return a, h


def measure(real, args, say):
    dtype = torch.float64 if real == 'float64' else torch.float32
    code, itemsize = (NF_F64, 8) if real == 'float64' else (NF_F32, 4)
    nt, n = args.nt, NZ * NY * NX
    a, h = series(dtype, nt)
    fill = float(numpy.dtype(real).type(FILL))
    accf = torch.empty(n, dtype=torch.float64, device='cuda')
    acch = torch.empty(n, dtype=torch.float64, device='cuda')
    stream = torch.cuda.current_stream().cuda_stream
    nbytes = 2 * nt * n * itemsize + 16 * n
    nbytes_one = nt * n * itemsize + 8 * n
    say(f'== thickness-weighted time mean, two series {NX} x {NY} x {NZ} x {nt} {real} in HBM, first && last: {nbytes / 1e9:.2f} GB '
        f'per call (2 x {nt} x n x {itemsize} in, 16 n out); medians of {args.reps} (min - max)')

    def weighted():
        check(lib.nf_time_mean_weighted(accf.data_ptr(), acch.data_ptr(), None, a.data_ptr(), n, h.data_ptr(), n, nt, n, code,
                                        FILL, MISSING, THFILL, THMISSING, 1, 1, nt, fill, stream))

    def plain():
        check(lib.nf_time_mean(accf.data_ptr(), None, a.data_ptr(), nt, n, n, code, FILL, MISSING, 1, 1, NF_MEAN_OVER_STEPS, nt,
                               fill, stream))

    def line(label, t, nb, note=''):
        say(f'{label:<58s}{t[0]:9.3f} ms ({t[1]:.3f} - {t[2]:.3f})  {nb / t[0] / 1e6:8.1f} GB/s = '
            f'{nb / (t[0] * 1e-3) / HBM_PEAK:.3f} of 8 TB/s{note}')

    # the two alternate, so that both see the same machine
    tw, tp = [], []
    for _ in range(2):
        tp.append(timed(plain, args.reps))
        tw.append(timed(weighted, args.reps))
    tw, tp = min(tw), min(tp)
    line('nf_time_mean_weighted', tw, nbytes)
    line(f'nf_time_mean on the velocity alone ({nbytes_one / 1e9:.2f} GB)', tp, nbytes_one)
    fw, fp = nbytes / (tw[0] * 1e-3) / HBM_PEAK, nbytes_one / (tp[0] * 1e-3) / HBM_PEAK
    say(f'    fraction of the peak: weighted {fw:.3f}, nf_time_mean {fp:.3f}, ratio {fw / fp:.3f}; time ratio {tw[0] / tp[0]:.3f} '
        f'for {nbytes / nbytes_one:.3f} x the bytes')
    if args.no_torch:
        del a, h, accf, acch
        torch.cuda.empty_cache()
        return
    weighted()
    torch.cuda.synchronize()
    got_f, got_h = accf.clone(), acch.clone()

    marks = [torch.tensor(m, dtype=dtype, device='cuda') for m in (FILL, MISSING, THFILL, THMISSING)]
    # a divisor in HBM: torch divides by a Python number through its reciprocal, which is not the quotient's rounding
    steps = torch.full((1,), float(nt), dtype=torch.float64, device='cuda')
    zero = torch.zeros((), dtype=torch.float64, device='cuda')
    out = {}

    def torch_steps():
        sF = torch.zeros((NZ, NY, NX), dtype=torch.float64, device='cuda')
        sH = torch.zeros((NZ, NY, NX), dtype=torch.float64, device='cuda')
        c = torch.zeros((NZ, NY, NX), dtype=torch.int32, device='cuda')
        for t in range(nt):
            x, e = a[t], h[t]
            ok = ~(torch.isnan(x) | (x == marks[0]) | (x == marks[1]))
            hh = torch.where(torch.isnan(e) | (e == marks[2]) | (e == marks[3]), zero, e.to(torch.float64))
            sH += hh
            prod = hh * x.to(torch.float64)         # rounded, then added
            sF = torch.where(ok, sF + prod, sF)
            c += ok
        mean = torch.where(sH == 0, zero, sF / sH)
        out['f'] = torch.where(c > 0, mean, torch.full((), fill, dtype=torch.float64, device='cuda'))
        out['h'] = sH / steps

    t = timed(torch_steps, max(3, args.reps // 3), warm=1)
    line('torch, step by step (the same order of operations)', t, nbytes, f'   = {t[0] / tw[0]:.2f} x the kernel')
    same_f = bool(torch.equal(out['f'].reshape(-1).view(torch.int64), got_f.view(torch.int64)))
    same_h = bool(torch.equal(out['h'].reshape(-1).view(torch.int64), got_h.view(torch.int64)))
    say(f'    the kernel gives the bits of the step-by-step torch form: mean velocity {same_f}, mean thickness {same_h}')
    del a, h, accf, acch, got_f, got_h, out
    torch.cuda.empty_cache()


def main():
    ap = argparse.ArgumentParser(description=__doc__.split('\n')[0])
    ap.add_argument('--reps', type=int, default=10)
    ap.add_argument('--dtype', choices=['f64', 'f32'], default=None)
    ap.add_argument('--nt', type=int, default=NT)
    ap.add_argument('--no-torch', dest='no_torch', action='store_true', help='time the two library calls only')
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
