"""Cost of the time mean of one array (nf_time_mean, the kernel behind Field.timeMean), all in one process on one build.

Bench shape 3600 x 1800 x 75 x 12, one array in HBM, float64 and float32, one call with first && last (nothing carried); ms per
call, HIP events on the stream of the launches, median with min and max of --reps repetitions after warm-up:
  * nf_time_mean;
  * GB/s over the bytes the definition moves, nsteps * n * sizeof(T) in and 8 n out, and that rate as a fraction of the 8 TB/s
    HBM peak -- the yardstick is K1, the flux kernel, at 0.81 - 0.84 of it;
  * the same masked float64 sum written with torch on the same tensor: step by step (the same order of additions, so the same
    bits, which is checked) and as one masked sum over the step axis (memory permitting).
About a third of the values are land (_FillValue at every step); NaN and a second marker are sprinkled over the rest.

    python tools/timemean_timing.py [--reps N] [--dtype f64|f32] [--nt N] [--out FILE]
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
    """(nt, NZ, NY, NX) in HBM, filled step by step: values of O(1), land columns, NaN and the second marker"""
    gen = torch.Generator(device='cuda')
    gen.manual_seed(20261017)
    a = torch.empty((nt, NZ, NY, NX), dtype=dtype, device='cuda')
    land = torch.rand((NY, NX), generator=gen, device='cuda') < 0.33
    for t in range(nt):
        for z in range(NZ):
            x = torch.randn((NY, NX), generator=gen, dtype=torch.float32, device='cuda')
            r = torch.rand((NY, NX), generator=gen, device='cuda')
            x[r < 0.01] = float('nan')
            x[r > 0.99] = MISSING
            x[land] = FILL
            a[t, z] = x.to(dtype)
    return a


def measure(real, args, say):
    dtype = torch.float64 if real == 'float64' else torch.float32
    code, itemsize = (NF_F64, 8) if real == 'float64' else (NF_F32, 4)
    nt, n = args.nt, NZ * NY * NX
    a = series(dtype, nt)
    fill = float(numpy.dtype(real).type(FILL))
    acc = torch.empty(n, dtype=torch.float64, device='cuda')
    stream = torch.cuda.current_stream().cuda_stream
    nbytes = nt * n * itemsize + 8 * n
    say(f'== time mean of one array {NX} x {NY} x {NZ} x {nt} {real} in HBM, first && last: {nbytes / 1e9:.2f} GB per call '
        f'({nt} x n x {itemsize} in, 8 n out); medians of {args.reps} (min - max)')

    def kernel():
        check(lib.nf_time_mean(acc.data_ptr(), None, a.data_ptr(), nt, n, n, code, FILL, MISSING, 1, 1, NF_MEAN_OVER_STEPS, nt,
                               fill, stream))

    def line(label, t, note=''):
        say(f'{label:<58s}{t[0]:9.3f} ms ({t[1]:.3f} - {t[2]:.3f})  {nbytes / t[0] / 1e6:8.1f} GB/s = '
            f'{nbytes / (t[0] * 1e-3) / HBM_PEAK:.3f} of 8 TB/s{note}')

    best = timed(kernel, args.reps)
    line('nf_time_mean', best)
    kernel()
    torch.cuda.synchronize()
    got = acc.clone()

    m1, m2 = torch.tensor(FILL, dtype=dtype, device='cuda'), torch.tensor(MISSING, dtype=dtype, device='cuda')
    # a divisor in HBM: torch divides by a Python number through its reciprocal, which is not the quotient's rounding
    steps = torch.full((1,), float(nt), dtype=torch.float64, device='cuda')
    out = {}

    def torch_steps():
        s = torch.zeros((NZ, NY, NX), dtype=torch.float64, device='cuda')
        c = torch.zeros((NZ, NY, NX), dtype=torch.int32, device='cuda')
        for t in range(nt):
            x = a[t]
            ok = ~(torch.isnan(x) | (x == m1) | (x == m2))
            s += torch.where(ok, x, torch.zeros((), dtype=dtype, device='cuda')).to(torch.float64)
            c += ok
        out['steps'] = torch.where(c > 0, s / steps, torch.full((), fill, dtype=torch.float64, device='cuda'))

    def torch_one_sum():
        ok = ~(torch.isnan(a) | (a == m1) | (a == m2))
        s = torch.where(ok, a, torch.zeros((), dtype=dtype, device='cuda')).sum(dim=0, dtype=torch.float64)
        out['sum'] = torch.where(ok.any(dim=0), s / steps, torch.full((), fill, dtype=torch.float64, device='cuda'))

    t = timed(torch_steps, max(3, args.reps // 3), warm=1)
    line('torch, step by step (the same order of additions)', t, f'   = {t[0] / best[0]:.2f} x the kernel')
    same = bool(torch.equal(out['steps'].reshape(-1).view(torch.int64), got.view(torch.int64)))
    say(f'    the kernel gives the bits of the step-by-step torch form: {same}')
    try:
        t = timed(torch_one_sum, max(3, args.reps // 3), warm=1)
        line('torch, one masked sum over the step axis', t, f'   = {t[0] / best[0]:.2f} x the kernel')
        d = (out['sum'].reshape(-1) - got).abs()
        say(f'    max |difference| from the kernel (torch chooses the order of additions): {float(d[torch.isfinite(d)].max()):.3g}')
    except torch.cuda.OutOfMemoryError:
        say('torch, one masked sum over the step axis: not measured (out of memory: it holds a masked copy of the series)')
    del a, acc, got, out
    torch.cuda.empty_cache()


def main():
    ap = argparse.ArgumentParser(description=__doc__.split('\n')[0])
    ap.add_argument('--reps', type=int, default=10)
    ap.add_argument('--dtype', choices=['f64', 'f32'], default=None)
    ap.add_argument('--nt', type=int, default=NT)
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
