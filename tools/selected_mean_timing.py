"""Cost of the time means over selected, weighted steps (nf_time_mean_steps, nf_time_mean_weighted_steps: the kernels behind
Field.timeMean(select=, weights=)), all in one process on one build.

Bench shape 3600 x 1800 x 75 x 12: one velocity series and one thickness series in HBM (93 GB at float64), float64 and float32,
calls with first && last; ms per call, HIP events on the stream of the launches, median with min and max of --reps repetitions
after warm-up, the calls that are compared alternating:
  1. parity: nf_time_mean_steps with unit weights on the offsets j * n beside nf_time_mean on the same series, and the
     thickness-weighted pair.  The kernels are bandwidth-bound and the new ones add one multiply per value, so the bar is the
     existing call's own time in this process plus the spread (max - min) its repeated timings show here;
  2. month-length weights on the same offsets: the same bar against (1);
  3. every other step (6 of 12): half the bytes, so the yardstick is the fraction of the HBM peak reached in (1), not the time;
  4. the same weighted sum written with torch step by step (the same order of operations, so the same bits, which is checked);
  5. a table of 4 x 16 steps (the 12 steps, repeated): the table travels as kernel arguments, 16 steps a launch, so this call
     is four launches that carry acc and cnt between them -- what that traffic costs per byte.
GB/s are over the bytes the definition moves: nsteps * n * sizeof(T) in (twice that for the weighted pair), 8 n (16 n) out,
plus 12 n (28 n) each way per further launch of a chain.

    python tools/selected_mean_timing.py [--reps N] [--dtype f64|f32] [--no-torch] [--out FILE]
"""
import argparse
import ctypes
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy  # noqa: E402
import torch  # noqa: E402

from nemoflux_amd._lib import lib, check, NF_F64, NF_F32, NF_MEAN_OVER_STEPS  # noqa: E402
from weighted_mean_timing import FILL, MISSING, THFILL, THMISSING, HBM_PEAK, NX, NY, NZ, NT, series, timed  # noqa: E402

MONTHS = [31., 28., 31., 30., 31., 30., 31., 31., 30., 31., 30., 31.]
TABLE = 16      # kTmTable of nf_timemean.hip


def table(offsets, weights):
    off = (ctypes.c_longlong * len(offsets))(*offsets)
    w = None if weights is None else (ctypes.c_double * len(weights))(*weights)
    total = 0.0
    for x in (weights or [1.0] * len(offsets)):
        total = total + x
    return off, w, len(offsets), total


def measure(real, args, say):
    dtype = torch.float64 if real == 'float64' else torch.float32
    code, itemsize = (NF_F64, 8) if real == 'float64' else (NF_F32, 4)
    nt, n = NT, NZ * NY * NX
    a, h = series(dtype, nt)
    fill = float(numpy.dtype(real).type(FILL))
    accf = torch.empty(n, dtype=torch.float64, device='cuda')
    acch = torch.empty(n, dtype=torch.float64, device='cuda')
    stream = torch.cuda.current_stream().cuda_stream
    say(f'== time means over selected, weighted steps, {NX} x {NY} x {NZ} x {nt} {real} in HBM, first && last; medians of '
        f'{args.reps} (min - max)')

    def plain():
        check(lib.nf_time_mean(accf.data_ptr(), None, a.data_ptr(), nt, n, n, code, FILL, MISSING, 1, 1, NF_MEAN_OVER_STEPS, nt,
                               fill, stream))

    def weighted():
        check(lib.nf_time_mean_weighted(accf.data_ptr(), acch.data_ptr(), None, a.data_ptr(), n, h.data_ptr(), n, nt, n, code,
                                        FILL, MISSING, THFILL, THMISSING, 1, 1, nt, fill, stream))

    def steps(tab):
        off, w, k, total = tab
        return lambda: check(lib.nf_time_mean_steps(accf.data_ptr(), None, None, a.data_ptr(), off, w, k, n, code, FILL, MISSING,
                                                    1, 1, NF_MEAN_OVER_STEPS, total, fill, stream))

    def wsteps(tab):
        off, w, k, total = tab
        return lambda: check(lib.nf_time_mean_weighted_steps(accf.data_ptr(), acch.data_ptr(), None, a.data_ptr(), off, h.data_ptr(),
                                                             off, w, k, n, code, FILL, MISSING, THFILL, THMISSING, 1, 1, total,
                                                             fill, stream))

    def nbytes(k, two):
        launches = (k + TABLE - 1) // TABLE
        return (2 if two else 1) * k * n * itemsize + (16 if two else 8) * n + (launches - 1) * 2 * (28 if two else 12) * n

    def frac(t, nb):
        return nb / (t[0] * 1e-3) / HBM_PEAK

    def line(label, t, nb, note=''):
        say(f'{label:<62s}{t[0]:9.3f} ms ({t[1]:.3f} - {t[2]:.3f})  {nb / t[0] / 1e6:8.1f} GB/s = {frac(t, nb):.3f} of 8 TB/s{note}')

    def best(calls):
        """every call timed twice, the calls alternating so that all see the same machine; the better median of each"""
        got = [[] for _ in calls]
        for _ in range(2):
            for k, c in enumerate(calls):
                got[k].append(timed(c, args.reps))
        return [min(g) for g in got]

    every = [t * n for t in range(nt)]
    unit, months, half = table(every, None), table(every, MONTHS[:nt]), table(every[::2], MONTHS[:nt:2])
    long = table([every[j % nt] for j in range(4 * TABLE)], [MONTHS[j % 12] for j in range(4 * TABLE)])
    for two, old, new, name in ((False, plain, steps, 'nf_time_mean'), (True, weighted, wsteps, 'nf_time_mean_weighted')):
        t_old, t_unit, t_months, t_half, t_long = best([old, new(unit), new(months), new(half), new(long)])
        nb = nbytes(nt, two)
        bar = t_old[0] + (t_old[2] - t_old[1])
        say(f'-- {name} and {name}_steps, {nb / 1e9:.2f} GB per call over all {nt} steps')
        line(f'{name}', t_old, nb)
        line(f'1. {name}_steps, unit weights, offsets j * n', t_unit, nb)
        line(f'2. {name}_steps, month-length weights', t_months, nb)
        for label, t in (('1. unit weights', t_unit), ('2. month lengths', t_months)):
            say(f'    {label}: {t[0]:.3f} ms against the bar {bar:.3f} ms = {t_old[0]:.3f} + spread {t_old[2] - t_old[1]:.3f}: '
                f'{"met" if t[0] <= bar else "MISSED"} ({t[0] / t_old[0]:.3f} x)')
        line(f'3. every other step (6 of {nt}), month-length weights', t_half, nbytes(len(half[0]), two),
             f'   = {frac(t_half, nbytes(len(half[0]), two)) / frac(t_unit, nb):.3f} of the fraction of (1)')
        line(f'5. {4 * TABLE} steps in 4 launches of {TABLE}', t_long, nbytes(4 * TABLE, two),
             f'   = {frac(t_long, nbytes(4 * TABLE, two)) / frac(t_unit, nb):.3f} of the fraction of (1)')
        if two:
            continue
        if args.no_torch:
            continue
        steps(months)()
        torch.cuda.synchronize()
        got = accf.clone()
        marks = [torch.tensor(m, dtype=dtype, device='cuda') for m in (FILL, MISSING)]
        # a divisor in HBM: torch divides by a Python number through its reciprocal, which is not the quotient's rounding
        total = torch.full((1,), months[3], dtype=torch.float64, device='cuda')
        wdev = [torch.full((), w, dtype=torch.float64, device='cuda') for w in MONTHS[:nt]]
        out = {}

        def torch_steps():
            s = torch.zeros((NZ, NY, NX), dtype=torch.float64, device='cuda')
            c = torch.zeros((NZ, NY, NX), dtype=torch.int32, device='cuda')
            for t in range(nt):
                x = a[t]
                ok = ~(torch.isnan(x) | (x == marks[0]) | (x == marks[1]))
                prod = wdev[t] * x.to(torch.float64)         # rounded, then added
                s = torch.where(ok, s + prod, s)
                c += ok
            out['m'] = torch.where(c > 0, s / total, torch.full((), fill, dtype=torch.float64, device='cuda'))

        t = timed(torch_steps, max(3, args.reps // 3), warm=1)
        line('4. torch, step by step (the same order of operations)', t, nb, f'   = {t[0] / t_months[0]:.2f} x the kernel')
        same = bool(torch.equal(out['m'].reshape(-1).view(torch.int64), got.view(torch.int64)))
        say(f'    the kernel gives the bits of the step-by-step torch form: {same}')
        del got, out
    del a, h, accf, acch
    torch.cuda.empty_cache()


def main():
    ap = argparse.ArgumentParser(description=__doc__.split('\n')[0])
    ap.add_argument('--reps', type=int, default=10)
    ap.add_argument('--dtype', choices=['f64', 'f32'], default=None)
    ap.add_argument('--no-torch', dest='no_torch', action='store_true', help='time the library calls only')
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
