"""Cost of a joint class step (nf_field_compute_joint_class_transport_async) against the emulation it replaces.

For the bench workload (3600 x 1800 x 75, README singular transect + 64 seeded transects), float64 and float32, with 16 x 16
and 64 x 64 class edges ((nA + 2) * (nB + 2) = 324 and 4356 joint rows): ms per joint step (HIP events on the field's stream,
medians of --reps with min - max, everything in one process) with the block skip on and off ("joint_skip"), and the baseline
measured in the same process: what the library offered before for the same rows, nB + 2 computeClassTransport calls binned by
A over uo / vo masked by the class of B at each U / V face.  Only the device time of the class calls is counted -- the masking
is done outside the events, which favours the baseline.

Checked and printed as it goes: the joint rows' marginals against the 1-D rows binned by A and by B, and the baseline's rows
against the joint rows, each as the largest difference relative to sum |terms| of the value (bar 1e-12; a torch restatement
of the terms on the device gives the sums).  Stage times: the joint call is one gather launch (stage 1) and one binning
launch plus the finalize per window (stage 2); with the skip off every window costs the same, so the two configurations, 11
and 137 windows of 32 rows, give stage 1 and the per-window cost of stage 2 as the intercept and the slope of a line -- an
estimate, printed as such; for the kernels' own times run the tool under rocprofv3 --kernel-trace --stats with
--no-baseline.  --ballast-gb G holds G GB of HBM besides the tool's own arrays while the joint calls run and prints what is
free before and after the first one: whether the term table (11.6 GB here) fits beside the bench's fields.

The tracers are generated on the device from a seeded generator: A temperature-like (class_timing.make_tracer: latitude,
depth and 1.5 degrees of noise; edges evenly spaced over [1, 29]), B salinity-like (longitude, depth and 0.3 of noise; edges
over [33, 37]).  Only the timed step is generated (nt = 1).

    python tools/joint_class_timing.py [--reps N] [--dtype f64|f32] [--classes 16,64] [--no-baseline] [--ballast-gb G]
                                       [--json OUT]
"""
import argparse
import ctypes
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tools'))

import numpy  # noqa: E402
import torch  # noqa: E402

import bench  # noqa: E402
import class_timing  # noqa: E402
from nemoflux_amd._lib import lib, check  # noqa: E402
from nemoflux_amd.datagen import DataGen, STREAM_FUNCTIONS  # noqa: E402

BAR = 1e-12
WINDOW = 32     # nf_tuning_set("joint_window") default


def make_salinity(u, nx, nz):
    gen = torch.Generator(device='cuda')
    gen.manual_seed(20261017)
    lon = torch.linspace(-179.95, 179.95, nx, dtype=torch.float64, device='cuda')
    z = torch.arange(nz, dtype=torch.float64, device='cuda')
    base = 35. + 1.8 * torch.cos(2. * torch.deg2rad(lon))[None, None, :] * torch.exp(-z / 40.)[:, None, None]
    noise = torch.rand(tuple(u.shape), generator=gen, dtype=torch.float64, device='cuda') * 0.3
    return (base[None] + noise).to(u.dtype).contiguous()


def joint_abs_terms(fld, u, v, rows_a, rows_b, na, nb):
    """sum |terms| per (joint row, value) of one step, restated with torch on the device from the weights"""
    ce, w, sg = (torch.from_numpy(x).cuda() for x in fld.getWeights())
    nx = fld.nx
    c, slot = ce // 4, ce % 4
    j, i = c // nx, c % nx
    cell = torch.where(slot == 0, torch.where(j > 0, c - nx, c), torch.where(slot == 3, torch.where(i > 0, c - 1, c - 1 + nx), c))
    ew = (slot == 1) | (slot == 3)
    keep = (slot != 0) | (j > 0)
    arc = torch.from_numpy(fld.arcLengths).cuda()
    a = torch.where(ew, arc[cell, 1], arc[cell, 2])
    th = fld.thickness
    nrow = (na + 2) * (nb + 2)
    mag = torch.zeros(nrow * fld._nseg, dtype=torch.float64, device='cuda')
    for z in range(fld.nz):
        d = torch.where(ew, u[0, z].reshape(-1)[cell].double(), v[0, z].reshape(-1)[cell].double()) * th[z] * a
        ra = torch.where(ew, rows_a[0][0, z].reshape(-1)[cell], rows_a[1][0, z].reshape(-1)[cell]).long()
        rb = torch.where(ew, rows_b[0][0, z].reshape(-1)[cell], rows_b[1][0, z].reshape(-1)[cell]).long()
        mag.index_add_(0, (ra * (nb + 2) + rb) * fld._nseg + sg, torch.where(keep, (w * d).abs(), torch.zeros_like(d)))
    mag = mag.reshape(nrow, fld._nseg).cpu().numpy()
    o = fld._tr_off
    tot = numpy.stack([mag[:, o[p]:o[p + 1]].sum(axis=1) for p in range(len(o) - 1)], axis=1)
    return numpy.concatenate([mag, tot], axis=1).reshape(na + 2, nb + 2, -1)


def timed(step, reps, warm=2):
    stream = torch.cuda.current_stream()
    for _ in range(warm):
        step()
    torch.cuda.synchronize()
    ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(reps)]
    for a, b in ev:
        a.record(stream)
        step()
        b.record(stream)
    torch.cuda.synchronize()
    return [a.elapsed_time(b) for a, b in ev]


def stats(ms):
    ms = sorted(ms)
    return dict(median=ms[len(ms) // 2], min=ms[0], max=ms[-1])


def free_gb():
    free, total = torch.cuda.mem_get_info()
    return free / 1e9, total / 1e9


def measure(name, mk_field, u, v, A, B, args):
    res = []
    fld = mk_field(u, v)
    fld.setTracer(A)
    fld.setClassTracer(B)
    nrec = fld.getWeights()[0].size // 4
    table_gb = 40 * nrec * fld.nz / 1e9
    ballast = None
    if args.ballast_gb > 0:
        ballast = torch.empty(int(args.ballast_gb * 1e9), dtype=torch.uint8, device='cuda')
    first = True
    for n in args.classes:
        eA, eB = numpy.linspace(1., 29., n), numpy.linspace(33., 37., n)
        na = nb = n
        nrow = (na + 2) * (nb + 2)
        fld.setJointClassEdges(eA, eB)
        out = torch.zeros((nrow, fld._rowlen), dtype=torch.float64, device='cuda')

        def joint():
            check(lib.nf_field_compute_joint_class_transport_async(ctypes.byref(fld._h), 0, 0, ctypes.c_void_p(out.data_ptr())))
        r = dict(case=name, edges=f'{n}x{n}', rows=nrow, windows=-(-nrow // WINDOW), row_length=fld._rowlen, records=int(nrec),
                 table_GB=table_gb, reps=args.reps)
        if first:
            before = free_gb()
            try:
                joint()
                torch.cuda.synchronize()
            except RuntimeError as err:
                r.update(error=str(err), free_GB_before=before[0])
                print(json.dumps(r), flush=True)
                return res + [r]
            after = free_gb()
            r.update(ballast_GB=args.ballast_gb, free_GB_before_first_call=before[0], free_GB_after_first_call=after[0],
                     device_GB=before[1])
            first = False
        by_skip = {}
        for skip in (1, 0):
            check(lib.nf_tuning_set(b'joint_skip', skip))
            by_skip[skip] = stats(timed(joint, args.reps))
            if skip:
                rows = out.cpu().numpy().copy()
            else:
                r['skip_off_same_bits'] = bool(numpy.array_equal(out.cpu().numpy().view(numpy.uint64), rows.view(numpy.uint64)))
        check(lib.nf_tuning_set(b'joint_skip', 1))
        r.update(joint_ms_skip_on=by_skip[1], joint_ms_skip_off=by_skip[0],
                 rows_nonzero=int((numpy.abs(rows).max(axis=1) > 0).sum()))
        if not args.no_baseline:
            rows3 = rows.reshape(na + 2, nb + 2, -1)
            rows_a, rows_b = class_timing.face_rows(A, eA), class_timing.face_rows(B, eB)
            mag = joint_abs_terms(fld, u, v, rows_a, rows_b, na, nb)
            del rows_a
            # marginals: the 1-D rows binned by B, then (class tracer cleared) by A
            one = torch.zeros((n + 2, fld._rowlen), dtype=torch.float64, device='cuda')

            def class_step(f=fld):
                check(lib.nf_field_compute_class_transport_async(ctypes.byref(f._h), 0, ctypes.c_void_p(one.data_ptr())))
            fld.setClassEdges(eB)
            class_step()
            by_b = one.cpu().numpy().copy()
            fld.setClassTracer(None)
            fld.setClassEdges(eA)
            class_step()
            by_a = one.cpu().numpy().copy()
            fld.setClassTracer(B)
            rel = lambda d, m: float((numpy.abs(d) / numpy.where(m > 0, m, 1.0)).max())   # noqa: E731
            r.update(marginal_over_b_vs_rows_by_a=rel(rows3.sum(axis=1) - by_a, mag.sum(axis=1)),
                     marginal_over_a_vs_rows_by_b=rel(rows3.sum(axis=0) - by_b, mag.sum(axis=0)))
            # the baseline: nB + 2 class steps binned by A over uo / vo masked by the class of B; its device time only
            um, vm = torch.empty_like(u), torch.empty_like(v)
            emu = mk_field(um, vm)
            emu.setTracer(A)
            emu.setClassEdges(eA)
            totals = numpy.zeros(args.reps)
            base_rows = numpy.zeros_like(rows3)
            for k in range(nb + 2):
                torch.where(rows_b[0] == k, u, torch.zeros_like(u), out=um)
                torch.where(rows_b[1] == k, v, torch.zeros_like(v), out=vm)
                torch.cuda.synchronize()
                totals += numpy.array(timed(lambda: class_step(emu), args.reps, warm=1))
                base_rows[:, k] = one.cpu().numpy()
            del um, vm, emu, rows_b
            base = stats(totals)
            r.update(baseline_ms=base, baseline_vs_joint_rows=rel(base_rows - rows3, mag),
                     speedup_skip_on=base['median'] / by_skip[1]['median'], speedup_skip_off=base['median'] / by_skip[0]['median'])
            r['within_bar'] = bool(max(r['marginal_over_b_vs_rows_by_a'], r['marginal_over_a_vs_rows_by_b'],
                                       r['baseline_vs_joint_rows']) <= BAR)
            r['faster_than_baseline'] = bool(by_skip[1]['median'] < base['median'])
        print(json.dumps(r), flush=True)
        res.append(r)
        del out
        torch.cuda.empty_cache()
    if len(res) == 2:   # stage 1 and the per-window cost of stage 2, skip off: the intercept and the slope over the windows
        (w0, t0), (w1, t1) = [(x['windows'], x['joint_ms_skip_off']['median']) for x in res]
        per_window = (t1 - t0) / (w1 - w0)
        est = dict(case=name, estimate='skip off: T = stage1 + windows * stage2', stage2_ms_per_window=per_window,
                   stage1_ms=t0 - w0 * per_window)
        print(json.dumps(est), flush=True)
        res.append(est)
    del fld, ballast
    torch.cuda.empty_cache()
    return res


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
    A = class_timing.make_tracer(u, ny, nz, -89.95, 89.95)
    B = make_salinity(u, nx, nz)
    r = measure(f'bench {nx}x{ny}x{nz} {real}, {len(xyzs)} transects', class_timing.field_maker(dg, xyzs), u, v, A, B, args)
    del u, v, A, B, dg
    torch.cuda.empty_cache()
    return r


def main():
    ap = argparse.ArgumentParser(description=__doc__.split('\n')[0])
    ap.add_argument('--reps', type=int, default=10)
    ap.add_argument('--dtype', choices=['f64', 'f32'], default=None)
    ap.add_argument('--classes', default='16,64')
    ap.add_argument('--json', default='')
    ap.add_argument('--ballast-gb', dest='ballast_gb', type=float, default=0.0)
    ap.add_argument('--no-baseline', dest='no_baseline', action='store_true', help='joint launches only (for rocprofv3 runs)')
    args = ap.parse_args()
    args.classes = [int(x) for x in args.classes.split(',') if x]
    out = []
    for dt, real in (('f64', 'float64'), ('f32', 'float32')):
        if args.dtype and dt != args.dtype:
            continue
        out += bench_case(real, args)
        if args.json:       # written as it goes: a later case that runs out of time keeps the earlier ones
            with open(args.json, 'w') as f:
                json.dump(out, f, indent=1)
    if not args.no_baseline and not all(x.get('faster_than_baseline', True) and x.get('within_bar', True) for x in out):
        sys.exit('joint_class_timing: a case is not faster than the baseline, or a check misses its bar (see the lines above)')


if __name__ == '__main__':
    main()
