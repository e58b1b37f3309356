"""Cost of the z* thicknesses derived from the sea surface height (nf_ssh_thickness, the kernel behind
nemoflux_amd.thickness.SshThickness), all in one process on one build.

One time step of the bench shape, 3600 x 1800 x 75, the statics in HBM, float64 and float32, with and without areas; ms per
call, HIP events on the stream of the launches, median with min and max of --reps repetitions after warm-up:
  * nf_ssh_thickness; GB/s over the bytes the definition moves -- 4 * n * sizeof(T), the two statics in and the two thicknesses
    out, the planes not counted -- and that rate as a fraction of the 8 TB/s HBM peak;
  * nf_sigma_eos80 at pref = 0 on arrays of the same size in the same process, which moves 3 * n * sizeof(T) bytes: the
    yardstick.  The aim is 0.9 x its fraction;
  * nf_face_thickness under 'anomaly', the closest existing route to the same thicknesses, which moves 6 * n * sizeof(T);
  * nf_column_depth of one static, once;
  * the count of values that differ from the numpy restatement (tests/ssh_thickness_reference.py), 100 rows at a time;
  * Field.computeFluxProfile per step in three forms, the steps alternating so that the kernel runs at every call: from an
    SshThickness whose two-step ssh lives on the host (one plane is staged per step), from the resulting e3u / e3v as HBM
    arrays, and from a FaceThickness whose two-step e3t lives on the host (one volume is staged per step): host clock around the
    call, which ends with the rows on the host.
About a third of the columns are land (the statics' _FillValue); NaN and exact zeros are sprinkled over the rest.

    python tools/ssh_thickness_timing.py [--reps N] [--dtype f64|f32] [--no-field] [--no-check] [--out FILE]
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
sys.path.insert(0, os.path.join(ROOT, 'tools'))

import numpy  # noqa: E402
import torch  # noqa: E402

import bench  # noqa: E402
import ssh_thickness_reference as ref  # noqa: E402
from face_thickness_timing import FILL, FILL0, HBM_PEAK, NAN, NX, NY, NZ, thickness  # noqa: E402
from nemoflux_amd._lib import lib, check, NF_F64, NF_F32  # noqa: E402
from nemoflux_amd.datagen import DataGen, STREAM_FUNCTIONS  # noqa: E402
from nemoflux_amd.field import Field  # noqa: E402
from nemoflux_amd.thickness import FaceThickness, SshThickness, column_depth, face_thickness, ssh_thickness  # noqa: E402
from timemean_timing import timed  # noqa: E402


def planes(dtype, seed):
    """(ssh (2, NY, NX) of dtype on the lattice of 1/8 in [-2, 2] with its _FillValue and NaN, the three areas (NY, NX) float64
    on the lattice of 1/4 in [1, 8] with a few NaN and face areas <= 0), in HBM"""
    gen = torch.Generator(device='cuda')
    gen.manual_seed(seed)
    ssh = (torch.randint(-16, 17, (2, NY, NX), generator=gen, device='cuda').to(torch.float64) / 8.)
    r = torch.rand((2, NY, NX), generator=gen, device='cuda')
    ssh[r < 0.01] = NAN
    ssh[(r >= 0.01) & (r < 0.05)] = FILL
    areas = []
    for k in range(3):
        a = torch.randint(4, 33, (NY, NX), generator=gen, device='cuda').to(torch.float64) / 4.
        r = torch.rand((NY, NX), generator=gen, device='cuda')
        a[r < 0.005] = NAN
        if k:
            a[(r >= 0.005) & (r < 0.01)] = 0.0
            a[(r >= 0.01) & (r < 0.015)] = -1.0
        areas.append(a)
    return ssh.to(dtype), tuple(areas)


def differing(got, ssh, e3u0, e3v0, hu0, hv0, areas, rows=100):
    """the number of values of (e3u, e3v) on the host that differ from the numpy restatement, `rows` rows at a time"""
    bad = 0
    for j0 in range(0, NY, rows):
        j1 = min(NY, j0 + rows)
        j2 = min(NY, j1 + 1)              # one more row: the north neighbour of the slab's last row
        sl = slice(j0, j2)
        want = ref.ssh_thickness(ssh[sl], e3u0[:, sl], e3v0[:, sl], hu0[sl], hv0[sl],
                                 None if areas is None else tuple(a[sl] for a in areas), wrap=True, markers=(FILL,),
                                 static_markers=(FILL0,))
        for g, w in zip(got, want):
            a, b = g[:, j0:j1], w[:, :j1 - j0]
            same = ((a == b) & (numpy.signbit(a) == numpy.signbit(b))) | (numpy.isnan(a) & numpy.isnan(b))
            bad += int((~same).sum())
    return bad


def measure(real, args, say):
    dtype = torch.float64 if real == 'float64' else torch.float32
    code, itemsize = (NF_F64, 8) if real == 'float64' else (NF_F32, 4)
    n = NZ * NY * NX
    e3u0, land = thickness(dtype, 1, 20261021, FILL0)
    e3u0 = e3u0[0]
    e3v0 = thickness(dtype, 1, 20261022, FILL0, land)[0][0]
    ssh2, areas = planes(dtype, 20261023)
    ssh = ssh2[0]
    outs = (torch.empty_like(e3u0), torch.empty_like(e3u0))
    stream = torch.cuda.current_stream().cuda_stream
    say(f'== one step {NX} x {NY} x {NZ} {real} in HBM; medians of {args.reps} (min - max)')

    def line(label, t, nbytes, note=''):
        say(f'{label:<58s}{t[0]:9.3f} ms ({t[1]:.3f} - {t[2]:.3f})  {nbytes / t[0] / 1e6:8.1f} GB/s = '
            f'{nbytes / (t[0] * 1e-3) / HBM_PEAK:.3f} of 8 TB/s{note}')
        return nbytes / (t[0] * 1e-3) / HBM_PEAK

    def sigma():
        check(lib.nf_sigma_eos80(outs[0].data_ptr(), e3u0.data_ptr(), e3v0.data_ptr(), n, code, 0.0, FILL0, NAN, FILL0, NAN,
                                 NAN, stream))

    fs = line(f'nf_sigma_eos80, pref = 0, on two of the arrays ({3 * n * itemsize / 1e9:.2f} GB)', timed(sigma, args.reps),
              3 * n * itemsize)
    hu0 = torch.empty((NY, NX), dtype=torch.float64, device='cuda')
    hv0 = torch.empty_like(hu0)
    t = timed(lambda: column_depth(e3u0, (FILL0, NAN), out=hu0, stream=stream), max(3, args.reps // 3), warm=1)
    line(f'nf_column_depth of one static ({n * itemsize / 1e9:.2f} GB)', t, n * itemsize)
    column_depth(e3v0, (FILL0, NAN), out=hv0, stream=stream)
    torch.cuda.synchronize()
    host = None
    if not args.no_check:
        host = [x.cpu().numpy() for x in (ssh, e3u0, e3v0, hu0, hv0) + areas]
    nbytes = 4 * n * itemsize
    for label, ar in (('without areas', None), ('with areas', areas)):
        def kernel():
            ssh_thickness(ssh, e3u0, e3v0, hu0, hv0, areas=ar, wrapX=True, markers=(FILL, NAN), static_markers=(FILL0, NAN),
                          out=outs, stream=stream)

        fk = line(f'nf_ssh_thickness, {label} ({nbytes / 1e9:.2f} GB)', timed(kernel, args.reps), nbytes)
        say(f'    fraction of the peak: {fk:.3f}, nf_sigma_eos80 {fs:.3f}, ratio {fk / fs:.3f} (the aim: 0.9; '
            f'{"met" if fk / fs >= 0.9 else "MISSED"})')
        kernel()
        torch.cuda.synchronize()
        if host is not None:
            got = [o.cpu().numpy() for o in outs]
            t0 = time.perf_counter()
            bad = differing(got, *host[:5], None if ar is None else host[5:])
            moved = sum(int((g != numpy.where(numpy.isnan(s) | (s == s.dtype.type(FILL0)), 0, s)).sum())
                        for g, s in zip(got, host[1:3]))
            say(f'    values that differ from the numpy restatement, 100 rows at a time: {bad} of {2 * n} '
                f'({time.perf_counter() - t0:.0f} s on the host); values that ssh moved off the static: {moved}')
            del got
    del host
    # the closest existing route: the anomaly rule on a full e3t beside its three statics
    e3t = thickness(dtype, 1, 20261024, FILL, land)[0][0]
    e3t0 = thickness(dtype, 1, 20261025, FILL0, land)[0][0]

    def anomaly():
        face_thickness(e3t, 'anomaly', e3t0, e3u0, e3v0, wrapX=True, markers=(FILL, NAN), static_markers=(FILL0, NAN), out=outs,
                       stream=stream)

    line(f'nf_face_thickness, rule anomaly ({6 * n * itemsize / 1e9:.2f} GB)', timed(anomaly, args.reps), 6 * n * itemsize)
    del e3t0
    if not args.no_field:
        field_step(real, ssh2, e3u0, e3v0, e3t, args, say)
    del e3t, e3u0, e3v0, outs
    torch.cuda.empty_cache()


def field_step(real, ssh2, e3u0, e3v0, e3t, args, say):
    """computeFluxProfile whose cell thickness is an SshThickness over a host-resident ssh, the same step on the resident
    e3u / e3v arrays, and a FaceThickness over a host-resident e3t"""
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

    fld.setCellThickness(SshThickness(ssh2.cpu().numpy(), e3u0, e3v0, fill_value=FILL, static_fill_value=FILL0))
    a, rows_a = clock()
    e3u, e3v = torch.empty((2,) + tuple(e3u0.shape), dtype=e3u0.dtype, device='cuda'), None
    e3v = torch.empty_like(e3u)
    hu0, hv0 = column_depth(e3u0, (FILL0, NAN)), column_depth(e3v0, (FILL0, NAN))
    for t in range(2):
        ssh_thickness(ssh2[t], e3u0, e3v0, hu0, hv0, markers=(FILL, NAN), static_markers=(FILL0, NAN), out=(e3u[t], e3v[t]))
    torch.cuda.synchronize()
    fld.setCellThickness(e3u, e3v)
    b, rows_b = clock()
    same = all(numpy.array_equal(x, y) for x, y in zip(rows_a, rows_b))
    del e3u, e3v
    torch.cuda.empty_cache()
    e3t_host = numpy.stack([e3t.cpu().numpy()] * 2)
    fld.setCellThickness(FaceThickness(e3t_host, 'min', fill_value=FILL))
    c, _ = clock()
    say(f'computeFluxProfile, 64 transects: from an SshThickness with ssh on the host {a[0]:.3f} ms ({a[1]:.3f} - {a[2]:.3f}), '
        f'from the resident e3u / e3v arrays {b[0]:.3f} ms ({b[1]:.3f} - {b[2]:.3f}); the same rows: {same}, levels with water: '
        f'{int((numpy.abs(rows_b[0]).max(axis=1) > 0).sum())}; from a FaceThickness with e3t on the host {c[0]:.3f} ms '
        f'({c[1]:.3f} - {c[2]:.3f})')
    fld.setCellThickness(None, None)
    del fld, u, v, dg, e3t_host
    torch.cuda.empty_cache()


def main():
    ap = argparse.ArgumentParser(description=__doc__.split('\n')[0])
    ap.add_argument('--reps', type=int, default=10)
    ap.add_argument('--dtype', choices=['f64', 'f32'], default=None)
    ap.add_argument('--no-field', action='store_true', help='the kernels and nf_sigma_eos80 only')
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
