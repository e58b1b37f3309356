"""The resolved products at the bench shape, 3600 x 1800 x 75 with the seam-crossing batch of
test_c5_full_size_seam_crossing_batch plus one two-vertex diagonal (68 transects, 3.9 million records in 15 000 workgroups),
against tests/resolved_reference.py: volume profile, tracer profile, tracer row and the two-tracer class rows with 16 and with
256 edges.  float32 with 6 steps, checked at steps 0 and 5 (step 5 starts 2.43e9 elements = 9.7e9 bytes into each array:
beyond 2^31 elements and 2^32 bytes); float64 with 3 steps, checked at step 2 (7.8e9 bytes in).  A segment holds up to
nx + ny records (more than 64 x 64).  uo / vo come from the device generator (x-periodic psi, menu entry 3) with a land block
of _FillValue / NaN; the carried tracer and the class field are closed forms of (t, z, j, i) made on the device slice by
slice, with blocks of their own markers and NaN.  About 47 GB of inputs are live in either case and freed after it; the
reference reads them level by level at the cells of the records only.  Bar: 1e-12 x sum |terms| per value.

Worst |err| / mag measured on an MI355X: float32 5.3e-16 (steps 0 and 5), float64 3.9e-16 (step 2).
Run time on an MI355X, one run of the whole suite: 85 s (float32, two checked steps) + 45 s (float64, one) = 130 s, of which
the host reference takes 43 to 46 s per checked step and generating and computing on the device about 5 s per case.
tests/test_gpu_baseline_full.py, which moves the same 47-93 GB per case, took between 14 and 19 s in that run (its four
slowest tests 13.6 s together, the other four under 1.4 s each): the device work is of the same order, the reference is what
this file adds."""
import gc

import numpy
import pytest

import bench
from resolved_reference import ResolvedReference

pytestmark = pytest.mark.gpu

NX, NY, NZ = 3600, 1800, 75
BOX = (-180., 180., -90., 90.)
FILL = 1.e20                                 # marker of uo / vo (vo's block is NaN)
TFILL, TMISSING = -32768., 12345.            # markers of the class field
CFILL, CMISSING = 9999., -7777.              # markers of the carried tracer
REF = 7.5
BAR = 1e-12
THREADS = 12
# the class field spans 4 .. 19.7 along every transect: the edges cover its central part, so the open classes at both ends and
# every class between hold faces
EDGE_SETS = [numpy.linspace(7., 16., 16), numpy.linspace(7., 16., 256)]


def _tracers(nt, real):
    """carried tracer and class field (nt, nz, ny, nx) on the device, slice by slice from closed forms; marker / NaN blocks"""
    import torch
    dt = getattr(torch, real)
    tau = torch.empty((nt, NZ, NY, NX), dtype=dt, device='cuda')
    sig = torch.empty((nt, NZ, NY, NX), dtype=dt, device='cuda')
    j = torch.arange(NY, dtype=torch.float64, device='cuda')[:, None]
    i = torch.arange(NX, dtype=torch.float64, device='cuda')[None, :]
    for t in range(nt):
        for z in range(NZ):
            tau[t, z] = (REF + 6. * torch.cos(2 * numpy.pi * (j / NY + 0.07 * t)) * torch.sin(2 * numpy.pi * (5. * i / NX + z / 50.))
                         + 0.02 * z).to(dt)
            sig[t, z] = (10. + 6. * torch.sin(2 * numpy.pi * (3. * i / NX + 0.05 * t)) * torch.cos(2 * numpy.pi * (2. * j / NY + z / 90.))
                         + 0.05 * z).to(dt)
    tau[:, 5:40, 200:900, 300:1400] = CFILL
    tau[:, 30:, 850:1000, 1700:2000] = float('nan')
    tau[:, :, 1200:1500, 2500:3600] = CMISSING            # up to the last column: faces across the seam
    sig[:, 10:60, 700:1100, 1500:2301] = float('nan')     # both sides missing inside the block: the no-value row
    sig[:, :20, 300:600, 0:700] = TFILL                   # from column 0
    sig[:, 50:, 1100:1600, 900:1300] = TMISSING
    return tau, sig


def _run_case(real, nt, steps):
    import contextlib
    import io
    import time
    import torch
    from nemoflux_amd.datagen import DataGen, STREAM_FUNCTIONS
    from nemoflux_amd.field import Field
    polys = bench.make_transects(NX, NY, *BOX, 64, seed=20260402, seam=True)
    polys.append([(-171.3, -76.2), (172.4, 77.7)])
    xyzs = [numpy.array([(x, y, 0.) for x, y in p]) for p in polys]
    dg = DataGen(real=real)
    dg.setSizes(NX, NY, NZ, nt)
    dg.setBoundingBox(*BOX, 0., 1.)
    dg.build()
    dg.applyStreamFunction(STREAM_FUNCTIONS[3])
    u, v = dg.computeUVFromPotential()
    u[:, 20:, 400:650, 2000:2901] = FILL
    v[:, 20:, 400:650, 2000:2901] = float('nan')
    tau, sig = _tracers(nt, real)
    arrays = {'uo': u, 'vo': v, 'tracer': tau, 'class': sig}
    step_elems = NZ * NY * NX
    assert max(steps) * step_elems * u.element_size() > 2 ** 32
    if real == 'float32':
        assert max(steps) * step_elems > 2 ** 31
    with contextlib.redirect_stdout(io.StringIO()):
        f = Field.fromArrays(dg.bounds_lon, dg.bounds_lat, dg.deptht_bounds, u, v, xyzs, readback=False, fill_value=FILL)
    f.setTracer(tau, fill_value=CFILL, missing_value=CMISSING, reference=REF, wrapX=True)
    f.setClassTracer(sig, fill_value=TFILL, missing_value=TMISSING)
    ce, w, sg = f.getWeights()
    per_seg = numpy.bincount(sg, minlength=f._nseg) // 4
    assert ce.size // 4 > 3_000_000 and per_seg.max() > 4096
    ref = ResolvedReference(ce, w, sg, f.arcLengths, f.thickness, f._tr_off, NX, NY, uv_markers=(FILL,),
                            tracer_markers=(CFILL, CMISSING), class_markers=(TFILL, TMISSING), reference=REF, wrap=True)
    del ce, w, sg
    cells = torch.from_numpy(ref.cells).cuda()
    worst = {}

    def check(label, got, pair):
        want, mag = pair
        assert got.shape == want.shape, label
        assert (mag.max(axis=-1) > 0).all(), f'{label}: every row must carry flux in some column'
        ratio = float((numpy.abs(got - want) / numpy.maximum(mag, 1e-300)).max())
        worst[label] = ratio
        print(f'{real} {label}: max |err| / mag = {ratio:.3g}')
        return numpy.all(numpy.abs(got - want) <= BAR * mag)

    def rows(pair):
        return numpy.concatenate([pair[1], pair[0]], axis=-1)

    ok = True
    for t in steps:
        got = {'volume_profile': rows(f.computeFluxProfile(t)), 'tracer_profile': rows(f.computeTracerProfile(t)),
               'tracer': rows(f.computeTracerFlux(t))}
        for k, edges in enumerate(EDGE_SETS):
            f.setClassEdges(edges)
            got['tracer_classes', k] = rows(f.computeClassTracerTransport(t))
        t0 = time.time()
        want = ref.step(lambda name, z, c: arrays[name][t, z].reshape(-1)[cells].cpu().numpy(), EDGE_SETS, threads=THREADS,
                        volume_classes=False)
        print(f'{real} t={t}: reference took {time.time() - t0:.0f} s')
        for key, g in got.items():
            ok = check(f't={t} {key}', g, want[key]) and ok
    del f, dg, u, v, tau, sig, arrays, cells
    gc.collect()
    torch.cuda.empty_cache()
    print(f'{real}: worst |err| / mag = {max(worst.values()):.3g}')
    assert ok, worst


def test_float32_six_steps_checked_at_steps_0_and_5():
    _run_case('float32', 6, (0, 5))


def test_float64_three_steps_checked_at_step_2():
    _run_case('float64', 3, (2,))
