"""Per-cell layer thicknesses at the bench shape, 3600 x 1800 x 75 float64 with the seam-crossing batch of
tests/test_gpu_resolved_full.py (68 transects, 3.9 million records), HBM-resident and generated on the device, with a
time-varying thickness: 6 steps, checked at step 5, which starts 2.43e9 elements = 1.9e10 bytes into uo, vo, e3u and e3v --
beyond 2^31 elements and 2^32 bytes.  The volume row, the depth profile and the tracer row against the sparse reference of
tests/cellthick_reference.py, which reads the arrays level by level at the cells of the records only.  uo / vo come from the
device generator with a land block of _FillValue / NaN; e3u, e3v and the tracer are closed forms of (t, z, j, i) made slice
by slice, with blocks of their own markers and NaN (on the land block and on wet faces).  About 117 GB of inputs are live
and freed afterwards.  Bar: 1e-12 x sum |terms| per value.

Measured on an MI355X: |err| / mag at most 2.2e-16 (volume row), 3.6e-16 (profile), 2.0e-16 (tracer row); 44 to 47 s, of
which the host reference takes 27 s for the checked step."""
import gc

import numpy
import pytest

import bench
from cellthick_reference import CellThickReference

pytestmark = pytest.mark.gpu

NX, NY, NZ, NT = 3600, 1800, 75, 6
STEP = 5
BOX = (-180., 180., -90., 90.)
FILL = 1.e20                                 # marker of uo / vo (vo's block is NaN)
THFILL, THMISSING = -1.e30, 9.e9             # markers of e3u / e3v
CFILL, CMISSING = 9999., -7777.              # markers of the tracer
REF = 7.5
BAR = 1e-12
THREADS = 12


def _closed_forms():
    """e3u, e3v and the tracer (NT, NZ, NY, NX) float64 on the device, slice by slice; marker / NaN blocks"""
    import torch
    e3u = torch.empty((NT, NZ, NY, NX), dtype=torch.float64, device='cuda')
    e3v = torch.empty_like(e3u)
    tau = torch.empty_like(e3u)
    j = torch.arange(NY, dtype=torch.float64, device='cuda')[:, None]
    i = torch.arange(NX, dtype=torch.float64, device='cuda')[None, :]
    for t in range(NT):
        for z in range(NZ):
            nominal = 1. + 0.2 * z
            e3u[t, z] = nominal * (0.6 + 0.4 * torch.sin(2 * numpy.pi * (7. * i / NX + 0.11 * t)) * torch.cos(2 * numpy.pi * (3. * j / NY + z / 40.)))
            e3v[t, z] = nominal * (0.6 + 0.4 * torch.cos(2 * numpy.pi * (5. * i / NX + z / 60.)) * torch.sin(2 * numpy.pi * (2. * j / NY + 0.13 * t)))
            tau[t, z] = (REF + 6. * torch.cos(2 * numpy.pi * (j / NY + 0.07 * t)) * torch.sin(2 * numpy.pi * (5. * i / NX + z / 50.))
                         + 0.02 * z)
    e3u[:, 20:, 400:650, 2000:2901] = THFILL              # the land block of uo / vo
    e3v[:, 20:, 400:650, 2000:2901] = float('nan')
    e3u[:, 40:, 900:1100, 3300:3600] = float('nan')       # wet faces, up to the last column
    e3v[:, :10, 1300:1500, 0:500] = THMISSING
    tau[:, 5:40, 200:900, 300:1400] = CFILL
    tau[:, 30:, 850:1000, 1700:2000] = float('nan')
    tau[:, :, 1200:1500, 2500:3600] = CMISSING
    return e3u, e3v, tau


def test_float64_six_steps_checked_at_step_5():
    import contextlib
    import io
    import time
    import torch
    from nemoflux_amd.datagen import DataGen, STREAM_FUNCTIONS
    from nemoflux_amd.field import Field
    polys = bench.make_transects(NX, NY, *BOX, 64, seed=20260402, seam=True)
    polys.append([(-171.3, -76.2), (172.4, 77.7)])
    xyzs = [numpy.array([(x, y, 0.) for x, y in p]) for p in polys]
    dg = DataGen(real='float64')
    dg.setSizes(NX, NY, NZ, NT)
    dg.setBoundingBox(*BOX, 0., 1.)
    dg.build()
    dg.applyStreamFunction(STREAM_FUNCTIONS[3])
    u, v = dg.computeUVFromPotential()
    u[:, 20:, 400:650, 2000:2901] = FILL
    v[:, 20:, 400:650, 2000:2901] = float('nan')
    e3u, e3v, tau = _closed_forms()
    arrays = {'uo': u, 'vo': v, 'e3u': e3u, 'e3v': e3v, 'tracer': tau}
    step_elems = NZ * NY * NX
    assert STEP * step_elems > 2 ** 31 and STEP * step_elems * u.element_size() > 2 ** 32
    with contextlib.redirect_stdout(io.StringIO()):
        f = Field.fromArrays(dg.bounds_lon, dg.bounds_lat, dg.deptht_bounds, u, v, xyzs, readback=False, fill_value=FILL)
    f.setCellThickness(e3u, e3v, fill_value=THFILL, missing_value=THMISSING)
    f.setTracer(tau, fill_value=CFILL, missing_value=CMISSING, reference=REF, wrapX=True)
    ce, w, sg = f.getWeights()
    assert ce.size // 4 > 3_000_000
    ref = CellThickReference(ce, w, sg, f.arcLengths, f.thickness, f._tr_off, NX, NY, uv_markers=(FILL,),
                             tracer_markers=(CFILL, CMISSING), thick_markers=(THFILL, THMISSING), reference=REF, wrap=True)
    del ce, w, sg
    cells = torch.from_numpy(ref.cells).cuda()

    def rows(pair):
        return numpy.concatenate([pair[1], pair[0]], axis=-1)

    f.computeFlux(STEP)
    got = {'volume': numpy.array(f._row[:f._rowlen]), 'volume_profile': rows(f.computeFluxProfile(STEP)),
           'tracer': rows(f.computeTracerFlux(STEP))}
    t0 = time.time()
    want = ref.step(lambda name, z, c: arrays[name][STEP, z].reshape(-1)[cells].cpu().numpy(), threads=THREADS)
    print(f'reference took {time.time() - t0:.0f} s')
    worst, ok = {}, True
    for key, g in got.items():
        w_, mag = want[key]
        assert g.shape == w_.shape, key
        assert (mag.max(axis=-1) > 0).all(), f'{key}: every row must carry flux in some column'
        worst[key] = float((numpy.abs(g - w_) / numpy.maximum(mag, 1e-300)).max())
        print(f'{key}: max |err| / mag = {worst[key]:.3g}')
        ok = ok and bool(numpy.all(numpy.abs(g - w_) <= BAR * mag))
    # the thickness of step 5 is not that of step 0: t' = t was read
    static = ref.step(lambda name, z, c: arrays[name][0 if name.startswith('e3') else STEP, z].reshape(-1)[cells].cpu().numpy(),
                      threads=THREADS, tracer=False)['volume'][0]
    assert numpy.abs(static - want['volume'][0]).max() > 1e-3 * numpy.abs(want['volume'][0]).max()
    del f, dg, u, v, e3u, e3v, tau, arrays, cells
    gc.collect()
    torch.cuda.empty_cache()
    assert ok, worst
