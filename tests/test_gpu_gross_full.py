"""Gross transports at the bench shape, 3600 x 1800 x 75 with the seam-crossing batch of tests/test_gpu_resolved_full.py (68
transects, 3.9 million records), HBM-resident and generated on the device, against the sparse reference of
tests/gross_reference.py, which reads the arrays level by level at the cells of the records only.  float64 with 6 steps, checked
at step 5, which starts 2.43e9 elements = 1.9e10 bytes into every array -- beyond 2^31 elements and 2^32 bytes: the carried form
with a time-varying cell thickness, the form with the most gathers and the one no net product covers.  uo / vo are random with
magnitudes in [0.01, 1], either sign, a tenth exactly 0, and a land block of _FillValue / NaN, so that no |q| comes near
underflow (the reference's min_abs_q is asserted); the tracer and the thicknesses are the closed forms of
tests/test_gpu_cellthick_full.py with their marker and NaN blocks.  Bar: 1e-12 x sum |c| per value, every row, level and column
of both parts.  Prints the worst |err| / sum |c| and the times (-s); the README quotes the run time."""
import gc

import numpy
import pytest

import bench
from gross_reference import MIN_ABS_Q, GrossReference
from test_gpu_cellthick_full import BOX, CFILL, CMISSING, FILL, NT, NX, NY, NZ, REF, STEP, THFILL, THMISSING, _closed_forms

pytestmark = pytest.mark.gpu

BAR = 1e-12
THREADS = 12


def _velocities():
    """uo, vo (NT, NZ, NY, NX) float64 on the device, step by step"""
    import torch
    gen = torch.Generator(device='cuda')
    gen.manual_seed(20261017)
    out = []
    for k in range(2):
        a = torch.empty((NT, NZ, NY, NX), dtype=torch.float64, device='cuda')
        for t in range(NT):
            shape = (NZ, NY, NX)
            mag = 0.0101 + (1. - 0.0101) * torch.rand(shape, dtype=torch.float64, device='cuda', generator=gen)
            pick = torch.rand(shape, dtype=torch.float32, device='cuda', generator=gen)
            a[t] = torch.where(pick < 0.1, torch.zeros_like(mag), torch.where(pick < 0.55, mag, -mag))
            del mag, pick
        out.append(a)
    u, v = out
    u[:, 20:, 400:650, 2000:2901] = FILL
    v[:, 20:, 400:650, 2000:2901] = float('nan')
    return u, v


def test_float64_carried_form_with_a_time_varying_cell_thickness_at_step_5():
    import contextlib
    import io
    import time
    import torch
    from nemoflux_amd.datagen import DataGen
    from nemoflux_amd.field import Field
    t_begin = time.time()
    polys = bench.make_transects(NX, NY, *BOX, 64, seed=20260402, seam=True)
    polys.append([(-171.3, -76.2), (172.4, 77.7)])
    xyzs = [numpy.array([(x, y, 0.) for x, y in p]) for p in polys]
    dg = DataGen(real='float64')
    dg.setSizes(NX, NY, NZ, 1)
    dg.setBoundingBox(*BOX, 0., 1.)
    dg.build()
    u, v = _velocities()
    e3u, e3v, tau = _closed_forms()
    arrays = {'uo': u, 'vo': v, 'tracer': tau, 'e3u': e3u, 'e3v': e3v}
    assert STEP * NZ * NY * NX > 2 ** 31 and STEP * NZ * NY * NX * u.element_size() > 2 ** 32
    with contextlib.redirect_stdout(io.StringIO()):
        f = Field.fromArrays(dg.bounds_lon, dg.bounds_lat, dg.deptht_bounds, u, v, xyzs, readback=False, fill_value=FILL)
    f.setTracer(tau, fill_value=CFILL, missing_value=CMISSING, reference=REF, wrapX=True)
    f.setCellThickness(e3u, e3v, fill_value=THFILL, missing_value=THMISSING)
    ce, w, sg = f.getWeights()
    per_seg = numpy.bincount(sg, minlength=f._nseg) // 4
    assert ce.size // 4 > 3_000_000 and per_seg.max() > 4096
    ref = GrossReference(ce, w, sg, f.arcLengths, f.thickness, f._tr_off, NX, NY, uv_markers=(FILL,),
                         tracer_markers=(CFILL, CMISSING), thick_markers=(THFILL, THMISSING), reference=REF, wrap=True,
                         cell_thickness=True)
    cells = torch.from_numpy(ref.cells).cuda()
    t0 = time.time()
    tot, seg = f.computeGrossProfile(STEP, carry=True)
    print(f'computeGrossProfile(carry=True) with its read-back took {time.time() - t0:.2f} s')
    got = numpy.concatenate([seg, tot], axis=-1)
    t0 = time.time()
    want = ref.gross_step(lambda name, z, c: arrays[name][STEP, z].reshape(-1)[cells].cpu().numpy(), threads=THREADS)
    print(f'the reference took {time.time() - t0:.0f} s; smallest non-zero |q| = {want["min_abs_q"]:.3g}')
    assert want['min_abs_q'] >= MIN_ABS_Q
    w_, mag = want['carried']
    assert got.shape == w_.shape == (2, NZ, f._rowlen)
    assert (mag.max(axis=-1) > 0).all(), 'every level must flow both ways in some column'
    worst = float((numpy.abs(got - w_) / numpy.maximum(mag, 1e-300)).max())
    ok = bool(numpy.all(numpy.abs(got - w_) <= BAR * mag))
    del f, dg, u, v, tau, e3u, e3v, arrays, cells
    gc.collect()
    torch.cuda.empty_cache()
    print(f'float64 t={STEP} carried, cell thickness: max |err| / sum |c| = {worst:.3g}; the case took {time.time() - t_begin:.0f} s')
    assert ok, worst
