"""Section area and area-weighted tracer at the bench shape, 3600 x 1800 x 75 with the seam-crossing batch of
tests/test_gpu_resolved_full.py (68 transects, 3.9 million records), HBM-resident and generated on the device, against the
sparse reference of tests/section_reference.py, which reads the arrays level by level at the cells of the records only.
float64 with 6 steps, checked at step 5, which starts 2.43e9 elements = 1.9e10 bytes into every array -- beyond 2^31 elements
and 2^32 bytes -- first with the scalar thickness, then with a time-varying cell thickness; float32 with 6 steps, checked at
steps 0 and 5.  uo / vo come from the device generator with a land block of _FillValue / NaN; the tracer and the thicknesses are
the closed forms of tests/test_gpu_cellthick_full.py with their marker and NaN blocks.  Bar: 1e-12 x sum |terms| per value,
every row and column.  Each case prints its worst |err| / mag and the time of its reference (-s); DESIGN.md section 4 quotes
them with the run time."""
import gc

import numpy
import pytest

import bench
from section_reference import SectionReference
from test_gpu_cellthick_full import BOX, CFILL, CMISSING, FILL, NT, NX, NY, NZ, REF, THFILL, THMISSING, _closed_forms
from test_gpu_resolved_full import _tracers

pytestmark = pytest.mark.gpu

BAR = 1e-12
THREADS = 12


def _run_case(real, steps, cell_thickness):
    import contextlib
    import io
    import time
    import torch
    from nemoflux_amd.datagen import DataGen, STREAM_FUNCTIONS
    from nemoflux_amd.field import Field
    t_begin = time.time()
    polys = bench.make_transects(NX, NY, *BOX, 64, seed=20260402, seam=True)
    polys.append([(-171.3, -76.2), (172.4, 77.7)])
    xyzs = [numpy.array([(x, y, 0.) for x, y in p]) for p in polys]
    dg = DataGen(real=real)
    dg.setSizes(NX, NY, NZ, NT)
    dg.setBoundingBox(*BOX, 0., 1.)
    dg.build()
    dg.applyStreamFunction(STREAM_FUNCTIONS[3])
    u, v = dg.computeUVFromPotential()
    u[:, 20:, 400:650, 2000:2901] = FILL
    v[:, 20:, 400:650, 2000:2901] = float('nan')
    if cell_thickness:
        e3u, e3v, tau = _closed_forms()
        arrays = {'uo': u, 'vo': v, 'tracer': tau, 'e3u': e3u, 'e3v': e3v}
        del e3u, e3v
    else:
        tau, sig = _tracers(NT, real)
        del sig
        arrays = {'uo': u, 'vo': v, 'tracer': tau}
    step_elems = NZ * NY * NX
    assert max(steps) * step_elems > 2 ** 31 and max(steps) * step_elems * u.element_size() > 2 ** 32
    with contextlib.redirect_stdout(io.StringIO()):
        f = Field.fromArrays(dg.bounds_lon, dg.bounds_lat, dg.deptht_bounds, u, v, xyzs, readback=False, fill_value=FILL)
    f.setTracer(tau, fill_value=CFILL, missing_value=CMISSING, reference=REF, wrapX=True)
    ce, w, sg = f.getWeights()
    per_seg = numpy.bincount(sg, minlength=f._nseg) // 4
    assert ce.size // 4 > 3_000_000 and per_seg.max() > 4096
    cells = None
    worst, ok = {}, True
    for ct in ((False, True) if cell_thickness else (False,)):
        if ct:
            f.setCellThickness(arrays['e3u'], arrays['e3v'], fill_value=THFILL, missing_value=THMISSING)
        ref = SectionReference(ce, w, sg, f.arcLengths, f.thickness, f._tr_off, NX, NY, uv_markers=(FILL,),
                               tracer_markers=(CFILL, CMISSING), thick_markers=(THFILL, THMISSING), reference=REF, wrap=True,
                               cell_thickness=ct)
        if cells is None:
            cells = torch.from_numpy(ref.cells).cuda()
        for t in steps:
            a, tr = f.computeAreaProfile(t)
            got = numpy.stack([numpy.concatenate([a[1], a[0]], axis=-1), numpy.concatenate([tr[1], tr[0]], axis=-1)])
            t0 = time.time()
            want = ref.area_step(lambda name, z, c: arrays[name][t, z].reshape(-1)[cells].cpu().numpy(), threads=THREADS)
            print(f'{real} t={t} cell thickness {ct}: reference took {time.time() - t0:.0f} s')
            for k, key in enumerate(('area_profile', 'tracer_area_profile')):
                w_, mag = want[key]
                assert got[k].shape == w_.shape, key
                assert (mag.max(axis=-1) > 0).all(), f'{key}: every level must have an area in some column'
                label = f'{real} t={t} {"cell thickness" if ct else "scalar"} {key}'
                worst[label] = float((numpy.abs(got[k] - w_) / numpy.maximum(mag, 1e-300)).max())
                print(f'{label}: max |err| / mag = {worst[label]:.3g}')
                ok = ok and bool(numpy.all(numpy.abs(got[k] - w_) <= BAR * mag))
    del f, dg, u, v, tau, arrays, cells
    gc.collect()
    torch.cuda.empty_cache()
    print(f'{real}: worst |err| / mag = {max(worst.values()):.3g}; the case took {time.time() - t_begin:.0f} s')
    assert ok, worst


def test_float32_six_steps_checked_at_steps_0_and_5():
    _run_case('float32', (0, 5), False)


def test_float64_six_steps_checked_at_step_5_scalar_and_time_varying_cell_thickness():
    _run_case('float64', (5,), True)
