"""Section area and area-weighted tracer on the GPU (Field.computeAreaProfile, nf_field_compute_area_profile) and the split of a
tracer transport into throughflow, overturning and gyre parts (Field.overturningGyre, decomposeTracerTransport, fluxplot
--decompose).  Every value is checked against the float64 / long-double restatement of the definition in
tests/section_reference.py to 1e-12 x sum |terms|, no row or column left out; anchored bit for bit (tau = ref + 1 gives T = A; the
values of uo / vo and the Sverdrup mode do not matter, only where uo / vo are present; a broadcast cell thickness is the scalar
form; sharded ranks add up; the asynchronous form is the host form); two closed forms; refusals; nothing else is disturbed;
fluxplot --decompose from files.

Grids 72 x 36 x 7 x 3 and 73 x 37 x 7 x 3, float64 and float32, host and HBM inputs, _FillValue, a second marker and NaN in
uo / vo and in the tracer (and +inf in the tracer), wrapX on and off, transects open, closed and across the seam.

Measured on an MI355X: see the figures printed by each test; DESIGN.md section 4 quotes them."""
import ctypes

import numpy
import pytest

from conftest import transect_xyz
from gpu_helpers import _field, _on, _quiet, _rows
from section_reference import SectionReference, array_values
from test_gpu_cellthick import (BAR, DB, FILL, GRIDS, LINES, MISSING, NT, NZ, TFILL, TH, THFILL, THMISSING, TMISSING, _broadcast,
                                _case, _make, _random_thickness, _resident, _row)
from test_gpu_tracer_resolved import H5_LINES, _h5_arrays, _h5_files, _read_csv
from test_section_cpu import ZONAL, zonal_line_area

pytestmark = pytest.mark.gpu

EPS = numpy.finfo(numpy.float64).eps
REF = 4.5


def _tau(real, grid, seed=3):
    """a tracer in [4, 5) with NaN, both markers and +inf (a face value that is not finite) in it"""
    nx, ny = grid
    dt = numpy.dtype(real).type
    tau = (4. + numpy.random.default_rng(seed).random((NT, NZ, ny, nx))).astype(real)
    tau[:, 1::3, 3:-2:3, 2:-2:4] = numpy.nan
    tau[:, :, 10:14, 50:60] = dt(TFILL)
    tau[:, 2:, 25:28, 5:12] = dt(TMISSING)
    tau[:, ::2, 30, 40:43] = numpy.inf
    tau[:, 1, 6, 60:62] = (numpy.inf, -numpy.inf)       # a face whose mean is NaN
    return tau


def _area(f, t, **kw):
    """(2, nz, row_length): A, T as [segments | transects] rows"""
    a, tr = f.computeAreaProfile(t, **kw)
    return numpy.stack([_rows(a), _rows(tr)])


def _reference(f, wrap=True, ref=REF, cell_thickness=False):
    ce, w, sg = f.getWeights()
    return SectionReference(ce, w, sg, f.arcLengths, f.thickness, f._tr_off, f.nx, f.ny, uv_markers=(FILL, MISSING),
                            tracer_markers=(TFILL, TMISSING), thick_markers=(THFILL, THMISSING), reference=ref, wrap=wrap,
                            cell_thickness=cell_thickness)


def _close(got, pair, label):
    want, mag = pair
    assert got.shape == want.shape, label
    err = numpy.abs(got - want)
    worst = float((err / numpy.maximum(mag, 1e-300)).max())
    print(f'{label}: max |err| / mag = {worst:.3g}')
    assert numpy.all(err <= BAR * mag), (label, worst)


def _set_tracer(f, tau, resident, ref=REF, wrap=True):
    f.setTracer(_on(tau, resident), fill_value=TFILL, missing_value=TMISSING, reference=ref, wrapX=wrap)


# ---- 1. against the reference ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize('thick', ['scalar', 'static', 'timevarying'])
@pytest.mark.parametrize('wrap', [True, False], ids=['wrap', 'nowrap'])
@pytest.mark.parametrize('resident', [True, False], ids=['hbm', 'host'])
@pytest.mark.parametrize('grid', GRIDS, ids=lambda g: f'{g[0]}x{g[1]}')
@pytest.mark.parametrize('real', ['float64', 'float32'])
def test_against_the_reference(real, grid, resident, wrap, thick):
    _, _, u, v = _case(real, grid)
    dt = u.dtype.type
    assert numpy.isnan(v).any() and (u == dt(FILL)).any() and (u == dt(MISSING)).any()
    tau = _tau(real, grid)
    f = _make(real, grid, resident, sverdrup=wrap)
    arrays = {'uo': u, 'vo': v, 'tracer': tau}
    if thick != 'scalar':
        e3u, e3v = _random_thickness(real, grid, NT if thick == 'timevarying' else 1, seed=61)
        e3u[:, 4, 12:16, 20:30] = 0          # a thickness of 0 removes the face
        f.setCellThickness(_on(e3u, resident), _on(e3v, resident), fill_value=THFILL, missing_value=THMISSING)
        arrays.update(e3u=e3u, e3v=e3v)
    _set_tracer(f, tau, resident, wrap=wrap)
    r = _reference(f, wrap=wrap, cell_thickness=thick != 'scalar')
    for t in range(NT):
        want = r.area_step(array_values(arrays, t))
        assert want['area_profile'][1][:, -3:].min() > 0, 'every line must have an area on every level'
        got = _area(f, t)
        assert got.shape == (2, NZ, f._rowlen)
        _close(got[0], want['area_profile'], f'area t={t}')
        _close(got[1], want['tracer_area_profile'], f'tracer area t={t}')
        assert (got[0] >= 0).all() and (got[1] < 0).any() and (got[1] > 0).any()


# ---- 2. bit-for-bit anchors ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('thick', ['scalar', 'timevarying'])
@pytest.mark.parametrize('resident', [True, False], ids=['hbm', 'host'])
@pytest.mark.parametrize('grid', GRIDS, ids=lambda g: f'{g[0]}x{g[1]}')
@pytest.mark.parametrize('real', ['float64', 'float32'])
def test_tracer_one_above_the_reference_gives_the_area(real, grid, resident, thick):
    """tau == ref + 1 wherever it is present, ref an integer: x - ref == 1 exactly, so T == A bit for bit"""
    tau = _tau(real, grid)
    tau[numpy.isfinite(tau) & (tau > 0.) & (tau < 100.)] = 8.          # every value that is neither a marker, NaN nor inf
    f = _make(real, grid, resident)
    if thick != 'scalar':
        e3u, e3v = _random_thickness(real, grid, NT, seed=67)
        f.setCellThickness(_on(e3u, resident), _on(e3v, resident), fill_value=THFILL, missing_value=THMISSING)
    _set_tracer(f, tau, resident, ref=7.0)
    for t in range(NT):
        got = _area(f, t)
        assert got[0][:, -3:].min() > 0
        assert numpy.array_equal(got[0], got[1]), t


@pytest.mark.parametrize('resident', [True, False], ids=['hbm', 'host'])
@pytest.mark.parametrize('grid', GRIDS, ids=lambda g: f'{g[0]}x{g[1]}')
@pytest.mark.parametrize('real', ['float64', 'float32'])
def test_only_the_presence_of_the_velocities_matters(real, grid, resident):
    """other values of uo / vo with the same presence pattern, and the Sverdrup mode, leave A and T as they are; another
    presence pattern does not"""
    _, _, u, v = _case(real, grid)
    dt = u.dtype.type
    tau = _tau(real, grid)

    def present(x):
        return ~(numpy.isnan(x) | (x == dt(FILL)) | (x == dt(MISSING)))

    u2, v2 = numpy.where(present(u), (3 * u + 1).astype(real), u), numpy.where(present(v), (v * v - 2).astype(real), v)
    assert not numpy.array_equal(u2[present(u)], u[present(u)]) and numpy.array_equal(present(u2), present(u))
    u3 = u.copy()
    u3[:, :, 12:30, 3:70] = dt(MISSING)
    rows = []
    for uu, vv, sv in ((u, v, False), (u2, v2, False), (u, v, True), (u2, v2, True), (u3, v, False)):
        f = _make(real, grid, resident, u=uu, v=vv, sverdrup=sv)
        _set_tracer(f, tau, resident)
        rows.append(numpy.array([_area(f, t) for t in range(NT)]))
    assert rows[0][:, 0, :, -3:].min() > 0
    for k in (1, 2, 3):
        assert numpy.array_equal(rows[k], rows[0]), k
    assert not numpy.array_equal(rows[4], rows[0])


@pytest.mark.parametrize('nt_th', [1, NT], ids=['static', 'timevarying'])
@pytest.mark.parametrize('resident', [True, False], ids=['hbm', 'host'])
@pytest.mark.parametrize('grid', GRIDS, ids=lambda g: f'{g[0]}x{g[1]}')
@pytest.mark.parametrize('real', ['float64', 'float32'])
def test_broadcast_cell_thickness_is_the_scalar_form(real, grid, resident, nt_th):
    tau = _tau(real, grid)
    a, b = _make(real, grid, resident), _make(real, grid, resident)
    e3 = _broadcast(real, grid, nt_th)
    a.setCellThickness(_on(e3, resident), _on(e3.copy(), resident))
    for f in (a, b):
        _set_tracer(f, tau, resident)
    for t in (1, 0, 2):
        want = _area(b, t)
        assert numpy.abs(want).max() > 0
        assert numpy.array_equal(_area(a, t), want), t
    a.setCellThickness(_on(2 * e3, resident), _on(e3, resident))
    assert not numpy.array_equal(_area(a, 1), _area(b, 1))
    a.setCellThickness(None, None)
    assert numpy.array_equal(_area(a, 1), _area(b, 1))


@pytest.mark.parametrize('thick', ['scalar', 'timevarying'])
@pytest.mark.parametrize('resident', [True, False], ids=['hbm', 'host'])
@pytest.mark.parametrize('real', ['float64', 'float32'])
def test_four_sharded_ranks_add_up_to_the_unsharded_rows(real, resident, thick):
    """slab ranges that cut inside a time step: every level belongs to one rank, the others give exact zeros, so the sum of the
    ranks' rows is the unsharded block bit for bit"""
    from nemoflux_amd.dist import slab_range
    grid, world = GRIDS[0], 4
    tau = _tau(real, grid)
    e3u, e3v = _random_thickness(real, grid, NT, seed=71)

    def make(**kw):
        f = _make(real, grid, resident, **kw)
        if thick != 'scalar':
            f.setCellThickness(_on(e3u, resident), _on(e3v, resident), fill_value=THFILL, missing_value=THMISSING)
        _set_tracer(f, tau, resident)
        return f

    full = make()
    want = numpy.array([_area(full, t) for t in range(NT)])
    acc = numpy.zeros_like(want)
    cut_inside = False
    for rank in range(world):
        sr = slab_range(NT, NZ, rank, world)
        cut_inside = cut_inside or sr[0] % NZ != 0
        part = make(slab_range=sr)
        for t in range(NT):
            got = _area(part, t)
            own = numpy.zeros(NZ, bool)
            lo, hi = max(sr[0], t * NZ), min(sr[1], (t + 1) * NZ)
            if hi > lo:
                own[lo - t * NZ:hi - t * NZ] = True
            assert numpy.all(got[:, ~own] == 0), (rank, t)
            assert numpy.array_equal(got[:, own], want[t][:, own]), (rank, t)
            acc[t] += got
    assert cut_inside and numpy.abs(want).max() > 0
    assert numpy.array_equal(acc, want)


@pytest.mark.parametrize('thick', ['scalar', 'static'])
@pytest.mark.parametrize('resident', [True, False], ids=['hbm', 'host'])
@pytest.mark.parametrize('real', ['float64', 'float32'])
def test_async_form_with_out_is_the_host_form(real, resident, thick):
    import torch
    grid = GRIDS[1]
    f = _make(real, grid, resident)
    if thick != 'scalar':
        e3u, e3v = _random_thickness(real, grid, 1, seed=73)
        f.setCellThickness(_on(e3u, resident), _on(e3v, resident), fill_value=THFILL, missing_value=THMISSING)
    _set_tracer(f, _tau(real, grid), resident)
    shape = (2, NZ, f._rowlen)
    for t in (2, 0):
        want = _area(f, t)
        out = torch.full(shape, numpy.nan, dtype=torch.float64, device='cuda')
        assert numpy.array_equal(_area(f, t, out=out), want) and numpy.abs(want).max() > 0
        assert numpy.array_equal(out.cpu().numpy(), want)
    for bad in (torch.zeros(shape, dtype=torch.float32, device='cuda'), torch.zeros((2, NZ + 1, f._rowlen), dtype=torch.float64,
                                                                                  device='cuda'),
                torch.zeros((2 * NZ, f._rowlen), dtype=torch.float64, device='cuda'), torch.zeros(shape, dtype=torch.float64),
                torch.zeros((2, f._rowlen, NZ), dtype=torch.float64, device='cuda').transpose(1, 2)):
        with pytest.raises(RuntimeError, match='out must be'):
            f.computeAreaProfile(0, out=bad)


# ---- 3. closed forms -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('real', ['float64', 'float32'])
def test_zonal_line_area_through_the_field(real):
    """the zonal line of tests/test_section_cpu.py through the Field: A(z) = th_z x the mean of the south-edge and north-edge
    lengths of the cell row over the span, to 1e-12 relative; with tau = ref + 2 the tracer row is twice that"""
    from nemoflux_amd.datagen import DataGen
    nx, ny = ZONAL['nx'], ZONAL['ny']
    dg = DataGen(real=real)
    dg.setSizes(nx, ny, NZ, 1)
    dg.setBoundingBox(-180., 180., -90., 90., 0., 1.)
    dg.build()
    u = numpy.ones((1, NZ, ny, nx), real)
    f = _field(dg.bounds_lon.cpu().numpy(), dg.bounds_lat.cpu().numpy(), DB, _on(u, True), _on(u.copy(), True),
               [transect_xyz(ZONAL['line'])], readback=False)
    f.setTracer(_on(numpy.full((1, NZ, ny, nx), 5., real), True), reference=3.0)
    (A, _), (T, _) = f.computeAreaProfile(0)
    want = zonal_line_area(f.arcLengths.reshape(-1, 4), nx, ZONAL['row'], ZONAL['i0'], ZONAL['i1'])
    assert abs(want - 1.575423835726685) < 1e-12
    for z in range(NZ):
        rel = abs(A[z, 0] - TH[z] * want) / (TH[z] * want)
        print(f'{real} zonal line level {z}: A = {A[z, 0]!r}, th x closed form = {TH[z] * want!r}, rel err = {rel:.3g}')
        assert rel <= 1e-12
        assert T[z, 0] == 2. * A[z, 0]


@pytest.mark.parametrize('resident', [True, False], ids=['hbm', 'host'])
@pytest.mark.parametrize('grid', GRIDS, ids=lambda g: f'{g[0]}x{g[1]}')
@pytest.mark.parametrize('real', ['float64', 'float32'])
def test_a_tracer_that_depends_on_depth_alone_has_no_gyre_part(real, grid, resident):
    """tau = g(z), present everywhere: the level mean is g(z) - ref to 8 eps |g| and the gyre part vanishes to 1e-12 x sum
    |terms| of the tracer row, for segments and transects, whatever is missing in uo / vo"""
    from resolved_reference import ResolvedReference, array_values as resolved_values
    nx, ny = grid
    _, _, u, v = _case(real, grid)
    g = numpy.array([18.5, 17.25, 14.0, 12.125, 8.5, 6.75, 5.0])       # exact in float32; g - ref has both signs
    ref = 10.0
    tau = numpy.ascontiguousarray(numpy.broadcast_to(g.astype(real)[None, :, None, None], (NT, NZ, ny, nx)))
    f = _make(real, grid, resident, sverdrup=True)
    f.setTracer(_on(tau, resident), reference=ref)
    ce, w, sg = f.getWeights()
    r = ResolvedReference(ce, w, sg, f.arcLengths, f.thickness, f._tr_off, nx, ny, uv_markers=(FILL, MISSING), reference=ref,
                          sverdrup=True)
    arrays = {'uo': u, 'vo': v, 'tracer': tau, 'class': tau}
    for t in range(NT):
        mag = r.step(resolved_values(arrays, t))['tracer'][1]
        V = _rows(f.computeFluxProfile(t))
        A, T = _area(f, t)
        H = _rows(f.computeTracerFlux(t))
        d = f.overturningGyre(V, (A, T), H)
        assert (A[:, -len(LINES):] > 0).all() and (A > 0).mean() > 0.9 and numpy.abs(H).max() > 0
        merr = numpy.where(A > 0, numpy.abs(d['mean'] - (g - ref)[:, None]), 0.0).max(axis=1) / numpy.abs(g)
        worst = float((numpy.abs(d['gyre']) / numpy.maximum(mag, 1e-300)).max())
        print(f't={t}: max |gyre| / mag = {worst:.3g}, max |m(z) - (g - ref)| / |g| = {merr.max():.3g}')
        assert numpy.all(numpy.abs(d['gyre']) <= BAR * mag), worst
        assert numpy.all(merr <= 8 * EPS)
        tot = f.decomposeTracerTransport(t)
        for k in ('total', 'throughflow', 'overturning', 'gyre'):
            assert numpy.array_equal(tot[k], d[k][-len(LINES):]), k
        assert numpy.abs(tot['overturning']).max() > 0 and numpy.abs(tot['throughflow']).max() > 0


# ---- 4. refusals and non-interference --------------------------------------------------------------------------------------
def test_compute_before_set_tracer_is_refused():
    import torch
    from nemoflux_amd._lib import lib
    f = _make('float64', GRIDS[0], True)
    with pytest.raises(RuntimeError, match='setTracer first'):
        f.computeAreaProfile(0)
    with pytest.raises(RuntimeError, match='setTracer first'):
        f.decomposeTracerTransport(0)
    out = torch.zeros((2, NZ, f._rowlen), dtype=torch.float64, device='cuda')
    host = numpy.zeros((2, NZ, f._rowlen))
    assert lib.nf_field_compute_area_profile_async(ctypes.byref(f._h), 0, ctypes.c_void_p(out.data_ptr())) == 2
    assert b'set_tracer first' in lib.nf_last_error()
    assert lib.nf_field_compute_area_profile(ctypes.byref(f._h), 0, host.ctypes.data_as(ctypes.POINTER(ctypes.c_double))) == 2
    assert float(out.abs().max()) == 0 and not host.any()
    f.setTracer(_on(_tau('float64', GRIDS[0]), True), fill_value=TFILL, missing_value=TMISSING)
    assert lib.nf_field_compute_area_profile_async(ctypes.byref(f._h), NT, ctypes.c_void_p(out.data_ptr())) == 1   # time index
    assert b'time index' in lib.nf_last_error()
    assert numpy.abs(_area(f, 0)).max() > 0


@pytest.mark.parametrize('compact', [False, True], ids=['full', 'compact'])
@pytest.mark.parametrize('thick', ['scalar', 'timevarying'])
@pytest.mark.parametrize('resident', [True, False], ids=['hbm', 'host'])
def test_the_area_profile_leaves_everything_else_alone(resident, thick, compact):
    real, grid = 'float64', GRIDS[0]
    a, b = _make(real, grid, resident, compact=compact), _make(real, grid, resident, compact=compact)
    tau = _tau(real, grid)
    for f in (a, b):
        if thick != 'scalar':
            e3u, e3v = _random_thickness(real, grid, NT, seed=79)
            f.setCellThickness(_on(e3u, resident), _on(e3v, resident), fill_value=THFILL, missing_value=THMISSING)
        _set_tracer(f, tau, resident)
    want_all, want_tr = _rows(b.computeAll()), _rows(b.computeTracerAll())
    area1 = _area(a, 1)
    for t in (1, 0, 2):
        assert a.computeFlux(t) == b.computeFlux(t)
        tr = _rows(a.computeTracerFlux(t))
        planes = _resident(a)
        _area(a, (t + 1) % NT), _area(a, t)
        assert numpy.array_equal(_row(a), _row(b)) and numpy.array_equal(_row(a), want_all[t])
        for k, (x, y, z) in enumerate(zip(_resident(a), planes, _resident(b))):
            assert numpy.array_equal(x, y), (t, k)
            assert k == 3 or numpy.array_equal(x, z), (t, k)        # (b's running max has seen every step)
        assert numpy.array_equal(_rows(a.computeTracerFlux(t)), tr) and numpy.array_equal(tr, want_tr[t])
        assert a.computeFlux(t) == b.computeFlux(t)
    _area(a, 0)
    assert numpy.array_equal(_rows(a.computeAll()), want_all)
    _area(a, 2)
    assert numpy.array_equal(_rows(a.computeAll()), want_all)           # a replayed pass where there is one
    assert numpy.array_equal(_rows(a.computeTracerAll()), want_tr)
    assert numpy.array_equal(_area(a, 1), area1)


# ---- 5. files and the command line -----------------------------------------------------------------------------------------
def test_fluxplot_decompose_is_the_field_table(tmp_path):
    """fluxplot --decompose on the HDF5 files with a tracer from an .npz bundle (and, once, cell thicknesses from another):
    the table of the in-memory Field, bit for bit in the returned array and to 15 digits in the CSV"""
    from nemoflux_amd import fluxplot
    files = _h5_files()
    blon, blat, db, u, v, ufill, vfill = _h5_arrays()
    nt, nz, ny, nx = u.shape
    rng = numpy.random.default_rng(83)
    z = numpy.arange(nz)[None, :, None, None]
    lat = numpy.linspace(-1, 1, ny)[None, None, :, None]
    tau = (2. + 20. * numpy.exp(-z / 3.) * (1 - lat * lat) + rng.random(u.shape)).astype(u.dtype)
    tau[:, :, 2:4, 5:9] = u.dtype.type(TFILL)
    tpath = str(tmp_path / 'tracer.npz')
    numpy.savez(tpath, thetao=tau, _FillValue_thetao=numpy.array(TFILL))
    e3u = rng.uniform(0.5, 2., u.shape).astype(u.dtype)
    e3v = rng.uniform(0.5, 2., (1,) + u.shape[1:]).astype(u.dtype)[0]
    epath = str(tmp_path / 'e3.npz')
    numpy.savez(epath, e3u=e3u, e3v=numpy.broadcast_to(e3v, u.shape))
    lines = fluxplot.readTargets(H5_LINES)[0]
    for cell in (False, True):
        mem = _field(blon, blat, db, u, v, lines, True, fill_value=ufill, readback=False)
        if cell:
            mem.setCellThickness(e3u, numpy.ascontiguousarray(numpy.broadcast_to(e3v, u.shape)))
        mem.setTracer(tau, fill_value=TFILL, reference=1.5)
        out = str(tmp_path / f'decompose{int(cell)}.csv')
        kw = dict(cellThickness=True, e3FileU=epath, e3FileV=epath) if cell else {}
        got = _quiet(fluxplot.main, lonLatPoints=H5_LINES, output=out, sverdrup=True, tracer='thetao', tracerFile=tpath,
                     tracerRef=1.5, tracerScale=4.1e-3, decompose=True, **kw, **files)
        assert got.shape == (nt, 4, 2)
        title, header, body = _read_csv(out)
        assert title == '# transport of thetao and its parts [thetao x Sv x 0.0041]'
        assert header == 'time,part,line0,line1' and len(body) == nt * 4
        for t in range(nt):
            d = mem.decomposeTracerTransport(t)
            for k, part in enumerate(('total', 'throughflow', 'overturning', 'gyre')):
                assert numpy.array_equal(got[t, k], d[part] * 4.1e-3), (t, part)
                ln = body[t * 4 + k]
                assert ln[1] == part
                assert numpy.allclose([float(x) for x in ln[2:]], got[t, k], rtol=1e-14, atol=1e-300)
            parts = got[t, 1:]
            assert numpy.all(numpy.abs(parts.sum(axis=0) - got[t, 0]) <= 8 * EPS * numpy.abs(parts).sum(axis=0))
            assert numpy.abs(got[t][[0, 1, 3]]).min() > 0
        if cell:    # (the files' flow is the same on both levels: its overturning part appears with the random thicknesses)
            assert not numpy.array_equal(got, plain) and numpy.abs(got[:, 2]).min() > 1e-6
        plain = got
