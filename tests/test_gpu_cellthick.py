"""Per-cell layer thicknesses on the GPU (Field.setCellThickness, nf_field_set_cell_thickness): e3u / e3v read at the face in
place of the one thickness per level.  Anchored bit for bit to the per-level path (thickness broadcast over the grid; a
staircase mask against masked velocities), the profile rows anchored to the volume rows, everything checked against the
float64 / long-double restatement of the definition in tests/cellthick_reference.py and against the closed form of a
z-independent stream function; sharded ranks add up; refusals; file-backed thicknesses and fluxplot --cell-thickness.

Grids 72 x 36 x 7 x 3 and 73 x 37 x 7 x 3 (odd: the one-cell-per-lane kernels), transects open, closed and across the seam.

Measured on an MI355X: worst |err| / sum |terms| against the definition 2.7e-16 (bar 1e-12), sharded sums 3.3e-16, closed form
2.6e-16 relative at float64 (bar 1e-12) and 7.0e-9 at float32 (bar 1e-6: the velocities' own float32 rounding)."""
import ctypes
import os

import numpy
import pytest

from conftest import transect_xyz
from cellthick_reference import CellThickReference, array_values
from gpu_helpers import _field, _on, _quiet, _rows

pytestmark = pytest.mark.gpu

PSI_ZT = "(1+10*z)*(t+1)*(cos(2*pi*y/360) + sin(2*pi*x/360))"
PSI_XY = "cos(2*pi*y/360) + sin(2*pi*x/360)"
T_TRI = "(-100,-80),(100,-80),(0,80),(-100,-80)"
T_OPEN = "(-100,-80),(100,-80),(0,80)"
T_SEAM = "(150,-30),(179.5,-20),(179.9,10),(175,40)"     # the east faces of the last column
NZ, NT = 7, 3
GRIDS = [(72, 36), (73, 37)]
FILL, MISSING = 1.e20, -999.             # uo / vo
THFILL, THMISSING = -1.e30, 9.e9         # e3u / e3v
TFILL, TMISSING = -32768., 12345.        # tracer
BAR = 1e-12
# thicknesses that float32 holds exactly, and bounds whose differences are those numbers exactly (sums of dyadic fractions)
TH = numpy.array([0.125, 0.25, 0.5, 0.375, 0.75, 1.0, 0.625])
DB = numpy.stack([numpy.concatenate([[0.], numpy.cumsum(TH)[:-1]]), numpy.cumsum(TH)], axis=1)


_CASES = {}


def _case(real, grid=GRIDS[0], psi=PSI_ZT, fill=True):
    """bounds and host u, v (nt, nz, ny, nx); with `fill`, land blocks of _FillValue, NaN and a second missing value"""
    key = (real, grid, psi, fill)
    if key not in _CASES:
        from nemoflux_amd.datagen import DataGen
        nx, ny = grid
        dg = DataGen(real=real)
        dg.setSizes(nx, ny, NZ, NT)
        dg.setBoundingBox(-180., 180., -90., 90., 0., 1.)
        dg.build()
        dg.applyStreamFunction(psi)
        dg.computeUVFromPotential()
        u, v = dg.u.cpu().numpy().copy(), dg.v.cpu().numpy().copy()
        v[:, :, -1, :] = 0                     # the generator's pole row is 1e13-sized garbage
        if fill:
            dt = u.dtype.type
            u[:, 3:, 4:9, 10:20] = dt(FILL)
            v[:, 3:, 4:9, 10:20] = numpy.nan
            u[:, :2, 20:24, 30:40] = dt(MISSING)
            v[:, 5:, 20:24, 30:40] = dt(MISSING)
        _CASES[key] = (dg.bounds_lon.cpu().numpy(), dg.bounds_lat.cpu().numpy(), u, v)
    return _CASES[key]


LINES = [T_OPEN, T_TRI, T_SEAM]


def _make(real, grid, resident, u=None, v=None, **kw):
    blon, blat, u0, v0 = _case(real, grid)
    kw.setdefault('readback', False)
    kw.setdefault('fill_value', FILL)
    kw.setdefault('missing_value', MISSING)
    return _field(blon, blat, DB, _on(u0 if u is None else u, resident), _on(v0 if v is None else v, resident),
                  [transect_xyz(s) for s in LINES], **kw)


def _row(f):
    return numpy.array(f._row[:f._rowlen])


def _resident(f):
    from nemoflux_amd import _lib
    from nemoflux_amd._lib import lib, check
    n = f.ny * f.nx
    iV, eU, eV, mx = numpy.zeros((n, 4)), numpy.zeros(n), numpy.zeros(n), ctypes.c_double()
    check(lib.nf_field_read_step(ctypes.byref(f._h), _lib.dptr(iV), _lib.dptr(eU), _lib.dptr(eV), ctypes.byref(mx)))
    return iV, eU, eV, numpy.array(mx.value)


def _broadcast(real, grid, nt_th):
    nx, ny = grid
    return numpy.ascontiguousarray(numpy.broadcast_to(TH.astype(real)[None, :, None, None], (nt_th, NZ, ny, nx)))


def _tracer(real, grid, seed=3):
    nx, ny = grid
    tau = (4. + numpy.random.default_rng(seed).random((NT, NZ, ny, nx))).astype(real)
    tau[:, 1::3, 3:-2:3, 2:-2:4] = numpy.nan
    return tau


def _random_thickness(real, grid, nt_th, seed, markers=True):
    """thicknesses in [0.2, 3] that differ per cell, level and step; with `markers`, all three kinds on the land block of
    uo / vo and on isolated wet faces"""
    nx, ny = grid
    rng = numpy.random.default_rng(seed)
    dt = numpy.dtype(real).type
    e3u = rng.uniform(0.2, 3., (nt_th, NZ, ny, nx)).astype(real)
    e3v = rng.uniform(0.2, 3., (nt_th, NZ, ny, nx)).astype(real)
    if markers:
        e3u[:, 3:, 4:9, 10:15] = dt(THFILL)
        e3u[:, 3:, 4:9, 15:20] = numpy.nan
        e3v[:, 3:, 4:9, 10:20] = dt(THMISSING)
        for k, m in enumerate((THFILL, THMISSING, numpy.nan)):
            e3u[:, k::3, 2 + k:-2:3, 2:-2:4] = dt(m)
            e3v[:, (k + 1) % 3::3, 2 + k:-2:3, 3:-2:4] = dt(m)
    return e3u, e3v


def _reference(f, wrap=True, ref=0.0, sverdrup=False):
    ce, w, sg = f.getWeights()
    return CellThickReference(ce, w, sg, f.arcLengths, f.thickness, f._tr_off, f.nx, f.ny, uv_markers=(FILL, MISSING),
                              tracer_markers=(TFILL, TMISSING), thick_markers=(THFILL, THMISSING), reference=ref, wrap=wrap,
                              sverdrup=sverdrup)


def _close(got, pair, label=''):
    want, mag = pair
    assert got.shape == want.shape, label
    err = numpy.abs(got - want)
    print(f'{label}: max |err| / mag = {float((err / numpy.maximum(mag, 1e-300)).max()):.3g}')
    assert numpy.all(err <= BAR * mag), (label, float((err / numpy.maximum(mag, 1e-300)).max()))


# ---- 1. thickness broadcast: the per-level path, bit for bit ---------------------------------------------------------------
@pytest.mark.parametrize('compact', [False, True], ids=['full', 'compact'])
@pytest.mark.parametrize('sverdrup', [False, True], ids=['m2', 'sv'])
@pytest.mark.parametrize('nt_th', [1, NT], ids=['static', 'timevarying'])
@pytest.mark.parametrize('resident', [True, False], ids=['hbm', 'host'])
@pytest.mark.parametrize('grid', GRIDS, ids=lambda g: f'{g[0]}x{g[1]}')
@pytest.mark.parametrize('real', ['float64', 'float32'])
def test_broadcast_thickness_is_the_per_level_path_bit_for_bit(real, grid, resident, nt_th, sverdrup, compact):
    a = _make(real, grid, resident, sverdrup=sverdrup, compact=compact)
    b = _make(real, grid, resident, sverdrup=sverdrup, compact=compact)
    assert numpy.array_equal(a.thickness, TH)
    e3 = _broadcast(real, grid, nt_th)
    assert numpy.array_equal(e3[0, :, 0, 0].astype(numpy.float64), TH)
    a.setCellThickness(_on(e3, resident), _on(e3.copy(), resident))
    tau = _tracer(real, grid)
    for f in (a, b):
        f.setTracer(_on(tau, resident), reference=4.25)
    for t in (1, 0, 2):
        assert a.computeFlux(t) == b.computeFlux(t)
        want = _row(b)
        assert numpy.abs(want).max() > 0
        assert numpy.array_equal(_row(a), want), t
        for x, y in zip(_resident(a), _resident(b)):      # six planes as (ncell, 4) + |eU|, |eV|, and the running max
            assert numpy.array_equal(x, y), t
        assert numpy.array_equal(_rows(a.computeFluxProfile(t)), _rows(b.computeFluxProfile(t))), t
        assert numpy.array_equal(_rows(a.computeTracerFlux(t)), _rows(b.computeTracerFlux(t))), t
    want_all = _rows(b.computeAll())
    got_all = _rows(a.computeAll())
    assert numpy.array_equal(got_all, want_all)
    for t in range(NT):                                    # computeAll rows are the per-step rows
        a.computeFlux(t)
        assert numpy.array_equal(_row(a), got_all[t]), t
    assert numpy.array_equal(_rows(a.computeAll()), want_all)       # a second pass (a replayed graph where there is one)
    for x, y in zip(_resident(a), _resident(b)):
        assert numpy.array_equal(x, y)
    assert numpy.array_equal(_rows(a.computeTracerAll()), _rows(b.computeTracerAll()))
    # another thickness gives other rows; clearing restores the original ones bit for bit
    a.setCellThickness(_on(2 * e3, resident), _on(e3, resident))
    assert not numpy.array_equal(_rows(a.computeAll()), want_all)
    a.setCellThickness(None, None)
    assert numpy.array_equal(_rows(a.computeAll()), want_all)
    a.computeFlux(1), b.computeFlux(1)
    assert numpy.array_equal(_row(a), _row(b))


@pytest.mark.parametrize('nt_th', [1, NT], ids=['static', 'timevarying'])
@pytest.mark.parametrize('real', ['float64', 'float32'])
def test_captured_pass_is_not_replayed_across_a_change_of_the_thickness(real, nt_th):
    """computeAll on a non-null stream captures the pass (pairs of steps included) and replays it: with a cell thickness the
    rows are those of direct launches; setting another thickness or clearing it re-captures; the library's per-launch
    timing counts one flux launch per step and sees the expansion behind the kernel"""
    import torch
    grid = GRIDS[0]
    e3u, e3v = _random_thickness(real, grid, nt_th, seed=19)
    direct = _make(real, grid, True)
    plain = _rows(direct.computeAll())
    direct.setCellThickness(_on(e3u, True), _on(e3v, True), fill_value=THFILL, missing_value=THMISSING)
    want = _rows(direct.computeAll())
    direct.setCellThickness(_on(e3v, True), _on(e3u, True), fill_value=THFILL, missing_value=THMISSING)
    swapped = _rows(direct.computeAll())
    assert not numpy.array_equal(want, plain) and not numpy.array_equal(want, swapped)
    st = torch.cuda.Stream()
    torch.cuda.synchronize()
    with torch.cuda.stream(st):
        g = _make(real, grid, True, stream=st.cuda_stream)
        out = torch.zeros((NT, g._rowlen), dtype=torch.float64, device='cuda')
        for rep in range(2):
            assert numpy.array_equal(_rows(g.computeAll(out=out)), plain), rep
        g.setCellThickness(_on(e3u, True), _on(e3v, True), fill_value=THFILL, missing_value=THMISSING)
        for rep in range(3):                    # capture, then two replays
            assert numpy.array_equal(_rows(g.computeAll(out=out)), want), rep
        planes = _resident(g)
        g.setCellThickness(_on(e3v, True), _on(e3u, True), fill_value=THFILL, missing_value=THMISSING)
        for rep in range(2):
            assert numpy.array_equal(_rows(g.computeAll(out=out)), swapped), rep
        g.setCellThickness(None, None)
        for rep in range(2):
            assert numpy.array_equal(_rows(g.computeAll(out=out)), plain), rep
        g.setCellThickness(_on(e3u, True), _on(e3v, True), fill_value=THFILL, missing_value=THMISSING)
        g.enableKernelTiming(True)
        assert numpy.array_equal(_rows(g.computeAll(out=out)), want)
        n, ms, flux, expand = g.readKernelTiming(split=True)
        k3 = g.readTransectTiming()
        g.enableKernelTiming(False)
        assert n == NT and flux > 0 and expand > 0 and k3 > 0 and abs(flux + expand - ms) <= 1e-9 * ms, (n, ms, flux, expand, k3)
        for x, y in zip(_resident(g)[:3], planes[:3]):      # (the running max has seen the other thicknesses since)
            assert numpy.array_equal(x, y)
    torch.cuda.synchronize()
    direct.setCellThickness(_on(e3u, True), _on(e3v, True), fill_value=THFILL, missing_value=THMISSING)
    direct.computeAll()
    for x, y in zip(_resident(direct)[:3], planes[:3]):
        assert numpy.array_equal(x, y)


# ---- 2. a staircase mask in the thickness is a mask on the velocities ------------------------------------------------------
@pytest.mark.parametrize('compact', [False, True], ids=['full', 'compact'])
@pytest.mark.parametrize('nt_th', [1, NT], ids=['static', 'timevarying'])
@pytest.mark.parametrize('resident', [True, False], ids=['hbm', 'host'])
@pytest.mark.parametrize('grid', GRIDS, ids=lambda g: f'{g[0]}x{g[1]}')
@pytest.mark.parametrize('real', ['float64', 'float32'])
def test_masked_thickness_is_masked_velocity(real, grid, resident, nt_th, compact):
    """e3 = th[z] * m, m in {0, 1}: the rows, planes and profile of the per-level path with uo / vo set to _FillValue where
    m = 0 (numpy.array_equal: +0 == -0)"""
    nx, ny = grid
    rng = numpy.random.default_rng(17)
    depth = rng.integers(0, NZ + 1, (nt_th, 1, ny, nx))               # wet levels of every column: a staircase
    m = numpy.arange(NZ)[None, :, None, None] < depth
    _, _, u, v = _case(real, grid)
    dt = u.dtype.type
    mm = numpy.broadcast_to(m, (NT, NZ, ny, nx)) if nt_th == 1 else m
    um, vm = numpy.where(mm, u, dt(FILL)), numpy.where(mm, v, dt(FILL))
    a = _make(real, grid, resident, compact=compact, sverdrup=True)
    b = _make(real, grid, resident, u=um, v=vm, compact=compact, sverdrup=True)
    e3 = (_broadcast(real, grid, nt_th) * m).astype(real)
    a.setCellThickness(_on(e3, resident), _on(e3.copy(), resident))
    for t in (2, 0, 1):
        a.computeFlux(t), b.computeFlux(t)
        assert numpy.abs(_row(b)).max() > 0
        assert numpy.array_equal(_row(a), _row(b)), t
        for x, y in zip(_resident(a), _resident(b)):
            assert numpy.array_equal(x, y), t
        assert numpy.array_equal(_rows(a.computeFluxProfile(t)), _rows(b.computeFluxProfile(t))), t
    assert numpy.array_equal(_rows(a.computeAll()), _rows(b.computeAll()))


# ---- 3. profile consistency ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('nt_th', [1, NT], ids=['static', 'timevarying'])
@pytest.mark.parametrize('grid', GRIDS, ids=lambda g: f'{g[0]}x{g[1]}')
@pytest.mark.parametrize('real', ['float64', 'float32'])
def test_profile_row_is_the_volume_row_of_that_level_alone(real, grid, nt_th):
    e3u, e3v = _random_thickness(real, grid, nt_th, seed=23)
    f = _make(real, grid, True, sverdrup=True)
    f.setCellThickness(_on(e3u, True), _on(e3v, True), fill_value=THFILL, missing_value=THMISSING)
    g = _make(real, grid, True, sverdrup=True)
    for t in (0, 2):
        prof = _rows(f.computeFluxProfile(t))
        assert (numpy.abs(prof).max(axis=1) > 0).all()
        for z in range(NZ):
            zu, zv = numpy.zeros_like(e3u), numpy.zeros_like(e3v)
            zu[:, z], zv[:, z] = e3u[:, z], e3v[:, z]
            g.setCellThickness(_on(zu, True), _on(zv, True), fill_value=THFILL, missing_value=THMISSING)
            g.computeFlux(t)
            assert numpy.array_equal(prof[z], _row(g)), (t, z)


@pytest.mark.parametrize('compact', [False, True], ids=['full', 'compact'])
@pytest.mark.parametrize('resident', [True, False], ids=['hbm', 'host'])
def test_profile_and_tracer_calls_leave_everything_else_alone(resident, compact):
    real, grid = 'float64', GRIDS[0]
    e3u, e3v = _random_thickness(real, grid, NT, seed=29)
    a = _make(real, grid, resident, compact=compact)
    b = _make(real, grid, resident, compact=compact)
    for f in (a, b):
        f.setCellThickness(_on(e3u, resident), _on(e3v, resident), fill_value=THFILL, missing_value=THMISSING)
    a.setTracer(_on(_tracer(real, grid), resident), reference=4.)
    p0, r0 = _rows(a.computeFluxProfile(1)), _rows(a.computeTracerFlux(1))
    for step in ('flux1', 'all', 'flux0', 'read', 'all', 'flux2', 'read'):
        a.computeFluxProfile(2), a.computeTracerFlux(0)
        if step == 'all':
            assert numpy.array_equal(_rows(a.computeAll()), _rows(b.computeAll()))
            a.computeTracerAll()
        elif step == 'read':
            for x, y in zip(_resident(a), _resident(b)):
                assert numpy.array_equal(x, y)
        else:
            t = int(step[-1])
            assert a.computeFlux(t) == b.computeFlux(t)
            a.computeFluxProfile(t), a.computeTracerFlux(t)
            assert numpy.array_equal(_row(a), _row(b))
    for x, y in zip(_resident(a), _resident(b)):
        assert numpy.array_equal(x, y)
    assert numpy.array_equal(_rows(a.computeFluxProfile(1)), p0) and numpy.array_equal(_rows(a.computeTracerFlux(1)), r0)


# ---- 4. against the definition ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize('wrap', [True, False], ids=['wrap', 'nowrap'])
@pytest.mark.parametrize('sverdrup', [False, True], ids=['m2', 'sv'])
@pytest.mark.parametrize('nt_th', [1, NT], ids=['static', 'timevarying'])
@pytest.mark.parametrize('resident', [True, False], ids=['hbm', 'host'])
@pytest.mark.parametrize('grid', GRIDS, ids=lambda g: f'{g[0]}x{g[1]}')
@pytest.mark.parametrize('real', ['float64', 'float32'])
def test_against_the_definition(real, grid, resident, nt_th, sverdrup, wrap):
    _, _, u, v = _case(real, grid)
    e3u, e3v = _random_thickness(real, grid, nt_th, seed=31 + nt_th)
    dt = u.dtype.type
    for x in (e3u, e3v):
        assert numpy.isnan(x).any() and ((x == dt(THFILL)) | (x == dt(THMISSING))).any()
    assert (e3u[:, 3:, 4:9, 10:20] != e3u[:, 3:, 4:9, 10:20]).any() and (u[:, 3:, 4:9, 10:20] == dt(FILL)).all()   # markers on land
    tau = _tracer(real, grid)
    tau[:, :, 10:14, 50:60] = dt(TFILL)
    ref = 3.25
    f = _make(real, grid, resident, sverdrup=sverdrup)
    f.setCellThickness(_on(e3u, resident), _on(e3v, resident), fill_value=THFILL, missing_value=THMISSING)
    f.setTracer(_on(tau, resident), fill_value=TFILL, missing_value=TMISSING, reference=ref, wrapX=wrap)
    r = _reference(f, wrap=wrap, ref=ref, sverdrup=sverdrup)
    arrays = {'uo': u, 'vo': v, 'e3u': e3u, 'e3v': e3v, 'tracer': tau}
    all_rows, all_tracer = _rows(f.computeAll()), _rows(f.computeTracerAll())
    for t in range(NT):
        want = r.step(array_values(arrays, t))
        assert want['volume'][1][-3:].min() > 0, 'every line must carry flux'
        f.computeFlux(t)
        _close(_row(f), want['volume'], f'volume t={t}')
        _close(_rows(f.computeFluxProfile(t)), want['volume_profile'], f'profile t={t}')
        _close(_rows(f.computeTracerFlux(t)), want['tracer'], f'tracer t={t}')
        assert numpy.array_equal(all_rows[t], _row(f)) and numpy.array_equal(all_tracer[t], _rows(f.computeTracerFlux(t)))


# ---- 5. closed form --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('nt_th', [1, NT], ids=['static', 'timevarying'])
@pytest.mark.parametrize('real', ['float64', 'float32'])
def test_closed_form_with_column_wise_splits_of_the_depth(real, nt_th):
    """psi = (t + 1) (cos(2 pi y / 360) + sin(2 pi x / 360)) has no z-dependence: u, v are the same on every level, and
    thicknesses that split one total depth D (D(t) when time-varying) differently in every column, at U points and at V
    points independently, give D (psi(end) - psi(start)) across a line between grid nodes.  float32 velocities carry their
    own rounding (6e-8), so the 1e-12 bar is asserted for float64; float32 is held to 1e-6."""
    from nemoflux_amd.fluxexact import exactFlux
    grid = GRIDS[0]
    nx, ny = grid
    blon, blat, u, v = _case(real, grid, psi=PSI_XY, fill=False)
    scale = (numpy.arange(NT) + 1.).astype(real)[:, None, None, None]
    u, v = u * scale, v * scale
    rng = numpy.random.default_rng(41)
    D = numpy.array([3.5, 2.25, 5.125])[:nt_th]

    def split():
        w = rng.uniform(0.1, 1., (nt_th, NZ, ny, nx))
        return (w / w.sum(axis=1, keepdims=True) * D[:, None, None, None]).astype(real)

    lines = ["(-100,-80),(100,-80),(0,80)", "(-150,-60),(-20,10),(120,55)"]
    f = _field(blon, blat, DB, _on(u, True), _on(v, True), [transect_xyz(s) for s in lines], readback=False)
    plain = _rows(f.computeAll())[:, -2:]
    f.setCellThickness(_on(split(), True), _on(split(), True))
    got = _rows(f.computeAll())[:, -2:]
    bar = 1e-12 if real == 'float64' else 1e-6
    for p, s in enumerate(lines):
        pts = [tuple(q[:2]) for q in transect_xyz(s)]
        dpsi = exactFlux(PSI_XY, pts, 1, 1)[0]
        assert abs(dpsi) > 0.5
        for t in range(NT):
            exact = D[t if nt_th > 1 else 0] * (t + 1) * dpsi
            print(f'{real} line {p} t={t}: rel err = {abs(got[t, p] - exact) / abs(exact):.3g}')
            assert abs(got[t, p] - exact) <= bar * abs(exact), (p, t, got[t, p], exact)
            assert f.computeFlux(t)[p] == got[t, p]
    if nt_th > 1:      # one deptht_bounds has one total depth: the per-level path cannot follow D(t)
        ratio = plain[:, 0] / (numpy.arange(NT) + 1.)
        assert numpy.allclose(ratio, ratio[0], rtol=1e-6) and not numpy.allclose(got[:, 0] / (numpy.arange(NT) + 1.), ratio[0] * numpy.ones(NT), rtol=1e-2)


# ---- 6. sharding -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('nt_th', [1, NT], ids=['static', 'timevarying'])
@pytest.mark.parametrize('resident', [True, False], ids=['hbm', 'host'])
@pytest.mark.parametrize('world', [2, 4, 5])
def test_sharded_ranks_add_up(world, resident, nt_th):
    """slab ranges that cut inside a time step: the ranks' volume rows, profiles and tracer rows add up to the full ones to
    1e-12 x sum |terms|; levels and steps a rank does not own give exact zeros"""
    import torch
    from nemoflux_amd.dist import slab_range
    real, grid = 'float64', GRIDS[0]
    _, _, u, v = _case(real, grid)
    e3u, e3v = _random_thickness(real, grid, nt_th, seed=43)
    tau = _tracer(real, grid)

    def make(**kw):
        f = _make(real, grid, resident, **kw)
        f.setCellThickness(_on(e3u, resident), _on(e3v, resident), fill_value=THFILL, missing_value=THMISSING)
        f.setTracer(_on(tau, resident), reference=4.)
        return f

    full = make()
    want = {'volume': _rows(full.computeAll()), 'tracer': _rows(full.computeTracerAll()),
            'profile': numpy.array([_rows(full.computeFluxProfile(t)) for t in range(NT)])}
    r = _reference(full, ref=4.)
    arrays = {'uo': u, 'vo': v, 'e3u': e3u, 'e3v': e3v, 'tracer': tau}
    refs = [r.step(array_values(arrays, t)) for t in range(NT)]
    mag = {'volume': numpy.array([x['volume'][1] for x in refs]), 'tracer': numpy.array([x['tracer'][1] for x in refs]),
           'profile': numpy.array([x['volume_profile'][1] for x in refs])}
    acc = {k: numpy.zeros_like(x) for k, x in want.items()}
    cut_inside = False
    for rank in range(world):
        sr = slab_range(NT, NZ, rank, world)
        cut_inside = cut_inside or sr[0] % NZ != 0
        part = make(slab_range=sr)
        out = torch.full((NT, part._rowlen), numpy.nan, dtype=torch.float64, device='cuda')
        got = {'volume': _rows(part.computeAll(out=out)), 'tracer': _rows(part.computeTracerAll()),
               'profile': numpy.array([_rows(part.computeFluxProfile(t)) for t in range(NT)])}
        assert numpy.array_equal(got['volume'], out.cpu().numpy())
        for t in range(NT):
            lo, hi = max(sr[0], t * NZ), min(sr[1], (t + 1) * NZ)
            if hi <= lo:
                assert numpy.all(got['volume'][t] == 0) and numpy.all(got['tracer'][t] == 0) and numpy.all(got['profile'][t] == 0)
            else:
                own = numpy.zeros(NZ, bool)
                own[lo - t * NZ:hi - t * NZ] = True
                assert numpy.all(got['profile'][t][~own] == 0), (rank, t)
                assert numpy.array_equal(got['profile'][t][own], want['profile'][t][own]), (rank, t)
                if own.all():
                    assert numpy.array_equal(got['volume'][t], want['volume'][t])
                    assert numpy.array_equal(got['tracer'][t], want['tracer'][t])
            part.computeFlux(t)
            assert numpy.array_equal(_row(part), got['volume'][t]), (rank, t)
        for k in acc:
            acc[k] += got[k]
    assert cut_inside
    for k in acc:
        assert numpy.abs(want[k]).max() > 0
        err = numpy.abs(acc[k] - want[k])
        print(f'world {world} {k}: max |err| / mag = {float((err / numpy.maximum(mag[k], 1e-300)).max()):.3g}')
        assert numpy.all(err <= BAR * mag[k]), k


# ---- 7. refusals -----------------------------------------------------------------------------------------------------------
def test_refusals():
    from nemoflux_amd import _lib
    from nemoflux_amd._lib import lib, NemofluxError, NF_F64, NF_F32
    real, grid = 'float64', GRIDS[0]
    nx, ny = grid
    f = _make(real, grid, True)
    e3 = _broadcast(real, grid, 1)
    dev = _on(e3, True)
    tau = _on(_tracer(real, grid), True)
    f.setTracer(tau)
    f.setClassEdges([4.2, 4.5, 4.8])
    before = {'tp': _rows(f.computeTracerProfile(1)), 'ct': _rows(f.computeClassTransport(1)),
              'ctt': _rows(f.computeClassTracerTransport(1))}
    f.setCellThickness(dev, dev)
    import torch
    out = torch.zeros((8, f._rowlen), dtype=torch.float64, device='cuda')
    for call, kw in ((f.computeTracerProfile, {}), (f.computeClassTransport, {}), (f.computeClassTracerTransport, {}),
                     (f.computeTracerProfile, dict(out=out[:NZ])), (f.computeClassTransport, dict(out=out[:5])),
                     (f.computeClassTracerTransport, dict(out=out[:5]))):
        with pytest.raises(NemofluxError) as e:
            call(1, **kw)
        msg = str(e.value)
        assert 'error 2' in msg and 'cell thickness' in msg and 'nf_field_set_cell_thickness(NULL)' in msg, msg
        assert 'per-cell thicknesses yet' in msg
    assert float(out.abs().max()) == 0
    # the forms that take it still run, and clearing brings the refused ones back with their rows
    f.computeFlux(1), f.computeFluxProfile(1), f.computeTracerFlux(1)
    f.setCellThickness(None, None)
    assert numpy.array_equal(_rows(f.computeTracerProfile(1)), before['tp'])
    assert numpy.array_equal(_rows(f.computeClassTransport(1)), before['ct'])
    assert numpy.array_equal(_rows(f.computeClassTracerTransport(1)), before['ctt'])
    # the C ABI: dtype mismatch names both dtypes, nt_th must be 1 or nt, call order
    h = ctypes.byref(f._h)
    p = dev.data_ptr()
    assert lib.nf_field_set_cell_thickness(h, p, p, 1, NF_F32, 1, numpy.nan) == 1
    msg = lib.nf_last_error()
    assert b'float32' in msg and b'float64' in msg
    for nt_th in (0, 2, NT + 1):
        assert lib.nf_field_set_cell_thickness(h, p, p, nt_th, NF_F64, 1, numpy.nan) == 1
        assert f'nt = {nt_th}'.encode() in lib.nf_last_error()
    assert lib.nf_field_set_cell_thickness(h, p, p, 1, NF_F64, 1, numpy.nan) == 0
    assert lib.nf_field_set_cell_thickness(h, None, None, 0, NF_F64, 0, numpy.nan) == 0
    g = ctypes.c_void_p()
    assert lib.nf_field_new(ctypes.byref(g)) == 0
    try:
        assert lib.nf_field_set_cell_thickness(ctypes.byref(g), p, p, 1, NF_F64, 1, numpy.nan) == 2      # before set_uv
        assert b'set_uv' in lib.nf_last_error()
        assert lib.nf_field_set_uv(ctypes.byref(g), p, p, 1, NF_F64, 1, numpy.nan) == 0
        assert lib.nf_field_set_cell_thickness(ctypes.byref(g), p, p, 1, NF_F64, 1, numpy.nan) == 2      # before set_thickness
        assert b'set_thickness first' in lib.nf_last_error()
        assert lib.nf_field_set_thickness(ctypes.byref(g), _lib.dptr(TH), NZ) == 0
        assert lib.nf_field_set_cell_thickness(ctypes.byref(g), p, p, 1, NF_F64, 1, numpy.nan) == 0
        assert lib.nf_field_set_cell_thickness(ctypes.byref(g), e3.ctypes.data, e3.ctypes.data, 1, NF_F64, 0, numpy.nan) == 2
        assert b'set_bounds first' in lib.nf_last_error()        # a static host array is uploaded at the call
    finally:
        assert lib.nf_field_del(ctypes.byref(g)) == 0
    # Python: shapes, and what is not cast
    with pytest.raises(RuntimeError, match=r'\(7, 36, 71\)'):
        f.setCellThickness(numpy.ones((NZ, ny, nx - 1)), e3)
    with pytest.raises(RuntimeError, match='float32'):
        f.setCellThickness(_on(e3.astype(numpy.float32), True), _on(e3.astype(numpy.float32), True))
    with pytest.raises(RuntimeError, match='both be host arrays or both be device arrays'):
        f.setCellThickness(dev, e3)
    f.computeFlux(1)      # none of the refused calls left a cell thickness behind


def test_static_host_thickness_of_another_float_dtype_is_cast():
    """a float64 thickness beside float32 velocities is rounded to float32: the rows of passing the rounded array"""
    real, grid = 'float32', GRIDS[0]
    e3u, e3v = _random_thickness('float64', grid, 1, seed=47, markers=False)
    a, b = _make(real, grid, True), _make(real, grid, True)
    a.setCellThickness(e3u[0], e3v[0])
    b.setCellThickness(_on(e3u.astype(numpy.float32), True), _on(e3v.astype(numpy.float32), True))
    assert numpy.array_equal(_rows(a.computeAll()), _rows(b.computeAll()))
    assert not numpy.array_equal(e3u.astype(numpy.float32).astype(numpy.float64), e3u)


# ---- 8. files and the command line -----------------------------------------------------------------------------------------
def _write_npz(tmp_path, real, nt_th, squeeze=False):
    blon, blat, u, v = _case(real, GRIDS[0])
    e3u, e3v = _random_thickness(real, GRIDS[0], nt_th, seed=53)
    paths = {k: str(tmp_path / f'{k}.npz') for k in 'TUV'}
    numpy.savez(paths['T'], bounds_lon=blon, bounds_lat=blat, deptht_bounds=DB)
    sq = (lambda x: x[0]) if squeeze else (lambda x: x)
    numpy.savez(paths['U'], uo=u, _FillValue_uo=numpy.array(FILL), _missing_value_uo=numpy.array(MISSING), e3u=sq(e3u),
                _FillValue_e3u=numpy.array(THFILL), _missing_value_e3u=numpy.array(THMISSING))
    numpy.savez(paths['V'], vo=v, _FillValue_vo=numpy.array(FILL), _missing_value_vo=numpy.array(MISSING), thk=sq(e3v),
                _FillValue_thk=numpy.array(THFILL), _missing_value_thk=numpy.array(THMISSING))
    return paths, u, v, e3u, e3v


def _write_classic(path, name, a, fill):
    """a (nt, nz, ny, nx) float32 record variable over an unlimited time axis, big-endian, the way IOIPSL-era NEMO wrote it"""
    from scipy.io import netcdf_file
    nt, nz, ny, nx = a.shape
    f = netcdf_file(path, 'w', version=2)
    for n, s in (('time_counter', None), ('depth', nz), ('y', ny), ('x', nx)):
        f.createDimension(n, s)
    var = f.createVariable(name, 'f4', ('time_counter', 'depth', 'y', 'x'))
    var._FillValue = numpy.float32(fill)
    var[:] = a
    f.close()


@pytest.mark.parametrize('form', ['static3d', 'static4d', 'timevarying'])
def test_file_backed_thickness_and_fluxplot(tmp_path, form):
    """(path, name) thicknesses from .npz bundles give the rows of the in-memory arrays bit for bit, and fluxplot
    --cell-thickness prints those totals (plain series, --zrange, --levels, --tracer)"""
    from nemoflux_amd import fluxplot
    from nemoflux_amd.field import Field
    real = 'float32'
    nt_th = NT if form == 'timevarying' else 1
    paths, u, v, e3u, e3v = _write_npz(tmp_path, real, nt_th, squeeze=form == 'static3d')
    lines = "[" + "],[".join(LINES) + "]"
    tr = fluxplot.readTargets(lines)[0]
    mem = _field(*_case(real, GRIDS[0])[:2], DB, u, v, tr, readback=False, fill_value=FILL, missing_value=MISSING)
    mem.setCellThickness(e3u, e3v, fill_value=THFILL, missing_value=THMISSING)
    want = _rows(mem.computeAll())
    ff = _quiet(Field, paths['T'], paths['U'], paths['V'], tr, readback=False)
    ff.setCellThickness((paths['U'], 'e3u'), (paths['V'], 'thk'))
    assert numpy.array_equal(_rows(ff.computeAll()), want)
    for t in (2, 0):
        ff.computeFlux(t)
        assert numpy.array_equal(_row(ff), want[t])
        assert numpy.array_equal(_rows(ff.computeFluxProfile(t)), _rows(mem.computeFluxProfile(t)))
    kw = dict(tFile=paths['T'], uFile=paths['U'], vFile=paths['V'], lonLatPoints=lines, cellThickness=True, e3v='thk')
    with pytest.raises(RuntimeError, match='could not read e3v'):       # the default name is e3v, of the V file
        _quiet(fluxplot.main, **dict(kw, e3v=''))
    totals = _quiet(fluxplot.main, output=str(tmp_path / 'a.csv'), **kw)
    assert numpy.array_equal(totals, want[:, -3:]) and numpy.abs(totals).max() > 0
    with open(tmp_path / 'a.csv') as fh:
        table = numpy.array([[float(x) for x in ln.split(',')[1:]] for ln in fh.read().splitlines()[2:]])
    assert numpy.allclose(table, want[:, -3:], rtol=1e-14, atol=0)
    plain = _quiet(fluxplot.main, output=str(tmp_path / 'b.csv'), **dict(kw, cellThickness=False, e3v=''))
    assert not numpy.array_equal(plain, totals)
    # e3 from files of their own
    other = _quiet(fluxplot.main, output=str(tmp_path / 'c.csv'),
                   **dict(kw, e3u='thk', e3FileU=paths['V'], e3v='e3u', e3FileV=paths['U']))
    mem.setCellThickness(e3v, e3u, fill_value=THFILL, missing_value=THMISSING)
    assert numpy.array_equal(other, _rows(mem.computeAll())[:, -3:])
    mem.setCellThickness(e3u, e3v, fill_value=THFILL, missing_value=THMISSING)
    levels = _quiet(fluxplot.main, output=str(tmp_path / 'd.csv'), levels=True, **kw)
    assert numpy.array_equal(levels, numpy.array([mem.computeFluxProfile(t)[0] for t in range(NT)]))
    band = _quiet(fluxplot.main, output=str(tmp_path / 'e.csv'), zrange='0.2,2.0', **kw)
    assert numpy.array_equal(band, numpy.array([mem.depthBandFlux(mem.computeFluxProfile(t)[0], 0.2, 2.0) for t in range(NT)]))
    tracer = _quiet(fluxplot.main, output=str(tmp_path / 'f.csv'), tracer='uo', tracerFile=paths['U'], tracerRef=0.5, **kw)
    mem.setTracer(u, fill_value=FILL, missing_value=MISSING, reference=0.5)
    assert numpy.array_equal(tracer, mem.computeTracerAll()[0]) and numpy.abs(tracer).max() > 0


def test_time_varying_thickness_read_step_by_step_from_classic_netcdf(tmp_path):
    """float32 record variables of a NetCDF-3 file (big-endian, one time step at a time through pinned buffers) give the rows
    of the in-memory arrays bit for bit, in any step order"""
    real, grid = 'float32', GRIDS[0]
    e3u, e3v = _random_thickness(real, grid, NT, seed=59)
    e3u[e3u == numpy.float32(THMISSING)] = numpy.float32(THFILL)       # one marker per file variable
    e3v[e3v == numpy.float32(THMISSING)] = numpy.float32(THFILL)
    pu, pv = str(tmp_path / 'e3u.nc'), str(tmp_path / 'e3v.nc')
    _write_classic(pu, 'e3u', e3u, THFILL)
    _write_classic(pv, 'e3v', e3v, THFILL)
    mem, ff = _make(real, grid, True), _make(real, grid, True)
    mem.setCellThickness(e3u, e3v, fill_value=THFILL)
    ff.setCellThickness((pu, 'e3u'), (pv, 'e3v'))
    assert ff._cell_thickness_lazy()
    mem.setTracer(_tracer(real, grid)), ff.setTracer(_tracer(real, grid))
    want = _rows(mem.computeAll())
    for t in (2, 0, 1, 1):
        ff.computeFlux(t)
        assert numpy.array_equal(_row(ff), want[t]) and numpy.abs(want[t]).max() > 0
        assert numpy.array_equal(_rows(ff.computeFluxProfile(t)), _rows(mem.computeFluxProfile(t)))
        assert numpy.array_equal(_rows(ff.computeTracerFlux((t + 1) % NT)), _rows(mem.computeTracerFlux((t + 1) % NT)))
    assert numpy.array_equal(_rows(ff.computeAll()), want)
    assert numpy.array_equal(_rows(ff.computeTracerAll()), _rows(mem.computeTracerAll()))
