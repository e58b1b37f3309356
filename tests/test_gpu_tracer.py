"""Tracer transports across transects (Field.setTracer / computeTracerFlux / computeTracerAll, nf_field_compute_tracer_*):
the integral of u * tau_face, tau at T-points interpolated to the U / V faces.  Anchored bit for bit to the volume rows
(tau == ref + 1, tau == 2**k), checked against a float64 numpy restatement of the definition (face rule, markers, wrap, last
row) on odd grids, against the depth profiles for a tracer that depends on z only; computing tracer rows changes nothing
else; sharded ranks add up; file-backed tracers; fluxplot --tracer."""
import os

import numpy
import pytest

from conftest import GOLDEN, transect_xyz
from gpu_helpers import _field, _on, _quiet, _resident

pytestmark = pytest.mark.gpu

PSI_ZT = "(1+10*z)*(t+1)*(cos(2*pi*y/360) + sin(2*pi*x/360))"
T_TRI = "(-100,-80),(100,-80),(0,80),(-100,-80)"
T_OPEN = "(-100,-80),(100,-80),(0,80)"
# crosses the periodic seam at lon = +-180: the east faces of the last column
T_SEAM = "(150,-30),(179.5,-20),(179.9,10),(175,40)"
NX, NY, NZ, NT = 72, 36, 7, 3
FILL, MISSING = 1.e20, -999.
TFILL, TMISSING = -32768., 12345.        # the tracer's own markers (not those of uo / vo)
R_SV = 6371000.0 / 1.e6


_CASES = {}


def _case(real, fill=True):
    """host u, v (nt, nz, ny, nx) of the PSI_ZT case; with `fill`, land blocks marked by _FillValue, NaN and a second
    missing value"""
    key = (real, fill)
    if key not in _CASES:
        from nemoflux_amd.datagen import DataGen
        dg = DataGen(real=real)
        dg.setSizes(NX, NY, NZ, NT)
        dg.setBoundingBox(-180., 180., -90., 90., 0., 1.)
        dg.build()
        dg.applyStreamFunction(PSI_ZT)
        dg.computeUVFromPotential()
        u, v = dg.u.cpu().numpy().copy(), dg.v.cpu().numpy().copy()
        v[:, :, -1, :] = 0                     # datagen's pole row is 1e13-sized garbage
        if fill:
            dt = u.dtype.type
            u[:, 3:, 4:9, 10:20] = dt(FILL)
            v[:, 3:, 4:9, 10:20] = numpy.nan
            u[:, :2, 20:24, 30:40] = dt(MISSING)
            v[:, 5:, 20:24, 30:40] = dt(MISSING)
        _CASES[key] = (dg.bounds_lon.cpu().numpy(), dg.bounds_lat.cpu().numpy(), dg.deptht_bounds, u, v)
    return _CASES[key]


def _args(real, resident, fill=True):
    blon, blat, db, u, v = _case(real, fill)
    return (blon, blat, db, _on(u, resident), _on(v, resident),
            [transect_xyz(T_OPEN), transect_xyz(T_TRI), transect_xyz(T_SEAM)])


def _kw(sverdrup, fill=True, **kw):
    kw.update(sverdrup=sverdrup, readback=False)
    if fill:
        kw.update(fill_value=FILL, missing_value=MISSING)
    return kw


def _row(f):
    """the [segments | transects] row of the last computeFlux"""
    return numpy.array(f._row[:f._rowlen])


def _tracer_row(f, t):
    tot, seg = f.computeTracerFlux(t)
    return numpy.concatenate([seg, tot])


def _all_rows(pair):
    tot, seg = pair
    return numpy.concatenate([seg, tot], axis=1)


def _isolated_markers(tau):
    """tracer markers (_FillValue, missing_value, NaN) on interior cells no two of which share a face"""
    dt = tau.dtype.type
    for k, m in enumerate((TFILL, TMISSING, numpy.nan)):
        tau[:, k::3, 2 + k:-2:3, 2:-2:4] = dt(m)    # one marker kind per level: rows 3 apart, columns 4 apart
    return tau


@pytest.mark.parametrize('ref', [0.0, 20.0])
@pytest.mark.parametrize('wrap', [True, False], ids=['wrap', 'nowrap'])
@pytest.mark.parametrize('compact', [False, True], ids=['full', 'compact'])
@pytest.mark.parametrize('resident', [True, False], ids=['hbm', 'host'])
@pytest.mark.parametrize('sverdrup', [False, True], ids=['m2', 'sv'])
@pytest.mark.parametrize('real', ['float64', 'float32'])
def test_unit_tracer_gives_the_volume_rows_bit_for_bit(real, sverdrup, resident, compact, wrap, ref):
    """tau == ref + 1 (with tracer markers on isolated cells, whose faces then take the other side's value) makes every face
    value exactly 1: the tracer rows are the volume rows, bit for bit, per step and for all steps."""
    f = _field(*_args(real, resident), **_kw(sverdrup, compact=compact))
    u = _case(real)[3]
    tau = _isolated_markers(numpy.full(u.shape, ref + 1.0, dtype=u.dtype))
    assert numpy.isnan(tau).any() and (tau == tau.dtype.type(TFILL)).any()
    f.setTracer(_on(tau, resident), fill_value=TFILL, missing_value=TMISSING, reference=ref, wrapX=wrap)
    for t in (1, 0, 2):
        got = _tracer_row(f, t)
        f.computeFlux(t)
        want = _row(f)
        assert numpy.abs(want).max() > 0
        assert numpy.array_equal(got, want), t
    assert numpy.array_equal(_all_rows(f.computeTracerAll()), _all_rows(f.computeAll()))


@pytest.mark.parametrize('k', [-3, 5])
@pytest.mark.parametrize('real', ['float64', 'float32'])
def test_power_of_two_tracer_scales_the_volume_rows_exactly(real, k):
    f = _field(*_args(real, True), **_kw(False))
    u = _case(real)[3]
    f.setTracer(_on(numpy.full(u.shape, 2.0 ** k, dtype=u.dtype), True))
    want = _all_rows(f.computeAll())
    assert numpy.array_equal(_all_rows(f.computeTracerAll()), want * 2.0 ** k)
    for t in range(NT):
        f.computeFlux(t)
        assert numpy.array_equal(_tracer_row(f, t), _row(f) * 2.0 ** k), t


# ---- the definition, restated in float64 numpy -----------------------------------------------------------------------------
def _restated_planes(u, v, tau, th, arc, umark, tmark, ref, wrap, sverdrup):
    """eU_tau, eV_tau (ncell,) of one step: u, v, tau (nz, ny, nx) in their own dtype; markers compared in that dtype"""
    dt = tau.dtype.type
    um = [dt(m) for m in umark if m == m]
    tm = [dt(m) for m in tmark if m == m]

    def present(x):
        ok = ~numpy.isnan(x)
        for m in tm:
            ok &= x != m
        return ok

    def fixed(x):
        bad = numpy.isnan(x)
        for m in um:
            bad |= x == m
        return numpy.where(bad, 0.0, x.astype(numpy.float64))

    def face(a, b, has_b):
        pa, pb = present(a), has_b & present(b)
        a64, b64 = a.astype(numpy.float64), b.astype(numpy.float64)
        with numpy.errstate(invalid='ignore', over='ignore'):
            s = numpy.where(pa & pb, 0.5 * (a64 + b64), numpy.where(pa, a64, b64))
            return numpy.where(pa | pb, s - ref, 0.0)

    nz, ny, nx = tau.shape
    has_e = numpy.ones((nz, ny, nx), bool)
    if not wrap:
        has_e[:, :, -1] = False
    has_n = numpy.ones((nz, ny, nx), bool)
    has_n[:, -1, :] = False
    tfE = face(tau, numpy.roll(tau, -1, axis=2), has_e)
    tfN = face(tau, numpy.roll(tau, -1, axis=1), has_n)
    accU = numpy.zeros((ny, nx))
    accV = numpy.zeros((ny, nx))
    for z in range(nz):
        accU = accU + th[z] * (fixed(u[z]) * tfE[z])
        accV = accV + th[z] * (fixed(v[z]) * tfN[z])
    eU = accU.reshape(-1) * arc[:, 1]
    eV = -accV.reshape(-1) * arc[:, 2]
    if sverdrup:
        eU, eV = eU * R_SV, eV * R_SV
    return eU, eV


def _restated_rows(f, eU, eV):
    """[segments | transects] of planes eU, eV through the field's own (cell, edge) weights, with the bound
    1e-12 * sum|terms| per value"""
    ny, nx = f.ny, f.nx
    iv = numpy.zeros((ny * nx, 4))
    iv[:, 1], iv[:, 2] = eU, eV
    iv[nx:, 0] = eV[:-nx]                                            # south slot = north value of the row below
    iv[:, 3] = eU.reshape(ny, nx)[:, numpy.r_[nx - 1, 0:nx - 1]].reshape(-1)   # west slot, periodic
    ce, w, sg = f.getWeights()
    terms = w * iv.reshape(-1)[ce]
    nseg = f._nseg
    seg = numpy.zeros(nseg)
    mag = numpy.zeros(nseg)
    numpy.add.at(seg, sg, terms)
    numpy.add.at(mag, sg, numpy.abs(terms))
    o = f._tr_off
    tot = numpy.array([seg[o[i]:o[i + 1]].sum() for i in range(len(o) - 1)])
    tmag = numpy.array([mag[o[i]:o[i + 1]].sum() for i in range(len(o) - 1)])
    return numpy.concatenate([seg, tot]), numpy.concatenate([mag, tmag])


def _small_grid(real, nx, ny, nz, nt, seed):
    """bounds of a regular 1-degree grid on [0, nx] x [0, ny], random u, v with markers, random tau with markers on
    isolated cells and on pairs of neighbours (faces with one and with both sides missing)"""
    from nemoflux_amd.datagen import DataGen
    dg = DataGen(real=real)
    dg.setSizes(nx, ny, nz, nt)
    dg.setBoundingBox(0., float(nx), 0., float(ny), 0., 1.)
    dg.build()
    rng = numpy.random.default_rng(seed)
    dt = numpy.dtype(real).type
    shape = (nt, nz, ny, nx)
    u = rng.standard_normal(shape).astype(dt)
    v = rng.standard_normal(shape).astype(dt)
    u.reshape(-1)[rng.choice(u.size, u.size // 9, replace=False)] = dt(FILL)
    v.reshape(-1)[rng.choice(v.size, v.size // 9, replace=False)] = numpy.nan
    u.reshape(-1)[rng.choice(u.size, u.size // 11, replace=False)] = dt(MISSING)
    tau = (10. + 5. * rng.standard_normal(shape)).astype(dt)
    for m in (TFILL, TMISSING, numpy.nan):
        tau.reshape(-1)[rng.choice(tau.size, tau.size // 7, replace=False)] = dt(m)
    return dg.bounds_lon.cpu().numpy(), dg.bounds_lat.cpu().numpy(), dg.deptht_bounds, u, v, tau


# transects inside [0, nx] x [0, ny] that cross the last column (its east faces) and the last row (its north faces)
def _small_lines(nx, ny):
    x1, y1 = nx - 0.37, ny - 0.41
    return [transect_xyz(f"(0.3,0.2),({x1},{0.6 * ny}),({0.5 * nx},{y1})"),
            transect_xyz(f"({x1},0.45),({x1 - 0.02},{y1})"),
            transect_xyz(f"(0.61,{y1}),({x1},{y1 - 0.03})")]


@pytest.mark.parametrize('wrap', [True, False], ids=['wrap', 'nowrap'])
@pytest.mark.parametrize('sverdrup', [False, True], ids=['m2', 'sv'])
@pytest.mark.parametrize('grid', [(37, 11), (38, 12), (72, 36), (1, 11), (37, 1), (5, 3)], ids=lambda g: f'{g[0]}x{g[1]}')
@pytest.mark.parametrize('real', ['float64', 'float32'])
def test_against_the_numpy_restatement(real, grid, sverdrup, wrap):
    nx, ny = grid
    nz, nt = 5, 2
    blon, blat, db, u, v, tau = _small_grid(real, nx, ny, nz, nt, seed=nx * 100 + ny)
    f = _field(blon, blat, db, u, v, _small_lines(nx, ny), sverdrup=sverdrup, readback=False, fill_value=FILL,
               missing_value=MISSING, periodX=0.)
    ref = 3.25
    f.setTracer(tau, fill_value=TFILL, missing_value=TMISSING, reference=ref, wrapX=wrap)
    th = f.thickness
    arc = f.arcLengths
    allrows = _all_rows(f.computeTracerAll())
    for t in range(nt):
        eU, eV = _restated_planes(u[t], v[t], tau[t], th, arc, (FILL, MISSING), (TFILL, TMISSING), ref, wrap, sverdrup)
        want, mag = _restated_rows(f, eU, eV)
        assert mag[-3:].min() > 0, 'every line must carry flux'
        got = _tracer_row(f, t)
        assert numpy.all(numpy.abs(got - want) <= 1e-12 * mag), (t, numpy.abs(got - want).max())
        assert numpy.array_equal(allrows[t], got)


@pytest.mark.parametrize('resident', [True, False], ids=['hbm', 'host'])
@pytest.mark.parametrize('real', ['float64', 'float32'])
def test_level_tracer_is_the_weighted_profile(real, resident):
    """tau[t, z, j, i] = c_z: the rows are sum_z (c_z - ref) * computeFluxProfile(t)[z] (fp64 rounding apart)."""
    f = _field(*_args(real, resident), **_kw(False))
    u = _case(real)[3]
    c = numpy.array([14., 11.5, 9., 6.25, 4., 3., 2.5])
    ref = 1.5
    tau = numpy.broadcast_to(c.astype(u.dtype)[None, :, None, None], u.shape).copy()
    f.setTracer(_on(tau, resident), reference=ref)
    for t in range(NT):
        tot, seg = f.computeFluxProfile(t)
        prof = numpy.concatenate([seg, tot], axis=1)
        want = ((c - ref)[:, None] * prof).sum(axis=0)
        bound = 1e-13 * (numpy.abs((c - ref)[:, None] * prof).sum(axis=0) + numpy.abs(want).max())
        got = _tracer_row(f, t)
        assert numpy.all(numpy.abs(got - want) <= bound), t


@pytest.mark.parametrize('compact', [False, True])
@pytest.mark.parametrize('resident', [True, False], ids=['hbm', 'host'])
def test_tracer_calls_leave_everything_else_alone(compact, resident):
    """tracer calls between computeFlux, computeAll and read-backs: rows, planes, |.| arrays and the running max equal those
    of a field that never saw a tracer, bit for bit; the tracer rows are reproducible"""
    args = _args('float64', resident)
    a = _field(*args, compact=compact, **_kw(False))
    b = _field(*args, compact=compact, **_kw(False))
    rng = numpy.random.default_rng(7)
    tau = (4. + rng.random(_case('float64')[3].shape)).astype(numpy.float64)
    a.setTracer(_on(tau, resident), reference=4.)
    p0 = _tracer_row(a, 1)
    for step in ('flux1', 'all', 'flux0', 'read', 'tall', 'all', 'flux2', 'read'):
        _tracer_row(a, 2)
        if step == 'all':
            assert all(numpy.array_equal(x, y) for x, y in zip(a.computeAll(), b.computeAll()))
            _tracer_row(a, 0)
        elif step == 'tall':
            a.computeTracerAll()
        elif step == 'read':
            for x, y in zip(_resident(a), _resident(b)):
                assert numpy.array_equal(x, y)
        else:
            t = int(step[-1])
            assert a.computeFlux(t) == b.computeFlux(t)
            assert numpy.array_equal(_row(a), _row(b))
            assert a.getSegmentFluxes()[0].tolist() == b.getSegmentFluxes()[0].tolist()
    for x, y in zip(_resident(a), _resident(b)):
        assert numpy.array_equal(x, y)
    assert numpy.array_equal(_tracer_row(a, 1), p0)


@pytest.mark.parametrize('world', [2, 3, 5])
def test_sharded_tracer_rows_add_up(world):
    """slab ranges that cut inside steps: steps a rank does not touch are exact zeros, a step one rank owns whole is the
    single-rank row bit for bit, and the ranks' rows sum to the single-rank rows (1e-13 relative)"""
    import torch
    from nemoflux_amd.dist import slab_range
    args = _args('float64', True)
    rng = numpy.random.default_rng(11)
    tau = _on((2. + rng.random(_case('float64')[3].shape)), True)
    full = _field(*args, **_kw(False))
    full.setTracer(tau)
    want = _all_rows(full.computeTracerAll())
    assert numpy.abs(want).max() > 0
    acc = numpy.zeros_like(want)
    for r in range(world):
        sr = slab_range(NT, NZ, r, world)
        part = _field(*args, slab_range=sr, **_kw(False))
        part.setTracer(tau)
        out = torch.full((NT, part._rowlen), numpy.nan, dtype=torch.float64, device='cuda')
        rows = _all_rows(part.computeTracerAll(out=out))
        assert numpy.array_equal(rows, out.cpu().numpy())
        for t in range(NT):
            lo, hi = max(sr[0], t * NZ), min(sr[1], (t + 1) * NZ)
            if hi <= lo:
                assert numpy.all(rows[t] == 0), (r, t)
            elif lo == t * NZ and hi == (t + 1) * NZ:
                assert numpy.array_equal(rows[t], want[t]), (r, t)
            assert numpy.array_equal(_tracer_row(part, t), rows[t]), (r, t)
        acc += rows
    assert numpy.allclose(acc, want, rtol=1e-13, atol=1e-13 * numpy.abs(want).max())


def _h5_files():
    h5 = os.path.join(GOLDEN, 'h5')
    return dict(tFile=os.path.join(h5, 'nemo_T.h5'), uFile=os.path.join(h5, 'nemo_U.h5'), vFile=os.path.join(h5, 'nemo_V.h5'))


def test_file_backed_tracer_equals_from_arrays():
    """setTracer((nemo_U.h5, 'uo')): a chunked, deflated float32 variable with a _FillValue, read one step at a time, gives
    the rows of fromArrays with the decoded array, bit for bit, in any step order"""
    from nemoflux_amd import hdf5min
    from nemoflux_amd.field import Field
    files = _h5_files()
    tr = [transect_xyz(T_OPEN), transect_xyz("(-180,-70),(-160,-10),(-35,40),(20,-50),(60,50),(180,40)")]
    ff = _quiet(Field, files['tFile'], files['uFile'], files['vFile'], tr)
    ff.setTracer((files['uFile'], 'uo'), reference=0.125)
    with hdf5min.File(files['tFile']) as f:
        blon, blat = f.datasets['bounds_lon'].read(), f.datasets['bounds_lat'].read()
        db = f.datasets['deptht_bounds'].read()
    with hdf5min.File(files['uFile']) as f:
        u = numpy.array(f.datasets['uo'].read())
        fill = float(f.datasets['uo'].fill_value)
    with hdf5min.File(files['vFile']) as f:
        v = numpy.array(f.datasets['vo'].read())
    fa = _field(blon, blat, db, u, v, tr, fill_value=fill)
    fa.setTracer(u.copy(), fill_value=fill, reference=0.125)
    assert u.dtype == numpy.float32 and (u == numpy.float32(1.e20)).any()
    for t in (2, 0, 1, 1):
        assert numpy.array_equal(_tracer_row(ff, t), _tracer_row(fa, t)), t
        assert numpy.abs(_tracer_row(ff, t)).max() > 0
    assert numpy.array_equal(_all_rows(ff.computeTracerAll()), _all_rows(fa.computeTracerAll()))
    assert ff.computeFlux(1) == fa.computeFlux(1)


def _read_table(path):
    with open(path) as fh:
        lines = [ln for ln in fh.read().splitlines() if not ln.startswith('#')]
    return lines[0], numpy.array([[float(x) for x in ln.split(',')[1:]] for ln in lines[1:]])


def test_fluxplot_tracer_is_the_scaled_table(tmp_path):
    from nemoflux_amd import fluxplot
    from nemoflux_amd.field import Field
    files = _h5_files()
    lines = "[(-100,-80),(100,-80),(0,80)],[(-180,-70),(-160,-10),(-35,40),(20,-50),(60,50),(180,40)]"
    out = str(tmp_path / 'tracer.csv')
    _quiet(fluxplot.main, lonLatPoints=lines, output=out, tracer='uo', tracerFile=files['uFile'], tracerRef=0.5,
           tracerScale=2.5, **files)
    head, table = _read_table(out)
    ff = _quiet(Field, files['tFile'], files['uFile'], files['vFile'], fluxplot.readTargets(lines)[0])
    ff.setTracer((files['uFile'], 'uo'), reference=0.5)
    want = ff.computeTracerAll()[0] * 2.5
    assert table.shape == want.shape == (3, 2)
    assert numpy.allclose(table, want, rtol=1e-14, atol=1e-14 * numpy.abs(want).max())
    assert numpy.abs(want).max() > 0
    with pytest.raises(RuntimeError, match='--zrange'):
        fluxplot.main(lonLatPoints=lines, tracer='uo', tracerFile=files['uFile'], zrange='0,10', **files)
