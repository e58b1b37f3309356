"""Depth-resolved transect fluxes (Field.computeFluxProfile, nf_field_compute_profile): row z of a profile is the flux that
level z alone carries.  Anchored bit for bit to computeFlux of a field whose only non-zero layer is z, checked against the
full-depth rows, the CPU oracle run on one level and the closed form of fluxexact; computing a profile changes nothing
else; sharded ranks add up to the single-rank profile; file-backed fields, depth bands and fluxplot --zrange."""
import ast
import os

import numpy
import pytest

from conftest import GOLDEN, case_box, load_golden, transect_xyz
from gpu_helpers import _field, _quiet, _resident

pytestmark = pytest.mark.gpu

PSI_ZT = "(1+10*z)*(t+1)*(cos(2*pi*y/360) + sin(2*pi*x/360))"
T_TRI = "(-100,-80),(100,-80),(0,80),(-100,-80)"
T_OPEN = "(-100,-80),(100,-80),(0,80)"
NX, NY, NZ, NT = 72, 36, 7, 3
FILL, MISSING = 1.e20, -999.


_CASES = {}


def _case(real, fill):
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


def _args(real, fill, resident, db=None):
    import torch
    blon, blat, db0, u, v = _case(real, fill)
    if resident:
        u, v = torch.from_numpy(u).cuda(), torch.from_numpy(v).cuda()
    return (blon, blat, db0 if db is None else db, u, v, [transect_xyz(T_OPEN), transect_xyz(T_TRI)])


def _kw(fill, sverdrup):
    kw = dict(sverdrup=sverdrup, readback=False)
    if fill:
        kw.update(fill_value=FILL, missing_value=MISSING)
    return kw


def _row(f):
    """the [segments | transects] row of the last computeFlux"""
    return numpy.array(f._row[:f._rowlen])


def _profile_rows(f, t):
    tot, seg = f.computeFluxProfile(t)
    return numpy.concatenate([seg, tot], axis=1)


@pytest.mark.parametrize('resident', [True, False], ids=['hbm', 'host'])
@pytest.mark.parametrize('fill', [False, True], ids=['nofill', 'fill'])
@pytest.mark.parametrize('sverdrup', [False, True], ids=['m2', 'sv'])
@pytest.mark.parametrize('real', ['float64', 'float32'])
def test_profile_level_is_the_one_layer_field_bit_for_bit(real, sverdrup, fill, resident):
    """Test A: row z of computeFluxProfile(t) == the computeFlux(t) row of a field whose deptht_bounds are collapsed so that
    only level z has a thickness (fma(0, x, acc) == acc: that field's vertical integral is level z's term exactly)."""
    db = numpy.asarray(_case(real, fill)[2], dtype=numpy.float64)
    f = _field(*_args(real, fill, resident), **_kw(fill, sverdrup))
    profiles = [_profile_rows(f, t) for t in range(NT)]
    for z in range(NZ):
        dz = db.copy()
        for k in range(NZ):
            if k != z:
                dz[k, 1] = dz[k, 0]
        assert (dz[:, 1] - dz[:, 0] != 0).sum() == 1
        one = _field(*_args(real, fill, resident, db=dz), **_kw(fill, sverdrup))
        for t in range(NT):
            one.computeFlux(t)
            assert numpy.array_equal(profiles[t][z], _row(one)), (z, t)


@pytest.mark.parametrize('fill', [False, True], ids=['nofill', 'fill'])
@pytest.mark.parametrize('real', ['float64', 'float32'])
def test_profile_sums_to_the_full_depth_row(real, fill):
    f = _field(*_args(real, fill, True), **_kw(fill, False))
    for t in range(NT):
        prof = _profile_rows(f, t)
        f.computeFlux(t)
        full = _row(f)
        assert numpy.abs(full).max() > 0
        assert numpy.allclose(prof.sum(axis=0), full, rtol=1e-13, atol=1e-13 * numpy.abs(full).max())
        if not fill and real == 'float64':
            # T_TRI is closed and the float64 flow has no sources: every level's loop is ~0 out of terms like the open line's
            # (float32 u, v are rounded independently: their loop is a few 1e-9, in the full-depth row as much as here)
            assert numpy.all(numpy.abs(prof[:, -1]) <= 1e-13 * numpy.abs(full).max())


def _golden_case(cases, name):
    return [c for c in cases if c['name'] == name][0], load_golden(name)


@pytest.mark.parametrize('name', ['rot36_zt', 'def36_zt', 'sv36_land', 'wrap36_zt'])
def test_profile_levels_against_the_oracle(name, oracle, cases):
    """Each level against the CPU oracle run on that level alone: vertical_integral(u[t, z:z+1], thickness[z:z+1]), then
    edge_flux and get_integral; the bound of the row checks of test_gpu_parity (A7: 1e-12 sum|w f|)."""
    m, g = _golden_case(cases, name)
    names = list(m['transects'])
    trs = [transect_xyz(m['transects'][n]['points']) for n in names]
    f = _field(g['bounds_lon'], g['bounds_lat'], g['deptht_bounds'], g['u'], g['v'], trs, sverdrup=m['sverdrup'],
               fill_value=m['fill_value'])
    pts = oracle.assemble_points(g['bounds_lon'], g['bounds_lat'])
    ows = [oracle.polyline_weights(pts, xyz) for xyz in trs]
    arc = f.arcLengths
    th = g['thickness']
    for t in range(m['nt']):
        tot, seg = f.computeFluxProfile(t)
        for z in range(m['nz']):
            st = oracle.EdgeFluxState(m['ny'], m['nx'])
            oracle.edge_flux(st, oracle.vertical_integral(g['u'][t, z:z + 1], th[z:z + 1], m['fill_value']),
                             oracle.vertical_integral(g['v'][t, z:z + 1], th[z:z + 1], m['fill_value']), arc, m['sverdrup'])
            data = st.integratedVelocity
            for i, ow in enumerate(ows):
                otot, osegs = oracle.get_integral(ow, data, True)
                bound = 1e-12 * max(numpy.abs(ow.weight * data.reshape(-1)[ow.cell_edge]).sum(), 1e-300)
                assert abs(tot[z, i] - otot) <= bound, (t, z, i)
                got = seg[z, f._tr_off[i]:f._tr_off[i + 1]]
                assert numpy.all(numpy.abs(got - osegs) <= bound), (t, z, i)


@pytest.mark.parametrize('name', ['def36_zt', 'reg16', 'wrap36_zt'])
def test_profile_levels_against_the_closed_form(name, cases):
    """The transect total of level k is the k-th term of fluxexact's inner loop (fluxexact.py:36-46):
    (psi(B, z_half[k], t) - psi(A, z_half[k], t)) * thickness[k]."""
    from nemoflux_amd import _expr
    m, g = _golden_case(cases, name)
    names = list(m['transects'])
    f = _field(g['bounds_lon'], g['bounds_lat'], g['deptht_bounds'], g['u'], g['v'],
               [transect_xyz(m['transects'][n]['points']) for n in names], sverdrup=m['sverdrup'], fill_value=m['fill_value'])
    zmin, zmax = case_box(m)[4:]
    nz, nt = m['nz'], m['nt']
    dz = (zmax - zmin) / float(nz)
    zhalf = numpy.array([zmin + (k + 0.5) * dz for k in range(nz)])
    thickness = -(numpy.array([zmin + k * dz for k in range(nz)]) - numpy.array([zmin + (k + 1) * dz for k in range(nz)]))
    code = _expr.compile_function(m['psi'])
    amp = max([1.0] + [abs(x) for n in names for x in (m['transects'][n]['fluxexact'] or [])])
    for t in range(nt):
        tot, _ = f.computeFluxProfile(t)
        for i, n in enumerate(names):
            xy = numpy.array(ast.literal_eval(m['transects'][n]['points']), dtype=numpy.float64)
            for k in range(nz):
                phiA = _expr.evaluate(code, x=xy[0, 0], y=xy[0, 1], z=zhalf[k], t=t, nt=nt)
                phiB = _expr.evaluate(code, x=xy[-1, 0], y=xy[-1, 1], z=zhalf[k], t=t, nt=nt)
                exact = float((phiB - phiA) * thickness[k])
                assert abs(tot[k, i] - exact) <= 1e-13 * max(amp, abs(exact)), (t, n, k)


@pytest.mark.parametrize('compact', [False, True])
@pytest.mark.parametrize('resident', [True, False], ids=['hbm', 'host'])
def test_profiles_leave_everything_else_alone(compact, resident):
    """computeFluxProfile calls between computeFlux, computeAll and read-backs: rows, planes, |.| arrays and the running max
    equal those of a field that never computed a profile, bit for bit."""
    args = _args('float64', True, resident)
    a = _field(*args, compact=compact, **_kw(True, False))
    b = _field(*args, compact=compact, **_kw(True, False))
    p0 = _profile_rows(a, 1)
    for step in ('flux1', 'all', 'flux0', 'read', 'all', 'flux2', 'read'):
        _profile_rows(a, 2)
        if step == 'all':
            assert all(numpy.array_equal(x, y) for x, y in zip(a.computeAll(), b.computeAll()))
            _profile_rows(a, 0)
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
    assert numpy.array_equal(_profile_rows(a, 1), p0)          # and a profile is reproducible


@pytest.mark.parametrize('world', [2, 3, 5])
def test_sharded_profiles_add_up_bit_for_bit(world):
    """Slab ranges that cut inside a step: every rank's profile is exactly zero on the levels it does not own, and the
    ranks' profiles sum to the single-rank profile bit for bit (each level comes from one rank)."""
    import torch
    from nemoflux_amd.dist import slab_range
    args = _args('float64', True, True)
    full = _field(*args, **_kw(True, False))
    want = [_profile_rows(full, t) for t in range(NT)]
    acc = [numpy.zeros_like(w) for w in want]
    for r in range(world):
        sr = slab_range(NT, NZ, r, world)
        part = _field(*args, slab_range=sr, **_kw(True, False))
        for t in range(NT):
            out = torch.full((NZ, part._rowlen), numpy.nan, dtype=torch.float64, device='cuda')
            tot, seg = part.computeFluxProfile(t, out=out)
            rows = out.cpu().numpy()
            assert numpy.array_equal(rows, numpy.concatenate([seg, tot], axis=1))
            for z in range(NZ):
                s = t * NZ + z
                if not sr[0] <= s < sr[1]:
                    assert numpy.all(rows[z] == 0), (r, t, z)
                else:
                    assert numpy.array_equal(rows[z], want[t][z]), (r, t, z)
            acc[t] += rows
    for t in range(NT):
        assert numpy.array_equal(acc[t], want[t])


def test_file_backed_profile_equals_from_arrays():
    """Field(tFile, uFile, vFile) on the NetCDF-4-style triple (uo chunked, shuffled and deflated, inflated step by step)
    gives the profile of fromArrays on the decoded arrays, bit for bit, in any step order."""
    from nemoflux_amd import hdf5min
    from nemoflux_amd.field import Field
    h5 = os.path.join(GOLDEN, 'h5')
    tr = [transect_xyz(T_OPEN), transect_xyz("(-180,-70),(-160,-10),(-35,40),(20,-50),(60,50),(180,40)")]
    ff = _quiet(Field, os.path.join(h5, 'nemo_T.h5'), os.path.join(h5, 'nemo_U.h5'), os.path.join(h5, 'nemo_V.h5'), tr)
    with hdf5min.File(os.path.join(h5, 'nemo_T.h5')) as f:
        blon, blat = f.datasets['bounds_lon'].read(), f.datasets['bounds_lat'].read()
        db = f.datasets['deptht_bounds'].read()
    with hdf5min.File(os.path.join(h5, 'nemo_U.h5')) as f:
        u = numpy.array(f.datasets['uo'].read())
        fill = float(f.datasets['uo'].fill_value)
    with hdf5min.File(os.path.join(h5, 'nemo_V.h5')) as f:
        v = numpy.array(f.datasets['vo'].read())
    fa = _field(blon, blat, db, u, v, tr, fill_value=fill)
    assert ff.nz == 2 and (u == numpy.float32(1.e20)).any()
    for t in (2, 0, 1, 1):
        pf, pa = ff.computeFluxProfile(t), fa.computeFluxProfile(t)
        assert numpy.array_equal(pf[0], pa[0]) and numpy.array_equal(pf[1], pa[1]), t
        assert numpy.abs(pf[0]).max() > 0
    assert ff.computeFlux(1) == fa.computeFlux(1)


@pytest.mark.parametrize('band', [(0.2, 0.55), (0.3, 2.0), (0.0, 0.25), (0.4, 0.4 + 1e-3)])
def test_depth_band_equals_a_clipped_column(band):
    """depthBandFlux(profile, ztop, zbot) == computeFlux of a field whose layers are clipped to the band (1e-13 relative)."""
    ztop, zbot = band
    args = _args('float64', True, True)
    f = _field(*args, **_kw(True, False))
    db = numpy.asarray(args[2], dtype=numpy.float64)
    clipped = numpy.stack([numpy.clip(db[:, 0], ztop, zbot), numpy.clip(db[:, 1], ztop, zbot)], axis=1)
    c = _field(*args[:2], clipped, *args[3:], **_kw(True, False))
    full = _field(*args, **_kw(True, False))
    for t in range(NT):
        tot, seg = f.computeFluxProfile(t)
        full.computeFlux(t)
        scale = numpy.abs(_row(full)).max()
        got = numpy.concatenate([f.depthBandFlux(seg, ztop, zbot), f.depthBandFlux(tot, ztop, zbot)])
        c.computeFlux(t)
        want = _row(c)
        assert numpy.abs(want).max() > 0
        assert numpy.allclose(got, want, rtol=1e-13, atol=1e-13 * scale), (band, t)


def _read_table(path):
    with open(path) as fh:
        lines = [ln for ln in fh.read().splitlines() if not ln.startswith('#')]
    return lines[0], numpy.array([[float(x) for x in ln.split(',')[1:]] for ln in lines[1:]])


def test_fluxplot_zrange_over_the_whole_column_is_the_full_table(tmp_path):
    from nemoflux_amd import fluxplot
    h5 = os.path.join(GOLDEN, 'h5')
    files = dict(tFile=os.path.join(h5, 'nemo_T.h5'), uFile=os.path.join(h5, 'nemo_U.h5'), vFile=os.path.join(h5, 'nemo_V.h5'))
    lines = "[(-100,-80),(100,-80),(0,80)],[(-180,-70),(-160,-10),(-35,40),(20,-50),(60,50),(180,40)]"
    full, band, half = (str(tmp_path / n) for n in ('full.csv', 'band.csv', 'half.csv'))
    _quiet(fluxplot.main, lonLatPoints=lines, output=full, **files)
    _quiet(fluxplot.main, lonLatPoints=lines, output=band, zrange='-10,1000', **files)
    hf, tf = _read_table(full)
    hb, tb = _read_table(band)
    assert hf == hb and tf.shape == tb.shape == (3, 2)
    assert numpy.allclose(tb, tf, rtol=1e-14, atol=1e-14 * numpy.abs(tf).max())
    # a band that holds the upper level only: the level-0 totals
    from nemoflux_amd.field import Field
    ff = _quiet(Field, files['tFile'], files['uFile'], files['vFile'], fluxplot.readTargets(lines)[0])
    z0, z1 = (float(x) for x in ff.bounds_depth[0])
    _quiet(fluxplot.main, lonLatPoints=lines, output=half, zrange=f'{z0!r},{z1!r}', **files)
    want = numpy.array([ff.computeFluxProfile(t)[0][0] for t in range(ff.nt)])
    assert numpy.allclose(_read_table(half)[1], want, rtol=1e-14, atol=1e-14 * numpy.abs(want).max())
    assert not numpy.allclose(want, tf, rtol=1e-6, atol=0)
