"""Isosurface and mixed-layer depths through Field: a Field whose depth surfaces are an IsoDepth / MixedLayerDepth against a
fresh Field whose surfaces are the (nt, ny, nx) series of tests/iso_depth_reference.py as arrays -- every row array_equal, in
the volume and the carried form, with the level thicknesses and with cell thicknesses, both dtypes, the sources in HBM, on the
host, in an .npz bundle and in classic NetCDF-3 files, a Sigma source (against tests/eos_reference.py), m = 1, 3 and 8, a derived
item next to a plain device surface, the steps visited 2, 0, 2, 1; getDepthSurfaces; two sharded halves; timeMean and
meanEddySplit; re-use of one handle; refusals; fluxplot --iso-depth and --mixed-layer.

Grids 72 x 36 x 7 x 3 and 73 x 37 x 7 x 3 with the three transects of tests/test_gpu_surface_transport.py."""
import numpy
import pytest

from conftest import write_classic_triple
from gpu_helpers import _field, _on, _quiet, _resident, _rows
import eos_reference as eos
import iso_depth_reference as ref
from surface_transport_reference import surface_values
from test_gpu_cellthick import FILL, MISSING, T_OPEN, T_SEAM, TFILL, TMISSING, _case
from test_gpu_depth_remap import DB, _check, _make, _set_thickness, _set_tracer
from test_gpu_gross import GRIDS, NT, NZ, _tau, _uv
from test_gpu_surface_transport import _reference, _st

pytestmark = pytest.mark.gpu

STEPS = (2, 0, 2, 1)
ZREF = 0.625          # ref.ZREF / 16: the thicknesses of these grids are sixteenths of those of the raw cases
TOP = -0.25
_SERIES = {}


def _series(real, grid, m, sense, relative, form):
    """(tau (NT, NZ, ny, nx), e3t (NT, NZ, ny, nx) or None, values): one raw case per step, the thicknesses scaled by 1 / 16"""
    key = (real, grid, m, sense, relative, form)
    if key not in _SERIES:
        nx, ny = grid
        steps = [ref.make_case(real, NZ, ny, nx, m, sense, relative, form, seed=100 * t) for t in range(NT)]
        tau = numpy.stack([s[0] for s in steps])
        e3t = numpy.stack([s[2] for s in steps]) / numpy.dtype(real).type(16) if form == 'e3t' else None
        _SERIES[key] = (tau, e3t, steps[0][3])
    return _SERIES[key]


def _want(tau, e3t, values, sense, relative, thickness, tm=(ref.TFILL, ref.TMISSING), em=(ref.EFILL, ref.EMISSING), top=TOP,
          zref=ZREF):
    """the restatement's (NT, m, ny, nx) series; a static e3t (NZ, ny, nx) serves every step"""
    return numpy.stack([ref.iso_depth(tau[t], values, sense, thickness=None if e3t is not None else thickness,
                                      e3t=None if e3t is None else (e3t[t] if e3t.ndim == 4 else e3t), top=top,
                                      relative=relative, zref=zref, tau_markers=tm, e3t_markers=em) for t in range(tau.shape[0])])


def _arrays(f, s, resident=True, top=TOP):
    """the Field gets the series s (NT, m, ny, nx) as one plain array per surface"""
    f.setDepthSurfaces([_on(numpy.ascontiguousarray(s[:, k]), resident) for k in range(s.shape[1])], top=top)


def _homes(real, grid, home, tau, e3t, tmp_path):
    """(tracer, e3t, keyword arguments of IsoDepth, (tau, e3t, tracer markers, e3t markers) as the restatement takes them)"""
    tm, em = (ref.TFILL, ref.TMISSING), (ref.EFILL, ref.EMISSING)
    kw = dict(fill_value=tm[0], missing_value=tm[1])
    if e3t is not None:
        kw.update(e3t_fill_value=em[0], e3t_missing_value=em[1])
    if home in ('hbm', 'host'):
        return _on(tau, home == 'hbm'), None if e3t is None else _on(e3t, home == 'hbm'), kw, (tau, e3t, tm, em)
    if home == 'npz':                 # the markers come from the file
        path = str(tmp_path / 'TE.npz')
        fv = lambda name, a, b: {f'_FillValue_{name}': numpy.array(a), f'_missing_value_{name}': numpy.array(b)}   # noqa: E731
        more = {} if e3t is None else dict(e3t=e3t, **fv('e3t', *em))
        numpy.savez(path, thetao=tau, **fv('thetao', *tm), **more)
        return (path, 'thetao'), None if e3t is None else (path, 'e3t'), {}, (tau, e3t, tm, em)
    # classic NetCDF-3 record variables, float32, read one step at a time: the tracer travels as the U file's variable (one
    # marker, its _FillValue), e3t as the V file's (NaN only); the writer adds its own land block to both
    assert real == 'float32'
    blon, blat = _case(real, grid)[:2]
    tau1 = numpy.where(tau == numpy.float32(tm[0]), numpy.float32(1.e20), tau)
    e1 = numpy.ones_like(tau) if e3t is None else numpy.where((e3t == numpy.float32(em[0])) | (e3t == numpy.float32(em[1])),
                                                              numpy.float32(numpy.nan), e3t)
    paths, tf, ef = write_classic_triple(tmp_path, dict(u=tau1, v=e1, bounds_lon=blon, bounds_lat=blat, deptht_bounds=DB))
    return (paths['U'], 'uo'), None if e3t is None else (paths['V'], 'vo'), {}, (tf, None if e3t is None else ef, (1.e20,), ())


CASES = [(real, grid, home) for real in ('float64', 'float32') for grid in GRIDS for home in ('hbm', 'host', 'npz')]
CASES += [('float32', grid, 'classic') for grid in GRIDS]


@pytest.mark.parametrize('real,grid,home', CASES, ids=[f'{r}-{g[0]}x{g[1]}-{h}' for r, g, h in CASES])
def test_field_with_an_iso_depth_gives_the_rows_of_the_restatements_series(real, grid, home, tmp_path):
    """two settings per case -- the level thicknesses and e3t, absolute and relative, rising and falling, m going round 1, 3,
    8 -- each in the volume and the carried form, with and without a time-varying cell thickness, the steps visited 2, 0, 2, 1"""
    from nemoflux_amd.surfaces import IsoDepth
    resident = home == 'hbm'
    n = CASES.index((real, grid, home))
    carried = _tau(real, grid)
    for k, form in enumerate(('levels', 'e3t')):
        m, sense, relative = (1, 3, 8)[(n + k) % 3], (1, -1)[(n + k) % 2], bool((n // 2 + k) % 2)
        tau, e3t, values = _series(real, grid, m, sense, relative, form)
        tracer, thick, kw, (tau_r, e3t_r, tm, em) = _homes(real, grid, home, tau, e3t, tmp_path)
        f, g = _make(real, grid, resident, sverdrup=True), _make(real, grid, resident, sverdrup=True)
        want_s = _want(tau_r, e3t_r, values, sense, relative, f.thickness, tm, em)
        ok = numpy.isfinite(want_s)
        assert 0.5 < ok.mean() < 0.97 and want_s.dtype == numpy.dtype(real) and len(numpy.unique(want_s[ok])) > 100
        for x in (f, g):
            _set_tracer(x, carried, resident)
        f.setDepthSurfaces([IsoDepth(tracer, values, sense, e3t=thick, relative=relative, zref=ZREF, **kw)], top=TOP)
        _arrays(g, want_s, resident)
        assert f._surfaces['derived'] and not g._surfaces['derived'] and len(f._surfaces['items']) == m
        for t in STEPS:
            label = (form, m, sense, relative, t)
            for carry in (False, True):
                want = _st(g, t, carry)
                assert numpy.abs(want).max() > 0 and (numpy.abs(want[:m + 1]).max(axis=1) > 0).sum() >= min(m, 2), label
                assert numpy.array_equal(_st(f, t, carry), want), label
            assert ref.same_bits(f.getDepthSurfaces(t), want_s[t]), label
            assert ref.same_bits(g.getDepthSurfaces(t), want_s[t]), label
            for x in (f, g):
                _set_thickness(x, real, grid, resident, 'timevarying')
            for carry in (False, True):
                want = _st(g, t, carry)
                assert numpy.abs(want).max() > 0 and numpy.array_equal(_st(f, t, carry), want), label
            for x in (f, g):
                x.setCellThickness(None, None)


@pytest.mark.parametrize('pref', [0., 2000.])
@pytest.mark.parametrize('real,home', [('float64', 'hbm'), ('float32', 'host'), ('float32', 'npz')])
def test_a_sigma_source_and_the_mixed_layer_depth(real, home, pref, tmp_path):
    """IsoDepth(Sigma(thetao, so, pref), three isopycnals) and MixedLayerDepth(thetao, so) next to a plain device surface"""
    from nemoflux_amd.eos import Sigma
    from nemoflux_amd.surfaces import IsoDepth, MixedLayerDepth
    from test_gpu_eos import SFILL, SMISSING, THFILL_, THMISS_, _theta_salt
    grid = GRIDS[1]
    th, sa = _theta_salt(real, grid)
    tm, sm = (THFILL_, THMISS_), (SFILL, SMISSING)
    kw = dict(fill_value=tm[0], missing_value=tm[1], so_fill_value=sm[0], so_missing_value=sm[1])
    if home == 'npz':
        path = str(tmp_path / 'TS.npz')
        fv = lambda name, a, b: {f'_FillValue_{name}': numpy.array(a), f'_missing_value_{name}': numpy.array(b)}   # noqa: E731
        numpy.savez(path, thetao=th, so=sa, **fv('thetao', *tm), **fv('so', *sm))
        thetao, so, kw = (path, 'thetao'), (path, 'so'), {}
    else:
        thetao, so = _on(th, home == 'hbm'), _on(sa, home == 'hbm')
    sig = eos.sigma(th, sa, pref, tm, sm)
    good = numpy.isfinite(sig)
    values = [float(x) for x in numpy.quantile(sig[good], [0.4, 0.6, 0.8])]
    f, g = _make(real, grid, True, sverdrup=True), _make(real, grid, True, sverdrup=True)
    iso = _want(sig, None, values, 1, False, f.thickness, (), ())
    mld = _want(sig, None, [0.03, 2.0], 1, True, f.thickness, (), ())
    assert numpy.isfinite(iso).mean() > 0.5 and len(numpy.unique(iso[numpy.isfinite(iso)])) > 100
    assert len(numpy.unique(mld[numpy.isfinite(mld)])) > 100
    plain = numpy.ascontiguousarray(iso[:, 1] + numpy.dtype(real).type(0.5))
    f.setDepthSurfaces([IsoDepth(Sigma(thetao, so, pref, **kw), values, 'rising', zref=ZREF)], top=TOP)
    _arrays(g, iso)
    for t in STEPS:
        assert numpy.array_equal(_st(f, t), _st(g, t)) and ref.same_bits(f.getDepthSurfaces(t), iso[t]), t
    if pref == 0.:
        f.setDepthSurfaces([MixedLayerDepth(thetao, so, delta=[0.03, 2.0], zref=ZREF, **kw), _on(plain, True)], top=TOP)
    else:
        f.setDepthSurfaces([IsoDepth(Sigma(thetao, so, pref, **kw), [0.03, 2.0], 1, relative=True, zref=ZREF), _on(plain, True)],
                           top=TOP)
    _arrays(g, numpy.concatenate([mld, plain[:, None]], axis=1))
    assert len(f._surfaces['items']) == 3
    for t in STEPS:
        want = _st(g, t)
        assert numpy.abs(want).max() > 0 and numpy.array_equal(_st(f, t), want), t
        assert ref.same_bits(f.getDepthSurfaces(t), numpy.concatenate([mld[t], plain[t][None]])), t


@pytest.mark.parametrize('real', ['float64', 'float32'])
def test_two_sharded_halves_add_up_to_the_unsharded_rows(real):
    """derived surfaces read whole columns of their own sources, so a rank's rows are those of the array-built Field under
    the same slab range, bit for bit; the halves add up to the unsharded rows as in tests/test_gpu_surface_transport.py"""
    from nemoflux_amd.dist import slab_range
    from nemoflux_amd.surfaces import IsoDepth
    grid, world, m = GRIDS[1], 2, 8
    u, v = _uv(real, grid)
    carried = _tau(real, grid)
    tau, e3t, values = _series(real, grid, m, 1, False, 'e3t')

    def make(derived, **kw):
        f = _make(real, grid, True, **kw)
        _set_tracer(f, carried, True)
        if derived:
            f.setDepthSurfaces([IsoDepth(_on(tau, True), values, 1, e3t=e3t, fill_value=ref.TFILL, missing_value=ref.TMISSING,
                                         e3t_fill_value=ref.EFILL, e3t_missing_value=ref.EMISSING)], top=TOP)
        else:
            _arrays(f, s)
        return f

    full = make(True)
    s = _want(tau, e3t, values, 1, False, full.thickness)
    want = numpy.array([[_st(full, t, carry) for carry in (False, True)] for t in range(NT)])
    acc = numpy.zeros_like(want)
    for rank in range(world):
        sr = slab_range(NT, NZ, rank, world)
        part, arr = make(True, slab_range=sr), make(False, slab_range=sr)
        for t in range(NT):
            for k, carry in enumerate((False, True)):
                got = _st(part, t, carry)
                assert numpy.array_equal(got, _st(arr, t, carry)), (rank, t, carry)
                acc[t, k] += got
    r = _reference(full)
    arrays = {'uo': u, 'vo': v, 'tracer': carried, 'surface': s}
    for t in range(NT):
        mags = r.surface_step(surface_values(arrays, t), m, top=TOP)
        for k, nm in enumerate(('volume', 'carried')):
            _check(acc[t, k], want[t, k], mags[nm][1], f'two halves, {nm} t={t}')


@pytest.mark.parametrize('real', ['float64', 'float32'])
def test_time_mean_and_mean_eddy_split_carry_derived_surfaces(real):
    from nemoflux_amd.surfaces import IsoDepth
    grid, m = GRIDS[0], 3
    select, weights = [0, 2], [1., 3.]
    carried = _tau(real, grid)
    tau, _, values = _series(real, grid, m, -1, True, 'levels')
    for home in (True, False):
        f, g = _make(real, grid, True, sverdrup=True), _make(real, grid, True, sverdrup=True)
        for x in (f, g):
            _set_tracer(x, carried, True)
        f.setDepthSurfaces([IsoDepth(_on(tau, home), values, -1, relative=True, zref=ZREF, fill_value=ref.TFILL,
                                     missing_value=ref.TMISSING)], top=TOP)
        _arrays(g, _want(tau, None, values, -1, True, f.thickness))
        mf, mg = _quiet(f.timeMean), _quiet(g.timeMean)
        assert mf._surfaces['nt'] == 1 and mf._surfaces['top'] == TOP and len(mf._surfaces['items']) == m
        for a, b in zip(mf._surfaces['items'], mg._surfaces['items']):
            assert ref.same_bits(numpy.asarray(a), numpy.asarray(b)) and numpy.isfinite(numpy.asarray(a)).mean() > 0.5
        for carry in (False, True):
            df = _quiet(f.meanEddySplit, 'computeSurfaceTransport', select=select, weights=weights, carry=carry)
            dg = _quiet(g.meanEddySplit, 'computeSurfaceTransport', select=select, weights=weights, carry=carry)
            for part in ('total', 'mean', 'eddy'):
                assert numpy.abs(_rows(dg[part])).max() > 0 and numpy.array_equal(_rows(df[part]), _rows(dg[part])), (carry, part)


def test_reuse_of_one_handle_equals_fresh_handles():
    """IsoDepth -> plain arrays -> None -> an IsoDepth with other values and another source home, on one handle; the other
    products and the resident planes are unchanged by it"""
    from nemoflux_amd.surfaces import IsoDepth
    real, grid = 'float32', GRIDS[1]
    carried = _tau(real, grid)
    tau, e3t, values = _series(real, grid, 3, 1, False, 'e3t')
    tau2, _, values2 = _series(real, grid, 8, -1, True, 'levels')
    marks = dict(fill_value=ref.TFILL, missing_value=ref.TMISSING)
    emarks = dict(e3t_fill_value=ref.EFILL, e3t_missing_value=ref.EMISSING)

    def fresh(s):
        x = _make(real, grid, True, sverdrup=True)
        _set_tracer(x, carried, True)
        if s is not None:
            _arrays(x, s)
        return x

    def rows(x):
        return [_st(x, t, carry) for t in (1, 2) for carry in (False, True)]

    def others(x):
        return [_rows(x.computeFluxProfile(1)), _rows(x.computeTracerProfile(2)), _rows(x.computeTracerFlux(0))]

    f = fresh(None)
    s1 = _want(tau, e3t, values, 1, False, f.thickness)
    s2 = s1 + numpy.float32(0.25)
    s3 = _want(tau2, None, values2, -1, True, f.thickness)
    before = others(f)
    planes = _resident(f)
    stages = [(lambda: f.setDepthSurfaces([IsoDepth(_on(tau, True), values, 1, e3t=_on(e3t, True), **marks, **emarks)], top=TOP), s1),
              (lambda: _arrays(f, s2), s2), (lambda: f.setDepthSurfaces(None), None),
              (lambda: f.setDepthSurfaces([IsoDepth(tau2, values2, -1, relative=True, zref=ZREF, **marks)], top=TOP), s3)]
    seen = []
    for change, s in stages:
        change()
        if s is None:
            with pytest.raises(RuntimeError, match='setDepthSurfaces first'):
                f.computeSurfaceTransport(0)
            continue
        got, want = rows(f), rows(fresh(s))
        for a, b in zip(got, want):
            assert numpy.abs(b).max() > 0 and numpy.array_equal(a, b)
        seen.append(got[0])
    assert not numpy.array_equal(seen[0], seen[1]) and seen[2].shape != seen[0].shape
    f.computeFluxProfile(0)        # the resident step is that of the last volume call of `planes`
    for a, b in zip(others(f), before):
        assert numpy.array_equal(a, b)
    f.computeTracerFlux(0)
    for a, b in zip(_resident(f), planes):
        assert numpy.array_equal(a, b)


def test_refusals():
    from nemoflux_amd.eos import Sigma
    from nemoflux_amd.surfaces import IsoDepth, MixedLayerDepth
    real, grid = 'float64', GRIDS[0]
    tau, e3t, values = _series(real, grid, 3, 1, False, 'e3t')
    f = _make(real, grid, True)
    d_tau = _on(tau, True)
    for bad, words in ((IsoDepth(tau[:, :-1], values, 1), 'surface 0: the tracer of the IsoDepth has shape'),
                       (IsoDepth(tau[:-1], values, 1), 'surface 0: the tracer of the IsoDepth has shape'),
                       (IsoDepth(tau.astype(numpy.float32), values, 1), 'the tracer of the IsoDepth is float32, uo/vo are float64'),
                       (IsoDepth(d_tau, values, 1, e3t=e3t[:2]), 'the e3t of the IsoDepth has shape'),
                       (IsoDepth(d_tau, values, 1, e3t=e3t.astype(numpy.float32)), 'the e3t of the IsoDepth is float32'),
                       (MixedLayerDepth(tau[:, 1:], tau[:, 1:]), 'thetao and so of the Sigma of surface 0 have shape'),
                       (IsoDepth(Sigma(tau.astype(numpy.float32), tau.astype(numpy.float32)), values, 1), 'are float32, uo/vo')):
        with pytest.raises(RuntimeError, match=words):
            f.setDepthSurfaces([bad])
        assert f._surfaces is None
    with pytest.raises(RuntimeError, match='values'):
        IsoDepth(d_tau, [1.0, numpy.inf], 1)
    with pytest.raises(RuntimeError, match='sense must be'):
        IsoDepth(d_tau, values, 0)
    plane = _on(numpy.zeros((NT, grid[1], grid[0])), True)
    with pytest.raises(RuntimeError, match='1 to 8 surfaces, got 9'):
        f.setDepthSurfaces([IsoDepth(d_tau, [1., 2., 3., 4., 5.], 1), IsoDepth(d_tau, values, 1), plane])
    # today's words for mixing with host arrays and with static items
    with pytest.raises(RuntimeError, match='all be host arrays .or files. or all be device arrays'):
        f.setDepthSurfaces([IsoDepth(d_tau, values, 1), numpy.zeros((NT, grid[1], grid[0]))])
    with pytest.raises(RuntimeError, match='all static or all per time step'):
        f.setDepthSurfaces([IsoDepth(d_tau, values, 1), _on(numpy.zeros((grid[1], grid[0])), True)])
    with pytest.raises(RuntimeError, match='setDepthSurfaces first'):
        f.getDepthSurfaces(0)
    f.setDepthSurfaces([IsoDepth(d_tau, values, 1), plane])
    with pytest.raises(RuntimeError, match='tIndex must be'):
        f.getDepthSurfaces(NT)
    with pytest.raises(RuntimeError, match='setTracer first'):
        f.computeSurfaceTransport(0, carry=True)
    assert f.getDepthSurfaces(1).shape == (4, grid[1], grid[0]) and numpy.abs(_st(f, 1)).max() > 0


# ---- the command line --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('kind', ['iso', 'iso-sigma-relative-e3t', 'mixed-layer'])
def test_fluxplot_iso_depth_and_mixed_layer_write_the_rows_of_the_array_built_field(tmp_path, kind):
    from nemoflux_amd import fluxplot
    from test_gpu_eos import SFILL, SMISSING, THFILL_, THMISS_, _theta_salt
    real, grid = 'float32', GRIDS[0]
    blon, blat = _case(real, grid)[:2]
    u, v = _uv(real, grid)
    th, sa = _theta_salt(real, grid)
    tm, sm = (THFILL_, THMISS_), (SFILL, SMISSING)
    _, e3t, _ = _series(real, grid, 3, 1, False, 'e3t')
    paths = {k: str(tmp_path / f'{k}.npz') for k in 'TUV'}
    fv = lambda name, a, b: {f'_FillValue_{name}': numpy.array(a), f'_missing_value_{name}': numpy.array(b)}   # noqa: E731
    numpy.savez(paths['T'], bounds_lon=blon, bounds_lat=blat, deptht_bounds=DB, thetao=th, so=sa, e3t=e3t, **fv('thetao', *tm),
                **fv('so', *sm), **fv('e3t', ref.EFILL, ref.EMISSING))
    numpy.savez(paths['U'], uo=u, **fv('uo', FILL, MISSING))
    numpy.savez(paths['V'], vo=v, **fv('vo', FILL, MISSING))
    lines = '[' + T_OPEN + '],[' + T_SEAM + ']'
    out = str(tmp_path / 'iso.csv')
    thickness = DB[:, 1] - DB[:, 0]
    em = (ref.EFILL, ref.EMISSING)
    if kind == 'iso':
        kw = dict(isoDepth='20,12', isoOf='thetao', tracer='so', tracerRef=1.5, tracerScale=4.1e-3)
        s = _want(th, None, [20.0, 12.0], -1, False, thickness, tm, (), top=-1.5)
        labels = ['thetao=20', 'thetao=12']
    elif kind == 'mixed-layer':
        kw = dict(mixedLayer='thetao,so,0.5,0.625')
        s = _want(eos.sigma(th, sa, 0., tm, sm), None, [0.5], 1, True, thickness, (), (), top=-1.5)
        labels = ['mld']
    else:
        kw = dict(isoDepth='0.25,1', sigma='thetao,so,2000', isoRelative='0.625', isoE3t='e3t')
        s = _want(eos.sigma(th, sa, 2000., tm, sm), e3t, [0.25, 1.0], 1, True, None, (), em, top=-1.5)
        labels = ['sigma2@0.625+0.25', 'sigma2@0.625+1']
    m = s.shape[1]
    totals = _quiet(fluxplot.main, tFile=paths['T'], uFile=paths['U'], vFile=paths['V'], lonLatPoints=lines, output=out,
                    sverdrup=True, depthTop=-1.5, **kw)
    mem = _field(blon, blat, DB, u, v, fluxplot.readTargets(lines)[0], True, fill_value=FILL, missing_value=MISSING,
                 readback=False)
    if kind == 'iso':
        mem.setTracer(sa, fill_value=sm[0], missing_value=sm[1], reference=1.5)
    mem.setDepthSurfaces([numpy.ascontiguousarray(s[:, k]) for k in range(m)], top=-1.5)
    with open(out) as fh:
        text = fh.read().splitlines()
    assert text[1] == 'time,upper,lower,line0,line1'
    assert text[2].split(',')[1:3] == ['top', labels[0]] and text[2 + m].split(',')[1:3] == [labels[-1], 'bottom']
    assert totals.shape == (NT, m + 2, 2) and len(text) == 2 + NT * (m + 2)
    for t in range(NT):
        want = mem.computeSurfaceTransport(t, carry=kind == 'iso')[0] * (4.1e-3 if kind == 'iso' else 1.0)
        assert numpy.array_equal(totals[t], want) and (numpy.abs(want[:m + 1]).max(axis=1) > 0).all(), t
