"""z* thicknesses from the sea surface height through Field: a Field with setCellThickness(SshThickness(...)) against a fresh Field
whose e3u / e3v are the series of tests/ssh_thickness_reference.py given as arrays -- every product that takes a cell thickness
array_equal, both dtypes, ssh in HBM, on the host, in an .npz bundle and in a classic NetCDF-3 file, static and time-varying,
e3u0 / e3v0 given and e3t0 alone, with and without areas, the steps visited 2, 0, 2, 1; ssh = 0 over the level vector against
the Field without a cell thickness; two sharded halves; timeMean(thicknessWeighted=True), meanEddySplit and
meanEddyTracerTransport; re-use of one handle; the refusal of computeClassTransport; fluxplot --cell-thickness --ssh; a grid
of 1030 x 6 (float32: 1028 x 6), past one column chunk of the kernel.

The grids, transects and helpers are those of tests/test_gpu_face_thickness_field.py."""
import numpy
import pytest

from gpu_helpers import _field, _on, _quiet, _resident, _rows
import face_thickness_reference as fref
import ssh_thickness_reference as ref
from test_gpu_cellthick import FILL, MISSING, T_OPEN, T_SEAM, _case
from test_gpu_depth_remap import DB, TH
from test_gpu_face_thickness_field import PRODUCTS, STEPS, WIDE_GRID, _build, _flat, _same_products, _seam_rows
from test_gpu_gross import GRIDS, NT, NZ, _uv

pytestmark = pytest.mark.gpu

EM, SM = ref.EM, ref.SM
MARKS = dict(fill_value=EM[0], missing_value=EM[1], static_fill_value=SM[0], static_missing_value=SM[1])
# (the statics: e3u0 / e3v0 given or e3t0 alone, areas, supplied column depths, static or time-varying ssh)
CONFIGS = {'given': ('given', False, False, 'timevarying'), 'e3t0-areas': ('e3t0', True, False, 'timevarying'),
           'static-areas-depths': ('given', True, True, 'static')}
_SERIES, _WANT = {}, {}


def _series(real, grid):
    if (real, grid) not in _SERIES:
        _SERIES[real, grid] = ref.series(real, grid, NT, NZ)
    return _SERIES[real, grid]


def _statics(c, route, wrap=True):
    """(e3u0, e3v0, their markers) the kernel works on: the given pair, or NEMO's partial-step rule of e3t0"""
    if route == 'given':
        return c['e3u0'], c['e3v0'], SM
    u0, v0 = fref.face_thickness(c['e3t0'], 'min', wrap=wrap, markers=SM)
    return u0, v0, ()


def _want(real, grid, route, areas, supplied, ssh=None, markers=EM, key=None):
    """the restatement's (e3u, e3v) of the series' ssh or of the one given; with a key, computed once"""
    k = (real, grid, route, areas, supplied, key)
    if key is not None and k in _WANT:
        return _WANT[k]
    c = _series(real, grid)
    u0, v0, sm = _statics(c, route)
    got = ref.ssh_thickness(c['ssh'] if ssh is None else ssh, u0, v0, c['hu0'] if supplied else None,
                            c['hv0'] if supplied else None, c['areas'] if areas else None, markers=markers, static_markers=sm)
    if key is not None:
        _WANT[k] = got
    return got


def _descriptor(real, grid, home, config, tmp_path, ssh=None):
    """(the SshThickness as the home holds its inputs, the restatement's pair)"""
    from nemoflux_amd.thickness import SshThickness
    route, areas, supplied, kind = CONFIGS[config]
    c = _series(real, grid)
    if ssh is None:
        ssh = c['ssh'] if kind == 'timevarying' else c['ssh'][1]
    want = _want(real, grid, route, areas, supplied, ssh=ssh)
    if home in ('hbm', 'host'):
        put = lambda a: _on(a, home == 'hbm')       # noqa: E731
        kw = dict(e3t0=put(c['e3t0'])) if route == 'e3t0' else dict(e3u0=put(c['e3u0']), e3v0=put(c['e3v0']))
        if supplied:
            kw.update(hu0=put(c['hu0']), hv0=put(c['hv0']))
        if areas:
            kw.update(areas=tuple(put(a) for a in c['areas']))
        return SshThickness(put(ssh), **kw, **MARKS), want
    fv = lambda name, m: {f'_FillValue_{name}': numpy.array(m[0]), f'_missing_value_{name}': numpy.array(m[1])}   # noqa: E731
    mesh = str(tmp_path / f'mesh_{config}.npz')
    numpy.savez(mesh, e3u_0=c['e3u0'], e3v_0=c['e3v0'], e3t_0=c['e3t0'], hu_0=c['hu0'], hv_0=c['hv0'], e1e2t=c['areas'][0],
                e1e2u=c['areas'][1], e1e2v=c['areas'][2],
                **{k: x for n in ('e3u_0', 'e3v_0', 'e3t_0') for k, x in fv(n, SM).items()})
    kw = dict(e3t0=(mesh, 'e3t_0')) if route == 'e3t0' else dict(e3u0=(mesh, 'e3u_0'), e3v0=(mesh, 'e3v_0'))
    if supplied:
        kw.update(hu0=(mesh, 'hu_0'), hv0=(mesh, 'hv_0'))
    if areas:
        kw.update(areas=tuple((mesh, n) for n in ('e1e2t', 'e1e2u', 'e1e2v')))
    if home == 'npz':                 # the markers come from the files
        path = str(tmp_path / f'T_{config}.npz')
        numpy.savez(path, zos=ssh, **fv('zos', EM))
        return SshThickness((path, 'zos'), **kw), want
    # a classic NetCDF-3 record variable, float32, big-endian, read and byte-swapped whole into a host array, then staged plane
    # by plane; one marker, its _FillValue: the other marker's value is data
    assert real == 'float32' and ssh.ndim == 3
    path = _classic_ssh(tmp_path / f'ssh_{config}.nc', ssh)
    return SshThickness((path, 'zos'), **kw), _want(real, grid, route, areas, supplied, ssh=ssh, markers=(EM[0],))


def _classic_ssh(path, ssh):
    from scipy.io import netcdf_file
    nt, ny, nx = ssh.shape
    f = netcdf_file(str(path), 'w', version=2)
    for n, s in (('time_counter', None), ('y', ny), ('x', nx)):
        f.createDimension(n, s)
    tc = f.createVariable('time_counter', 'f8', ('time_counter',))
    var = f.createVariable('zos', 'f4', ('time_counter', 'y', 'x'))
    var._FillValue = numpy.float32(EM[0])
    tc[:] = numpy.arange(nt) * 86400.
    var[:] = ssh
    f.close()
    return str(path)


CASES = [(real, grid, home) for real in ('float64', 'float32') for grid in GRIDS for home in ('hbm', 'host', 'npz')]
CASES += [('float32', grid, 'classic') for grid in GRIDS]


@pytest.mark.parametrize('real,grid,home', CASES, ids=[f'{r}-{g[0]}x{g[1]}-{h}' for r, g, h in CASES])
def test_field_with_an_ssh_thickness_gives_the_products_of_the_restatements_series(real, grid, home, tmp_path):
    """the statics given and derived from e3t0, with and without areas, time-varying with the steps visited 2, 0, 2, 1 and
    computeAll over all of them; a static ssh with supplied column depths too"""
    resident = home == 'hbm'
    f, g = _build(real, grid, resident), _build(real, grid, resident)
    for config, (route, areas, supplied, kind) in CONFIGS.items():
        if kind == 'static' and home == 'classic':
            continue
        st, want = _descriptor(real, grid, home, config, tmp_path)
        statics = _statics(_series(real, grid), route)
        for w, F0 in zip(want, statics):
            assert w.dtype == numpy.dtype(real) and (w == 0).mean() > 0.05 and len(numpy.unique(w[numpy.isfinite(w)])) > 20
            assert (w != numpy.where(ref.present(F0, statics[2]), F0, 0)).mean() > 0.1        # ssh moves the thicknesses
        f.setCellThickness(st)
        g.setCellThickness(_on(want[0], resident), _on(want[1], resident))
        assert f._cell_thickness_lazy() == (kind == 'timevarying') and f._e3['nt'] == (NT if kind == 'timevarying' else 1)
        for t in (STEPS if kind == 'timevarying' else (1,)):
            _same_products(f, g, t, (config, kind))
        for a, b in zip(f.computeAll(), g.computeAll()):
            assert numpy.abs(b).max() > 0 and numpy.array_equal(a, b), config
        for a, b in zip(f.computeTracerAll(), g.computeTracerAll()):
            assert numpy.abs(b).max() > 0 and numpy.array_equal(a, b), config


@pytest.mark.parametrize('real', ['float64', 'float32'])
def test_a_wide_short_grid_past_one_column_chunk(real):
    """time-varying ssh in HBM, the statics from e3t0, with areas, on 1030 x 6 and 1028 x 6; T_SEAM runs through the last
    column, whose east faces take column 0 from another chunk: with the restatement's wrapX off its rows are other rows"""
    grid = WIDE_GRID[real]
    f, g = _build(real, grid), _build(real, grid)
    st, want = _descriptor(real, grid, 'hbm', 'e3t0-areas', None)
    f.setCellThickness(st)
    g.setCellThickness(_on(want[0], True), _on(want[1], True))
    assert f._cell_thickness_lazy() and f._e3['nt'] == NT
    for t in STEPS:
        _same_products(f, g, t, ('wide', real))
    c = _series(real, grid)
    u0, v0, sm = _statics(c, 'e3t0', wrap=False)
    off = ref.ssh_thickness(c['ssh'], u0, v0, areas=c['areas'], wrap=False, markers=EM, static_markers=sm)
    assert ref.same_bits(off[0][..., :-1], want[0][..., :-1]) and ref.same_bits(off[1], want[1])
    rows = _seam_rows(g)
    assert numpy.array_equal(_seam_rows(f), rows) and numpy.abs(rows).max() > 0
    g.setCellThickness(_on(off[0], True), _on(off[1], True))
    assert not numpy.array_equal(_seam_rows(g), rows)


@pytest.mark.parametrize('real', ['float64', 'float32'])
def test_wrap_off_a_static_host_array_of_another_dtype_and_the_engines_buffers(real):
    """wrapX off, statics and a static ssh of the other float dtype cast once, (1, ny, nx); the engine's own buffers hold the
    restatement's bits"""
    from nemoflux_amd._lib import lib, check
    from nemoflux_amd.thickness import SshThickness
    grid = GRIDS[1]
    other = 'float32' if real == 'float64' else 'float64'
    c = _series(other, grid)
    f, g = _build(real, grid), _build(real, grid)
    with numpy.errstate(over='ignore'):
        cast = [a.astype(real) for a in (c['ssh'][0], c['e3u0'], c['e3v0'])]
        want = ref.ssh_thickness(*cast, areas=c['areas'], wrap=False, markers=EM, static_markers=SM)
    f.setCellThickness(SshThickness(c['ssh'][:1], c['e3u0'], c['e3v0'], areas=c['areas'], wrapX=False, **MARKS))
    assert f._e3['nt'] == 1 and not f._cell_thickness_lazy()
    for a, w in zip(f._e3['arrays'], want):
        host = numpy.empty(a.shape, a.dtype)
        check(lib.nf_memcpy_d2h(host.ctypes.data, a.ptr, host.nbytes))
        assert ref.same_bits(host, w)
    g.setCellThickness(_on(want[0], True), _on(want[1], True))
    _same_products(f, g, 1, 'cast')
    for bad, words in ((SshThickness(_on(c['ssh'][0], True), c['e3u0'], c['e3v0']), 'ssh is'),
                       (SshThickness(c['ssh'], c['e3u0'], c['e3v0']), 'ssh is'),
                       (SshThickness(cast[0], _on(c['e3u0'], True), c['e3v0']), 'e3u0 is'),
                       (SshThickness(cast[0], cast[1], cast[2], areas=(_on(c['areas'][0].astype(numpy.float32), True),) + c['areas'][1:]),
                        r'areas\[0\] is')):
        with pytest.raises(RuntimeError, match=words):
            f.setCellThickness(bad)
        assert f._e3 is None


@pytest.mark.parametrize('kind', ['static', 'timevarying'])
@pytest.mark.parametrize('grid', GRIDS, ids=lambda g: f'{g[0]}x{g[1]}')
@pytest.mark.parametrize('real', ['float64', 'float32'])
def test_zero_ssh_over_the_level_vector_is_the_field_without_a_cell_thickness(real, grid, kind):
    """ssh = 0: the factor is 1 and e3u = e3v = the statics, here the level vector at every face (a broadcast cell thickness
    is the scalar form: the anchor of tests/test_gpu_gross.py and tests/test_gpu_depth_remap.py)"""
    from nemoflux_amd.thickness import SshThickness
    nx, ny = grid
    f, g = _build(real, grid), _build(real, grid)
    st = numpy.ascontiguousarray(numpy.broadcast_to(TH.astype(real)[:, None, None], (NZ, ny, nx)))
    ssh = numpy.zeros((NT, ny, nx) if kind == 'timevarying' else (ny, nx), real)
    areas = tuple(numpy.full((ny, nx), a) for a in (3.0, 5.0, 7.0))
    for kw in (dict(e3u0=_on(st, True), e3v0=_on(st, True)), dict(e3t0=st, areas=areas)):
        f.setCellThickness(SshThickness(_on(ssh, True), **kw))
        for t in (1, 0, 2):
            _same_products(f, g, t, (kind, tuple(kw)), ('computeGrossProfile', 'computeGrossProfile-carry', 'computeDepthTransport'))


@pytest.mark.parametrize('real', ['float64', 'float32'])
def test_two_sharded_halves_add_up_as_they_do_with_arrays(real):
    """the column depth is over all levels and the derived buffers are full columns, whatever levels a rank owns"""
    from nemoflux_amd.dist import slab_range
    from nemoflux_amd.thickness import SshThickness
    grid, world = GRIDS[1], 2
    c = _series(real, grid)
    want = _want(real, grid, 'given', True, False, key='series')
    names = ('computeFluxProfile', 'computeGrossProfile-carry', 'computeDepthTransport', 'computeCrossings')

    def make(derived, **kw):
        f = _build(real, grid, True, **kw)
        if derived:
            f.setCellThickness(SshThickness(_on(c['ssh'], True), c['e3u0'], c['e3v0'], areas=c['areas'], **MARKS))
        else:
            f.setCellThickness(_on(want[0], True), _on(want[1], True))
        return f

    full = make(True)
    total = {(nm, t): _flat(PRODUCTS[nm](full, t)) for nm in names for t in range(NT)}
    acc, acc_arr = ({k: [numpy.zeros_like(a) for a in v] for k, v in total.items()} for _ in range(2))
    for rank in range(world):
        sr = slab_range(NT, NZ, rank, world)
        part, arr = make(True, slab_range=sr), make(False, slab_range=sr)
        for (nm, t), sums in acc.items():
            got, same = _flat(PRODUCTS[nm](part, t)), _flat(PRODUCTS[nm](arr, t))
            for k, (a, b) in enumerate(zip(got, same)):
                assert numpy.array_equal(a, b), (rank, nm, t)
                sums[k] += a
                acc_arr[nm, t][k] += b
    for key, sums in acc.items():
        for a, b in zip(sums, acc_arr[key]):
            assert numpy.array_equal(a, b), key
    for key in (('computeFluxProfile', 1), ('computeCrossings', 2)):      # levels belong to one rank: the sum is exact
        for a, b in zip(acc[key], total[key]):
            assert numpy.abs(b).max() > 0 and numpy.array_equal(a, b), key


@pytest.mark.parametrize('home', ['hbm', 'host', 'npz'])
@pytest.mark.parametrize('real', ['float64', 'float32'])
def test_time_means_equal_those_of_the_array_built_field(real, home, tmp_path):
    from nemoflux_amd.thickness import SshThickness
    grid = GRIDS[0]
    resident = home == 'hbm'
    config = 'given' if home == 'host' else 'e3t0-areas'
    f, g = _build(real, grid, resident), _build(real, grid, resident)
    st, want = _descriptor(real, grid, home, config, tmp_path)
    f.setCellThickness(st)
    g.setCellThickness(_on(want[0], resident), _on(want[1], resident))
    with pytest.raises(RuntimeError, match='time-varying cell thickness is not defined here'):
        _quiet(f.timeMean)
    for kw in (dict(), dict(select=[0, 2], weights=[1., 3.])):
        mf, mg = _quiet(f.timeMean, thicknessWeighted=True, **kw), _quiet(g.timeMean, thicknessWeighted=True, **kw)
        assert mf._e3['nt'] == 1
        for a, b in zip(mf._e3['arrays'], mg._e3['arrays']):
            assert numpy.abs(b.cpu().numpy()).max() > 0 and numpy.array_equal(a.cpu().numpy(), b.cpu().numpy())
        _same_products(mf, mg, 0, ('mean state', tuple(kw)), ('computeFlux', 'computeFluxProfile', 'computeTracerFlux',
                                                              'computeGrossProfile-carry'))
        df = _quiet(f.meanEddySplit, 'computeFluxProfile', thicknessWeighted=True, **kw)
        dg = _quiet(g.meanEddySplit, 'computeFluxProfile', thicknessWeighted=True, **kw)
        for part in ('total', 'mean', 'eddy'):
            assert numpy.abs(_rows(dg[part])).max() > 0 and numpy.array_equal(_rows(df[part]), _rows(dg[part])), (kw, part)
    d1, d2 = _quiet(f.meanEddyTracerTransport, thicknessWeighted=True), _quiet(g.meanEddyTracerTransport, thicknessWeighted=True)
    for part in ('total', 'mean', 'eddy'):
        assert numpy.array_equal(d1[part], d2[part]), part
    _same_products(f, g, 1, 'after the means', ('computeFluxProfile',))       # the slot's buffers are staged again
    # a static SshThickness is carried over to the mean state as the static thickness it is
    c = _series(real, grid)
    f.setCellThickness(SshThickness(_on(c['ssh'][1], True), c['e3u0'], c['e3v0'], **MARKS))
    w1 = _want(real, grid, 'given', False, False, ssh=c['ssh'][1])
    g.setCellThickness(_on(w1[0], True), _on(w1[1], True))
    mf, mg = _quiet(f.timeMean), _quiet(g.timeMean)
    _same_products(mf, mg, 0, 'static mean state', ('computeFlux', 'computeFluxProfile', 'computeGrossProfile'))


def test_reuse_of_one_handle_equals_fresh_handles():
    """SshThickness -> plain arrays -> FaceThickness -> None -> an SshThickness with other statics; then another dtype and more
    levels; every result equals a fresh handle's, the resident planes are the same bytes, computeClassTransport refuses
    throughout"""
    from nemoflux_amd.thickness import FaceThickness, SshThickness
    real, grid = 'float32', GRIDS[1]
    c = _series(real, grid)
    w_ssh = _want(real, grid, 'given', False, False, key='series')
    w_other = _want(real, grid, 'e3t0', True, False, key='series')
    arrays = [w + numpy.float32(0.25) for w in w_ssh]
    e3t = fref.series(real, grid, NT, NZ, 'min')[0]
    w_min = fref.want_series(e3t, 'min')
    names = ('computeFluxProfile', 'computeTracerFlux', 'computeGrossProfile-carry', 'computeDepthTransport')

    def fresh(e3):
        x = _build(real, grid)
        if e3 is not None:
            x.setCellThickness(_on(e3[0], True), _on(e3[1], True))
        return x

    f = fresh(None)
    f.computeFlux(0)
    planes = _resident(f)
    fmarks = dict(fill_value=fref.EFILL, missing_value=fref.EMISSING)
    stages = [(lambda: f.setCellThickness(SshThickness(_on(c['ssh'], True), c['e3u0'], c['e3v0'], **MARKS)), w_ssh),
              (lambda: f.setCellThickness(_on(arrays[0], True), _on(arrays[1], True)), arrays),
              (lambda: f.setCellThickness(FaceThickness(_on(e3t, True), 'min', **fmarks)), w_min),
              (lambda: f.setCellThickness(None, None), None),
              (lambda: f.setCellThickness(SshThickness(c['ssh'], e3t0=c['e3t0'], areas=c['areas'], **MARKS)), w_other)]
    seen = []
    for k, (change, e3) in enumerate(stages):
        change()
        x = fresh(e3)
        for t in (2, 1):
            _same_products(f, x, t, ('stage', k), names)
        seen.append(_rows(f.computeFluxProfile(1)))
        if e3 is not None:
            with pytest.raises(RuntimeError) as err:
                f.computeClassTransport(0)
            with pytest.raises(RuntimeError) as err_x:
                x.computeClassTransport(0)
            assert str(err.value) == str(err_x.value)
    assert not any(numpy.array_equal(seen[i], seen[j]) for i in range(5) for j in range(i))
    f.computeFlux(0)
    x = fresh(w_other)
    x.computeFlux(0)
    for a, b in zip(_resident(f), _resident(x)):
        assert numpy.array_equal(a, b)
    f.setCellThickness(None, None)
    f.computeFlux(0)
    for a, b in zip(_resident(f), planes):
        assert numpy.array_equal(a, b)
    # another dtype and more levels: a new Field of float64 with twice the levels
    from conftest import transect_xyz
    blon, blat = _case('float64', grid)[:2]
    u, v = _uv('float64', grid)
    u2, v2 = numpy.concatenate([u, u[:, ::-1]], axis=1), numpy.concatenate([v, v[:, ::-1]], axis=1)
    th2 = numpy.concatenate([TH, TH])
    db2 = numpy.stack([numpy.concatenate([[0.], numpy.cumsum(th2)[:-1]]), numpy.cumsum(th2)], axis=1)
    c2 = ref.series('float64', grid, NT, 2 * NZ, seed=50)
    w2 = ref.ssh_thickness(c2['ssh'], c2['e3u0'], c2['e3v0'], areas=c2['areas'], markers=EM, static_markers=SM)

    def big():
        return _field(blon, blat, db2, _on(u2, True), _on(v2, True), [transect_xyz(s) for s in (T_OPEN, T_SEAM)], readback=False,
                      fill_value=FILL, missing_value=MISSING)

    a, b = big(), big()
    a.setCellThickness(SshThickness(_on(c2['ssh'], True), _on(c2['e3u0'], True), _on(c2['e3v0'], True), areas=c2['areas'], **MARKS))
    b.setCellThickness(_on(w2[0], True), _on(w2[1], True))
    for t in STEPS:
        _same_products(a, b, t, 'float64, 14 levels', ('computeFlux', 'computeFluxProfile', 'computeGrossProfile'))


def test_compute_class_transport_still_refuses():
    from nemoflux_amd.thickness import SshThickness
    real, grid = 'float64', GRIDS[0]
    c = _series(real, grid)
    f, g = _build(real, grid), _build(real, grid)
    f.setCellThickness(SshThickness(_on(c['ssh'], True), c['e3u0'], c['e3v0'], **MARKS))
    w = _want(real, grid, 'given', False, False, key='series')
    g.setCellThickness(_on(w[0], True), _on(w[1], True))
    for name in ('computeClassTransport', 'computeTracerProfile', 'computeClassTracerTransport'):
        with pytest.raises(RuntimeError) as e1:
            getattr(f, name)(0)
        with pytest.raises(RuntimeError) as e2:
            getattr(g, name)(0)
        assert str(e1.value) == str(e2.value) and 'cell thickness' in str(e1.value).lower().replace('-', ' '), name


# ---- the command line ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('form', ['npz', 'npz-areas', 'classic'])
def test_fluxplot_ssh_writes_the_rows_of_the_array_built_field(tmp_path, form):
    from nemoflux_amd import fluxplot
    real, grid = 'float32', GRIDS[0]
    blon, blat = _case(real, grid)[:2]
    u, v = _uv(real, grid)
    c = _series(real, grid)
    paths = {k: str(tmp_path / f'{k}.npz') for k in 'TUVM'}
    fv = lambda name, m: {f'_FillValue_{name}': numpy.array(m[0]), f'_missing_value_{name}': numpy.array(m[1])}   # noqa: E731
    numpy.savez(paths['T'], bounds_lon=blon, bounds_lat=blat, deptht_bounds=DB, zos=c['ssh'], **fv('zos', EM))
    numpy.savez(paths['U'], uo=u, **fv('uo', (FILL, MISSING)))
    numpy.savez(paths['V'], vo=v, **fv('vo', (FILL, MISSING)))
    numpy.savez(paths['M'], e3u_0=c['e3u0'], e3v_0=c['e3v0'], thku=c['e3v0'], thkv=c['e3u0'], e1e2t=c['areas'][0],
                e1e2u=c['areas'][1], e1e2v=c['areas'][2],
                **{k: x for n in ('e3u_0', 'e3v_0', 'thku', 'thkv') for k, x in fv(n, SM).items()})
    kw, markers, statics, areas = dict(ssh='zos', e3Static=paths['M']), EM, (c['e3u0'], c['e3v0']), None
    if form == 'npz-areas':
        kw.update(e3Static=paths['M'] + ':thku,thkv', e3Areas='e1e2t,e1e2u,e1e2v')
        statics, areas = (c['e3v0'], c['e3u0']), c['areas']
    if form == 'classic':
        kw.update(sshFile=_classic_ssh(tmp_path / 'ssh.nc', c['ssh']))
        markers = (EM[0],)
    lines = '[' + T_OPEN + '],[' + T_SEAM + ']'
    out = str(tmp_path / 'levels.csv')
    totals = _quiet(fluxplot.main, tFile=paths['T'], uFile=paths['U'], vFile=paths['V'], lonLatPoints=lines, output=out,
                    sverdrup=True, levels=True, cellThickness=True, **kw)
    want = ref.ssh_thickness(c['ssh'], *statics, areas=areas, markers=markers, static_markers=SM)
    mem = _field(blon, blat, DB, u, v, fluxplot.readTargets(lines)[0], True, fill_value=FILL, missing_value=MISSING, readback=False)
    mem.setCellThickness(want[0], want[1])
    assert totals.shape[0] == NT
    for t in range(NT):
        rows = mem.computeFluxProfile(t)[0]
        assert numpy.abs(rows).max() > 0 and numpy.array_equal(numpy.asarray(totals[t]).reshape(rows.shape), rows), t
    with pytest.raises(RuntimeError, match='cannot be combined with --e3t'):
        _quiet(fluxplot.main, tFile=paths['T'], uFile=paths['U'], vFile=paths['V'], lonLatPoints=lines, levels=True,
               cellThickness=True, ssh='zos', e3Static=paths['M'], e3t='thk')


@pytest.mark.parametrize('kind', ['static', 'timevarying'])
def test_packed_file_variables_through_field(tmp_path, kind):
    """ssh, the statics and the column depths stored as int16 with a scale_factor in an .npz bundle: decoded once, masked values
    NaN; a FaceThickness takes packed (nz, ny, nx) statics as it did before the slot code was shared"""
    from nemoflux_amd.thickness import FaceThickness, SshThickness
    from test_ssh_thickness_cpu import _packed_bundle
    real, grid = 'float32', GRIDS[0]
    path, dec = _packed_bundle(tmp_path, _series(real, grid), kind == 'static')
    f, g = _build(real, grid), _build(real, grid)
    f.setCellThickness(SshThickness((path, 'zos'), (path, 'e3u_0'), (path, 'e3v_0'), hu0=(path, 'hu_0'), hv0=(path, 'hu_0')))
    want = ref.ssh_thickness(dec['zos'], dec['e3u_0'], dec['e3v_0'], dec['hu_0'], dec['hu_0'])
    assert (want[0] != numpy.where(numpy.isnan(dec['e3u_0']), 0, dec['e3u_0'])).mean() > 0.1
    g.setCellThickness(_on(want[0], True), _on(want[1], True))
    assert f._e3['nt'] == (1 if kind == 'static' else NT)
    for t in ((1,) if kind == 'static' else STEPS):
        _same_products(f, g, t, ('packed', kind), ('computeFlux', 'computeFluxProfile', 'computeGrossProfile'))
    e3t = fref.series(real, grid, NT, NZ, 'min')[0]
    e3t = e3t[1] if kind == 'static' else e3t
    f.setCellThickness(FaceThickness(e3t, 'anomaly', (path, 'e3u_0'), (path, 'e3v_0'), (path, 'e3u_0'), fill_value=fref.EFILL,
                                     missing_value=fref.EMISSING))
    want = fref.face_thickness(e3t, 'anomaly', dec['e3u_0'], dec['e3v_0'], dec['e3u_0'], markers=(fref.EFILL, fref.EMISSING))
    g.setCellThickness(_on(want[0], True), _on(want[1], True))
    for t in ((1,) if kind == 'static' else STEPS):
        _same_products(f, g, t, ('packed statics of a FaceThickness', kind), ('computeFlux', 'computeFluxProfile'))
