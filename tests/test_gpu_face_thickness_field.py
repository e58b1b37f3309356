"""Face thicknesses derived from e3t through Field: a Field with setCellThickness(FaceThickness(...)) against a fresh Field whose
e3u / e3v are the series of tests/face_thickness_reference.py given as arrays -- every product that takes a cell thickness
array_equal, both dtypes, e3t in HBM, on the host, in an .npz bundle and in a classic NetCDF-3 file, static and time-varying,
the three rules, the steps visited 2, 0, 2, 1; the level vector broadcast as e3t against the Field without a cell thickness; two
sharded halves; timeMean(thicknessWeighted=True) and meanEddySplit; re-use of one handle; the refusal of computeClassTransport;
fluxplot --cell-thickness --e3t; a grid of 1030 x 6 (float32: 1028 x 6), past one column chunk of the kernel.

Grids 72 x 36 x 7 x 3 and 73 x 37 x 7 x 3 with the three transects of tests/test_gpu_depth_remap.py (one across the seam)."""
import numpy
import pytest

from conftest import write_classic_triple
from depth_remap_reference import EDGES
from gpu_helpers import _field, _on, _quiet, _resident, _rows
import face_thickness_reference as ref
from test_gpu_cellthick import FILL, MISSING, T_OPEN, T_SEAM, _case
from test_gpu_depth_remap import DB, LINES, TH, _make, _set_tracer
from test_gpu_gross import GRIDS, NT, NZ, _tau, _uv

pytestmark = pytest.mark.gpu

STEPS = (2, 0, 2, 1)
RULES = ('min', 'mean', 'anomaly')
CLASS_EDGES = numpy.array([2.5, 4.5, 6.5])
EM, SM = (ref.EFILL, ref.EMISSING), (ref.SFILL, ref.SMISSING)
MARKS = dict(fill_value=EM[0], missing_value=EM[1], static_fill_value=SM[0], static_missing_value=SM[1])
_SERIES = {}


def _series(real, grid, rule):
    """(e3t (NT, NZ, ny, nx), [e3t0, e3u0, e3v0] or [None] * 3), computed once"""
    if (real, grid, rule) not in _SERIES:
        e3t, *statics = ref.series(real, grid, NT, NZ, rule)
        _SERIES[real, grid, rule] = (e3t, statics)
    return _SERIES[real, grid, rule]


def _surfaces(real, grid):
    nx, ny = grid
    rng = numpy.random.default_rng(17)
    return [(base + rng.integers(-16, 17, (NT, ny, nx)) / 8.).astype(real) for base in (5.0, 11.0)]


def _build(real, grid, resident=True, **kw):
    """a Field with everything the products need but the cell thickness"""
    f = _make(real, grid, resident, sverdrup=True, **kw)
    _set_tracer(f, _tau(real, grid), resident)
    f.setClassEdges(CLASS_EDGES)
    f.setDepthEdges(EDGES[3], -1.5)
    f.setDepthSurfaces([_on(s, resident) for s in _surfaces(real, grid)], top=-1.5)
    return f


def _flat(x):
    """every array of a product's result, in order"""
    if isinstance(x, (tuple, list)):
        return [a for y in x for a in _flat(y)]
    return [numpy.asarray(x, dtype=numpy.float64)]


PRODUCTS = {
    'computeFlux': lambda f, t: f.computeFlux(t),
    'computeFluxProfile': lambda f, t: f.computeFluxProfile(t),
    'computeTracerFlux': lambda f, t: f.computeTracerFlux(t),
    'computeAreaProfile': lambda f, t: f.computeAreaProfile(t),
    'computeGrossProfile': lambda f, t: f.computeGrossProfile(t),
    'computeGrossProfile-carry': lambda f, t: f.computeGrossProfile(t, carry=True),
    'computeDepthTransport': lambda f, t: (f.computeDepthTransport(t), f.computeDepthTransport(t, carry=True)),
    'computeSurfaceTransport': lambda f, t: (f.computeSurfaceTransport(t), f.computeSurfaceTransport(t, carry=True)),
    'computeGrossClassTransport': lambda f, t: f.computeGrossClassTransport(t),
    'computeGrossClassRemap': lambda f, t: f.computeGrossClassRemap(t),
    'computeClassArea': lambda f, t: f.computeClassArea(t),
    'computeCrossings': lambda f, t: (f.computeCrossings(t), f.computeCrossings(t, carry=True)),
}


def _same_products(f, g, t, label, names=PRODUCTS):
    for name in names:
        got, want = _flat(PRODUCTS[name](f, t)), _flat(PRODUCTS[name](g, t))
        assert len(got) == len(want) and max(numpy.abs(w).max() for w in want) > 0, (label, name)
        for a, b in zip(got, want):
            assert numpy.array_equal(a, b), (label, name, t)


def _homes(real, grid, home, rule, e3t, statics, tmp_path):
    """(FaceThickness arguments as the home holds them, (e3t, statics, e3t markers, static markers) for the restatement)"""
    from nemoflux_amd.thickness import FaceThickness
    if home in ('hbm', 'host'):
        ft = FaceThickness(_on(e3t, home == 'hbm'), rule, *[None if s is None else _on(s, home == 'hbm') for s in statics],
                           **MARKS)
        return ft, (e3t, statics, EM, SM)
    if home == 'npz':                 # the markers come from the file
        path = str(tmp_path / f'TE_{rule}_{e3t.ndim}.npz')
        fv = lambda name, m: {f'_FillValue_{name}': numpy.array(m[0]), f'_missing_value_{name}': numpy.array(m[1])}   # noqa: E731
        more = {}
        if rule == 'anomaly':
            for name, s in zip(('e3t_0', 'e3u_0', 'e3v_0'), statics):
                more.update({name: s}, **fv(name, SM))
        numpy.savez(path, e3t=e3t, **fv('e3t', EM), **more)
        pairs = [(path, n) for n in ('e3t_0', 'e3u_0', 'e3v_0')] if rule == 'anomaly' else []
        return FaceThickness((path, 'e3t'), rule, *pairs), (e3t, statics, EM, SM)
    # a classic NetCDF-3 record variable, float32, read one step at a time: e3t travels as the U file's variable (one marker,
    # its _FillValue; the other marker's value is data), the writer adds its own land block; the statics are host arrays
    assert real == 'float32' and e3t.ndim == 4
    blon, blat = _case(real, grid)[:2]
    paths, ef, _ = write_classic_triple(tmp_path, dict(u=e3t, v=numpy.ones_like(e3t), bounds_lon=blon, bounds_lat=blat,
                                                       deptht_bounds=DB))
    ft = FaceThickness((paths['U'], 'uo'), rule, *statics, static_fill_value=SM[0], static_missing_value=SM[1])
    return ft, (ef, statics, (1.e20,), SM)


CASES = [(real, grid, home) for real in ('float64', 'float32') for grid in GRIDS for home in ('hbm', 'host', 'npz')]
CASES += [('float32', grid, 'classic') for grid in GRIDS]


@pytest.mark.parametrize('real,grid,home', CASES, ids=[f'{r}-{g[0]}x{g[1]}-{h}' for r, g, h in CASES])
def test_field_with_a_face_thickness_gives_the_products_of_the_restatements_series(real, grid, home, tmp_path):
    """the three rules time-varying, the steps visited 2, 0, 2, 1, computeAll over all of them; one of the rules static too"""
    resident = home == 'hbm'
    n = CASES.index((real, grid, home))
    f, g = _build(real, grid, resident), _build(real, grid, resident)
    for k, rule in enumerate(RULES):
        e3t, statics = _series(real, grid, rule)
        kinds = ['timevarying'] + (['static'] if k == n % 3 and home != 'classic' else [])
        for kind in kinds:
            src = e3t if kind == 'timevarying' else e3t[1]
            ft, (e3t_r, st_r, em, sm) = _homes(real, grid, home, rule, src, statics, tmp_path)
            want = ref.face_thickness(e3t_r, rule, *st_r, wrap=True, markers=em, static_markers=sm)
            assert want[0].dtype == numpy.dtype(real) and (want[0] == 0).mean() > 0.05 and len(numpy.unique(want[0])) > 20
            f.setCellThickness(ft)
            g.setCellThickness(_on(want[0], resident), _on(want[1], resident))
            assert f._cell_thickness_lazy() == (kind == 'timevarying') and f._e3['nt'] == (NT if kind == 'timevarying' else 1)
            for t in (STEPS if kind == 'timevarying' else (1,)):
                _same_products(f, g, t, (rule, kind))
            for a, b in zip(f.computeAll(), g.computeAll()):
                assert numpy.abs(b).max() > 0 and numpy.array_equal(a, b), (rule, kind)
            for a, b in zip(f.computeTracerAll(), g.computeTracerAll()):
                assert numpy.abs(b).max() > 0 and numpy.array_equal(a, b), (rule, kind)


# a grid past one column chunk of nf_face_thickness / nf_ssh_thickness: three chunks of 16-byte lanes at float64 (512 + 512 + 6),
# two at float32, the last of one lane (1024 + 4)
WIDE_GRID = {'float64': (1030, 6), 'float32': (1028, 6)}


def _seam_rows(f):
    """T_SEAM's totals of every step, level by level"""
    return numpy.stack([numpy.asarray(f.computeFluxProfile(t)[0])[..., LINES.index(T_SEAM)] for t in range(NT)])


@pytest.mark.parametrize('real', ['float64', 'float32'])
def test_a_wide_short_grid_past_one_column_chunk(real):
    """time-varying e3t in HBM under the anomaly rule on 1030 x 6 and 1028 x 6; T_SEAM runs through the last column, whose
    east faces take column 0 from another chunk: with the restatement's wrapX off its rows are other rows"""
    from nemoflux_amd.thickness import FaceThickness
    grid = WIDE_GRID[real]
    e3t, statics = _series(real, grid, 'anomaly')
    want = ref.want_series(e3t, 'anomaly', statics)
    f, g = _build(real, grid), _build(real, grid)
    f.setCellThickness(FaceThickness(_on(e3t, True), 'anomaly', *[_on(s, True) for s in statics], **MARKS))
    g.setCellThickness(_on(want[0], True), _on(want[1], True))
    assert f._cell_thickness_lazy() and f._e3['nt'] == NT
    for t in STEPS:
        _same_products(f, g, t, ('wide', real))
    off = ref.want_series(e3t, 'anomaly', statics, wrap=False)
    assert ref.same_bits(off[0][..., :-1], want[0][..., :-1]) and ref.same_bits(off[1], want[1])
    rows = _seam_rows(g)
    assert numpy.array_equal(_seam_rows(f), rows) and numpy.abs(rows).max() > 0
    g.setCellThickness(_on(off[0], True), _on(off[1], True))
    assert not numpy.array_equal(_seam_rows(g), rows)


@pytest.mark.parametrize('real', ['float64', 'float32'])
def test_wrap_off_and_a_static_host_array_of_another_dtype(real):
    from nemoflux_amd.thickness import FaceThickness
    grid = GRIDS[1]
    other = 'float32' if real == 'float64' else 'float64'
    e3t, statics = _series(other, grid, 'anomaly')
    f, g = _build(real, grid), _build(real, grid)
    cast = [a.astype(real) for a in [e3t[0]] + statics]
    with numpy.errstate(over='ignore'):
        want = ref.face_thickness(cast[0], 'anomaly', *cast[1:], wrap=False, markers=EM, static_markers=SM)
    f.setCellThickness(FaceThickness(e3t[0], 'anomaly', *statics, wrapX=False, **MARKS))
    g.setCellThickness(_on(want[0], True), _on(want[1], True))
    _same_products(f, g, 1, 'cast')
    for bad, words in ((FaceThickness(_on(e3t[0], True)), 'e3t is'), (FaceThickness(e3t), 'e3t is'),
                       (FaceThickness(cast[0], 'anomaly', _on(statics[0], True), *cast[2:]), 'e3t0 is')):
        with pytest.raises(RuntimeError, match=words):
            f.setCellThickness(bad)
        assert f._e3 is None


@pytest.mark.parametrize('kind', ['static', 'timevarying'])
@pytest.mark.parametrize('grid', GRIDS, ids=lambda g: f'{g[0]}x{g[1]}')
@pytest.mark.parametrize('real', ['float64', 'float32'])
def test_the_level_vector_broadcast_as_e3t_is_the_field_without_a_cell_thickness(real, grid, kind):
    """min and mean of equal cells are the cell: e3u = e3v = the level vector at every face, the anchor of
    tests/test_gpu_gross.py and tests/test_gpu_depth_remap.py (a broadcast cell thickness is the scalar form)"""
    from nemoflux_amd.thickness import FaceThickness
    nx, ny = grid
    f, g = _build(real, grid), _build(real, grid)
    shape = (NT, NZ, ny, nx) if kind == 'timevarying' else (NZ, ny, nx)
    e3t = numpy.ascontiguousarray(numpy.broadcast_to(TH.astype(real)[:, None, None], shape))
    for rule in ('min', 'mean'):
        f.setCellThickness(FaceThickness(_on(e3t, True), rule))
        for t in (1, 0, 2):
            _same_products(f, g, t, (rule, kind), ('computeGrossProfile', 'computeGrossProfile-carry', 'computeDepthTransport'))


@pytest.mark.parametrize('real', ['float64', 'float32'])
def test_two_sharded_halves_add_up_as_they_do_with_arrays(real):
    from nemoflux_amd.dist import slab_range
    from nemoflux_amd.thickness import FaceThickness
    grid, world = GRIDS[1], 2
    e3t, statics = _series(real, grid, 'anomaly')
    want = ref.want_series(e3t, 'anomaly', statics)
    names = ('computeFluxProfile', 'computeGrossProfile-carry', 'computeDepthTransport', 'computeCrossings')

    def make(derived, **kw):
        f = _build(real, grid, True, **kw)
        if derived:
            f.setCellThickness(FaceThickness(_on(e3t, True), 'anomaly', *statics, **MARKS))
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
    grid = GRIDS[0]
    resident = home == 'hbm'
    rule = 'mean' if home == 'host' else 'anomaly'
    e3t, statics = _series(real, grid, rule)
    f, g = _build(real, grid, resident), _build(real, grid, resident)
    ft, (e3t_r, st_r, em, sm) = _homes(real, grid, home, rule, e3t, statics, tmp_path)
    want = ref.face_thickness(e3t_r, rule, *st_r, markers=em, static_markers=sm)
    f.setCellThickness(ft)
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
    # a static FaceThickness is carried over to the mean state as the static thickness it is
    from nemoflux_amd.thickness import FaceThickness
    f.setCellThickness(FaceThickness(_on(e3t[1], True), rule, *statics, **MARKS))
    w1 = ref.want_series(e3t[1], rule, statics)
    g.setCellThickness(_on(w1[0], True), _on(w1[1], True))
    mf, mg = _quiet(f.timeMean), _quiet(g.timeMean)
    _same_products(mf, mg, 0, 'static mean state', ('computeFlux', 'computeFluxProfile', 'computeGrossProfile'))
    mf, mg = _quiet(f.timeMean, thicknessWeighted=True), _quiet(g.timeMean, thicknessWeighted=True)
    _same_products(mf, mg, 0, 'static weighted mean state', ('computeFluxProfile',))


def test_reuse_of_one_handle_equals_fresh_handles():
    """arrays -> FaceThickness('min') -> None -> FaceThickness('anomaly'), then another dtype and more levels; every result
    equals a fresh handle's, the resident planes are the same bytes, computeClassTransport refuses throughout"""
    from nemoflux_amd.thickness import FaceThickness
    real, grid = 'float32', GRIDS[1]
    e3t, _ = _series(real, grid, 'min')
    e3t_a, statics = _series(real, grid, 'anomaly')
    w_min, w_an = ref.want_series(e3t, 'min'), ref.want_series(e3t_a, 'anomaly', statics)
    arrays = [w + numpy.float32(0.25) for w in w_min]
    names = ('computeFluxProfile', 'computeTracerFlux', 'computeGrossProfile-carry', 'computeDepthTransport')

    def fresh(e3):
        x = _build(real, grid)
        if e3 is not None:
            x.setCellThickness(_on(e3[0], True), _on(e3[1], True))
        return x

    f = fresh(None)
    f.computeFlux(0)
    planes = _resident(f)
    stages = [(lambda: f.setCellThickness(_on(arrays[0], True), _on(arrays[1], True)), arrays),
              (lambda: f.setCellThickness(FaceThickness(_on(e3t, True), 'min', **MARKS)), w_min),
              (lambda: f.setCellThickness(None, None), None),
              (lambda: f.setCellThickness(FaceThickness(e3t_a, 'anomaly', *statics, **MARKS)), w_an)]
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
    assert not any(numpy.array_equal(seen[i], seen[j]) for i in range(4) for j in range(i))
    f.computeFlux(0)
    x = fresh(w_an)
    x.computeFlux(0)
    for a, b in zip(_resident(f), _resident(x)):
        assert numpy.array_equal(a, b)
    f.setCellThickness(None, None)
    f.computeFlux(0)
    for a, b in zip(_resident(f), planes):
        assert numpy.array_equal(a, b)
    # another dtype and more levels on the raw engine's side: a new Field of float64 with twice the levels
    from conftest import transect_xyz
    blon, blat = _case('float64', grid)[:2]
    u, v = _uv('float64', grid)
    u2, v2 = numpy.concatenate([u, u[:, ::-1]], axis=1), numpy.concatenate([v, v[:, ::-1]], axis=1)
    th2 = numpy.concatenate([TH, TH])
    db2 = numpy.stack([numpy.concatenate([[0.], numpy.cumsum(th2)[:-1]]), numpy.cumsum(th2)], axis=1)
    e2 = numpy.stack([ref.make_case('float64', 2 * NZ, grid[1], grid[0], 'mean', seed=900 + t)[0] for t in range(NT)])
    w2 = ref.face_thickness(e2, 'mean', markers=EM)

    def big():
        return _field(blon, blat, db2, _on(u2, True), _on(v2, True), [transect_xyz(s) for s in (T_OPEN, T_SEAM)], readback=False,
                      fill_value=FILL, missing_value=MISSING)

    a, b = big(), big()
    a.setCellThickness(FaceThickness(_on(e2, True), 'mean', fill_value=EM[0], missing_value=EM[1]))
    b.setCellThickness(_on(w2[0], True), _on(w2[1], True))
    for t in STEPS:
        _same_products(a, b, t, 'float64, 14 levels', ('computeFlux', 'computeFluxProfile', 'computeGrossProfile'))


def test_compute_class_transport_still_refuses():
    from nemoflux_amd.thickness import FaceThickness
    real, grid = 'float64', GRIDS[0]
    e3t, _ = _series(real, grid, 'min')
    f, g = _build(real, grid), _build(real, grid)
    f.setCellThickness(FaceThickness(_on(e3t, True), **MARKS))
    w = ref.want_series(e3t, 'min')
    g.setCellThickness(_on(w[0], True), _on(w[1], True))
    for name in ('computeClassTransport', 'computeTracerProfile', 'computeClassTracerTransport'):
        with pytest.raises(RuntimeError) as e1:
            getattr(f, name)(0)
        with pytest.raises(RuntimeError) as e2:
            getattr(g, name)(0)
        assert str(e1.value) == str(e2.value) and 'cell thickness' in str(e1.value).lower().replace('-', ' '), name


# ---- the command line ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('rule', ['min', 'anomaly'])
def test_fluxplot_e3t_writes_the_rows_of_the_array_built_field(tmp_path, rule):
    from nemoflux_amd import fluxplot
    real, grid = 'float32', GRIDS[0]
    blon, blat = _case(real, grid)[:2]
    u, v = _uv(real, grid)
    e3t, statics = _series(real, grid, rule)
    paths = {k: str(tmp_path / f'{k}.npz') for k in 'TUVM'}
    fv = lambda name, m: {f'_FillValue_{name}': numpy.array(m[0]), f'_missing_value_{name}': numpy.array(m[1])}   # noqa: E731
    numpy.savez(paths['T'], bounds_lon=blon, bounds_lat=blat, deptht_bounds=DB, thk=e3t, **fv('thk', EM))
    numpy.savez(paths['U'], uo=u, **fv('uo', (FILL, MISSING)))
    numpy.savez(paths['V'], vo=v, **fv('vo', (FILL, MISSING)))
    kw = dict(e3t='thk')
    if rule == 'anomaly':
        numpy.savez(paths['M'], **{n: s for n, s in zip(('e3t_0', 'e3u_0', 'e3v_0'), statics)},
                    **{k: x for n in ('e3t_0', 'e3u_0', 'e3v_0') for k, x in fv(n, SM).items()})
        kw.update(e3Rule='anomaly', e3Static=paths['M'])
    lines = '[' + T_OPEN + '],[' + T_SEAM + ']'
    out = str(tmp_path / 'levels.csv')
    totals = _quiet(fluxplot.main, tFile=paths['T'], uFile=paths['U'], vFile=paths['V'], lonLatPoints=lines, output=out,
                    sverdrup=True, levels=True, cellThickness=True, **kw)
    want = ref.want_series(e3t, rule, statics)
    mem = _field(blon, blat, DB, u, v, fluxplot.readTargets(lines)[0], True, fill_value=FILL, missing_value=MISSING, readback=False)
    mem.setCellThickness(want[0], want[1])
    assert totals.shape[0] == NT
    for t in range(NT):
        rows = mem.computeFluxProfile(t)[0]
        assert numpy.abs(rows).max() > 0 and numpy.array_equal(numpy.asarray(totals[t]).reshape(rows.shape), rows), t
    with pytest.raises(RuntimeError, match='cannot be combined with --e3u'):
        _quiet(fluxplot.main, tFile=paths['T'], uFile=paths['U'], vFile=paths['V'], lonLatPoints=lines, levels=True,
               cellThickness=True, e3t='thk', e3u='e3u')
