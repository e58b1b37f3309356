"""Transports between surfaces on the GPU (Field.computeSurfaceTransport, nf_field_compute_surface_transport, fluxplot
--depth-surfaces).  Every value of every row in all four forms -- volume or carried tracer, scalar or per-cell thickness -- is
checked against the float64 / long-double restatement of the definition in tests/surface_transport_reference.py to
1e-12 x sum |share| of that value (the A7 bar of docs/PARITY.md), no row or column left out, for m = 1, 2, 3, 8 surfaces, both
dtypes, HBM and host, static and time-varying surfaces, the three thickness forms, wrapX and Sverdrup on and off, `top` 0 and
-1.5; anchored bit for bit to computeDepthTransport (surfaces constant over the grid, m = 1 against the edges [e, 1e300],
surfaces constant on three blocks of columns), to itself (negated / doubled uo, vo; tau = ref + 1; a broadcast cell thickness;
every class_window, out=, host inputs; a static set given as nt copies); the sum over the rows against the profile rows and the
tracer row; two sharded halves; meanEddySplit; fluxplot --depth-surfaces from files.

Grids 72 x 36 x 7 x 3 and 73 x 37 x 7 x 3 with the three transects of tests/test_gpu_depth_remap.py (one across the periodic
seam; two blocks of records).  The surfaces are those of surface_transport_reference.surface_fields (seed 91): multiples of 1/8
with both markers, NaN and +inf scattered; tests/test_surface_transport_cpu.py checks without a GPU that with these inputs
terms are spread over several rows, terms have lo == hi, interface depths lie exactly on an edge, the running max acts and at
most a quarter of the faces go to the last row.

Measured on an MI355X: see the figures printed by each test; docs/PARITY.md quotes the worst."""
import ctypes

import numpy
import pytest

from gpu_helpers import _field, _knob, _on, _quiet, _rows, _same_bits
from gross_reference import array_values
from surface_transport_reference import GPU_M, SFILL, SMISSING, SurfaceReference, gpu_case, surface_fields, surface_values
from test_gpu_cellthick import BAR, FILL, MISSING, T_OPEN, T_SEAM, TFILL, THFILL, THMISSING, TMISSING, _case
from test_gpu_depth_remap import DB, THICK, _broadcast, _check, _close, _make, _set_thickness, _set_tracer
from test_gpu_gross import GRIDS, NT, NZ, REF, _tau, _uv

pytestmark = pytest.mark.gpu

dp = ctypes.POINTER(ctypes.c_double)
_S = {}
WORST = {'reference': 0.0}


def _surf(real, grid, m, nt_s):
    if (real, grid, m, nt_s) not in _S:
        _S[real, grid, m, nt_s] = surface_fields(real, (nt_s, grid[1], grid[0]), m)
    return _S[real, grid, m, nt_s]


def _set_surfaces(f, s, resident, top=0.0, wrap=True):
    """s: (nt_s, m, ny, nx); the Field gets one array per surface, (ny, nx) for a static set"""
    items = [numpy.ascontiguousarray(s[0, k] if s.shape[0] == 1 else s[:, k]) for k in range(s.shape[1])]
    f.setDepthSurfaces([_on(a, resident) for a in items], top=top, fill_value=SFILL, missing_value=SMISSING, wrapX=wrap)


def _const(real, grid, levels, nt_s=1):
    """surfaces constant over the grid at `levels`"""
    nx, ny = grid
    return numpy.ascontiguousarray(numpy.broadcast_to(numpy.asarray(levels, dtype=real)[None, :, None, None],
                                                      (nt_s, len(levels), ny, nx)))


def _st(f, t, carry=False, **kw):
    """(m + 2, row_length): [segments | transects] rows"""
    return _rows(f.computeSurfaceTransport(t, carry=carry, **kw))


def _dt(f, t, carry=False, **kw):
    return _rows(f.computeDepthTransport(t, carry=carry, **kw))


def _reference(f, wrap=True, swrap=True, ref=REF, sverdrup=False, cell_thickness=False, uv_markers=(FILL, MISSING)):
    ce, w, sg = f.getWeights()
    return SurfaceReference(ce, w, sg, f.arcLengths, f.thickness, f._tr_off, f.nx, f.ny, uv_markers=uv_markers,
                            tracer_markers=(TFILL, TMISSING), thick_markers=(THFILL, THMISSING), reference=ref, wrap=wrap,
                            sverdrup=sverdrup, cell_thickness=cell_thickness, surface_markers=(SFILL, SMISSING),
                            surface_wrap=swrap)


# ---- against the reference -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('thick', THICK)
@pytest.mark.parametrize('wrap', [True, False], ids=['wrap-sv', 'nowrap-m2'])
@pytest.mark.parametrize('resident', [True, False], ids=['hbm', 'host'])
@pytest.mark.parametrize('grid', GRIDS, ids=lambda g: f'{g[0]}x{g[1]}')
@pytest.mark.parametrize('real', ['float64', 'float32'])
def test_against_the_reference(real, grid, resident, wrap, thick):
    """volume and carried forms; every m, each on one of the steps and with one of the tops (gpu_case); `wrap`: the wrapX of
    the tracer and of the surfaces, and Sverdrup"""
    u, v = _uv(real, grid)
    tau = _tau(real, grid)
    f = _make(real, grid, resident, sverdrup=wrap)
    ce = f.getWeights()[0]
    assert ce.size > 256 and (ce // 4 % f.nx == f.nx - 1).any()        # two blocks; the seam: east faces of the last column
    arrays = {'uo': u, 'vo': v, 'tracer': tau}
    arrays.update(_set_thickness(f, real, grid, resident, thick))
    _set_tracer(f, tau, resident, wrap=wrap)
    r = _reference(f, wrap=wrap, swrap=wrap, sverdrup=wrap, cell_thickness=thick != 'scalar')
    for k in range(len(GPU_M)):
        m, t, top, nt_s = gpu_case(k, THICK.index(thick), NT)
        s = _surf(real, grid, m, nt_s)
        dt = s.dtype.type
        assert numpy.isnan(s).any() and (s == dt(SFILL)).any() and (s == dt(SMISSING)).any() and numpy.isinf(s).any()
        arrays['surface'] = s
        _set_surfaces(f, s, resident, top=top, wrap=wrap)
        want = r.surface_step(surface_values(arrays, t), m, top=top)
        vol, car = _st(f, t), _st(f, t, carry=True)
        assert vol.shape == car.shape == (m + 2, f._rowlen)
        label = f'{thick} m={m} t={t} top={top} nt_s={nt_s}'
        for got, nm in ((vol, 'volume'), (car, 'carried')):
            WORST['reference'] = max(WORST['reference'], _close(got, *want[nm], f'{nm} {label}'))
        assert want['spread_terms'] > 0 and want['on_edge'] > 0 and 0 < 4 * want['unbinned'] <= want['faces']
        assert (want['volume'][1].max(axis=1) > 0).all(), label              # every row, the last one too, holds terms
    print(f'worst so far against the reference: {WORST["reference"]:.3g}')


# ---- bit for bit -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('thick', THICK)
@pytest.mark.parametrize('grid', GRIDS, ids=lambda g: f'{g[0]}x{g[1]}')
@pytest.mark.parametrize('real', ['float64', 'float32'])
def test_constant_surfaces_give_the_rows_of_the_depth_bins(real, grid, thick):
    """surfaces constant over the grid at e_1 < ... < e_m: every face has the edges e, so the rows are those of
    computeDepthTransport with these edges in all four forms; m = 1 at e: rows 0, 1 and the last row of the edges [e, 1e300]"""
    resident = grid == GRIDS[0]
    f = _make(real, grid, resident, sverdrup=True)
    _set_thickness(f, real, grid, resident, thick)
    _set_tracer(f, _tau(real, grid), resident)
    for levels, top, nt_s in (([10., 20.], 0.0, 1), ([8., 16., 24.], -1.5, NT), (list(2.5 + 2.75 * numpy.arange(8)), 0.0, 1)):
        _set_surfaces(f, _const(real, grid, levels, nt_s), resident, top=top)
        f.setDepthEdges(levels, top)
        for t in range(NT):
            for carry in (False, True):
                want = _dt(f, t, carry)
                assert (numpy.abs(want).max(axis=1) > 0).sum() >= 3
                assert _same_bits(_st(f, t, carry), want), (levels, t, carry)
    for e in (10., 5.5):
        _set_surfaces(f, _const(real, grid, [e]), resident)
        f.setDepthEdges([e, 1e300])
        for carry in (False, True):
            got, want = _st(f, 1, carry), _dt(f, 1, carry)
            assert got.shape == (3, f._rowlen) and numpy.abs(want[:2]).max(axis=1).min() > 0
            assert _same_bits(got, want[[0, 1, 3]]), (e, carry)


BLOCK_LINES = ['(-160,-40),(-100,30)', '(-30,-50),(30,40)', '(90,-30),(150,50)']
BLOCK_EDGES = [[3., 9., 15.], [5.5, 8., 20.], [1., 10., 12.25]]


@pytest.mark.parametrize('thick', ['scalar', 'timevarying'])
@pytest.mark.parametrize('real', ['float64', 'float32'])
def test_surfaces_constant_on_blocks_of_columns_give_each_block_its_depth_bins(real, thick):
    """three blocks of 24 columns with edges of their own and three transects, each at least two cells inside one block: per
    transect the columns are those of computeDepthTransport with that block's edges"""
    grid, resident = GRIDS[0], True
    nx, ny = grid
    f = _make(real, grid, resident, lines=BLOCK_LINES, sverdrup=True)
    ce = f.getWeights()[0]
    cols, seg = ce // 4 % nx, f.getWeights()[2]
    for p in range(3):          # every cell a transect touches, and its neighbours, lie two cells inside block p
        mine = cols[(seg >= f._tr_off[p]) & (seg < f._tr_off[p + 1])]
        assert mine.size > 0 and mine.min() >= 24 * p + 2 and mine.max() <= 24 * p + 21, p
    _set_thickness(f, real, grid, resident, thick)
    _set_tracer(f, _tau(real, grid), resident)
    s = numpy.empty((1, 3, ny, nx), real)
    for p in range(3):
        s[0, :, :, 24 * p:24 * (p + 1)] = numpy.asarray(BLOCK_EDGES[p], dtype=real)[:, None, None]
    _set_surfaces(f, s, resident)
    for t in range(NT):
        for carry in (False, True):
            got = _st(f, t, carry)
            for p in range(3):
                f.setDepthEdges(BLOCK_EDGES[p])
                want = _dt(f, t, carry)
                pick = list(range(f._tr_off[p], f._tr_off[p + 1])) + [f._nseg + p]
                assert numpy.abs(want[:, pick]).max() > 0 and _same_bits(got[:, pick], want[:, pick]), (t, carry, p)


@pytest.mark.parametrize('thick', ['scalar', 'timevarying'])
@pytest.mark.parametrize('grid', GRIDS, ids=lambda g: f'{g[0]}x{g[1]}')
@pytest.mark.parametrize('real', ['float64', 'float32'])
def test_negated_and_doubled_velocities_negate_and_double_the_rows(real, grid, thick):
    resident = grid == GRIDS[0]
    u, v = _uv(real, grid)
    dt = u.dtype.type

    def scaled(x, s):
        keep = numpy.isnan(x) | (x == dt(FILL)) | (x == dt(MISSING))
        return numpy.where(keep, x, dt(s) * x)

    fields = [_make(real, grid, resident, sverdrup=True)]
    fields += [_make(real, grid, resident, u=scaled(u, s), v=scaled(v, s), sverdrup=True) for s in (-1., 2.)]
    for f in fields:
        _set_thickness(f, real, grid, resident, thick)
        _set_tracer(f, _tau(real, grid), resident)
        _set_surfaces(f, _surf(real, grid, 8, NT), resident)
    a, neg, dbl = fields
    for t in range(NT):
        for carry in (False, True):
            rows = _st(a, t, carry)
            assert (numpy.abs(rows).max(axis=1) > 0).all()
            assert numpy.array_equal(_st(neg, t, carry), -rows), (t, carry)
            assert numpy.array_equal(_st(dbl, t, carry), 2. * rows), (t, carry)


@pytest.mark.parametrize('thick', ['scalar', 'timevarying'])
@pytest.mark.parametrize('grid', GRIDS, ids=lambda g: f'{g[0]}x{g[1]}')
@pytest.mark.parametrize('real', ['float64', 'float32'])
def test_tracer_one_above_the_reference_is_carried_like_the_water(real, grid, thick):
    """tau == ref + 1 everywhere: tf == 1 exactly at every face that has a value, so the carried rows are the volume rows"""
    resident = grid == GRIDS[1]
    nx, ny = grid
    tau = numpy.full((NT, NZ, ny, nx), 8., real)
    f = _make(real, grid, resident)
    assert (f.getWeights()[0] // 4 // nx).max() < ny - 1
    _set_thickness(f, real, grid, resident, thick)
    f.setTracer(_on(tau, resident), reference=7.0)
    _set_surfaces(f, _surf(real, grid, 3, 1), resident)
    for t in range(NT):
        vol = _st(f, t)
        assert (numpy.abs(vol).max(axis=1) > 0).all()
        assert numpy.array_equal(_st(f, t, carry=True), vol), t
    f.setTracer(_on(tau, resident), reference=6.0)                 # tf == 2: exactly twice
    assert numpy.array_equal(_st(f, 1, carry=True), 2. * _st(f, 1))


@pytest.mark.parametrize('nt_th', [1, NT], ids=['static', 'timevarying'])
@pytest.mark.parametrize('grid', GRIDS, ids=lambda g: f'{g[0]}x{g[1]}')
@pytest.mark.parametrize('real', ['float64', 'float32'])
def test_broadcast_cell_thickness_is_the_scalar_form(real, grid, nt_th):
    from depth_remap_reference import GPU_TH
    resident = grid == GRIDS[0]
    tau = _tau(real, grid)
    a, b = _make(real, grid, resident), _make(real, grid, resident)
    e3 = _broadcast(real, grid, nt_th, GPU_TH)
    b.setCellThickness(_on(e3, resident), _on(e3.copy(), resident))
    for f in (a, b):
        _set_tracer(f, tau, resident)
        _set_surfaces(f, _surf(real, grid, 8, NT), resident, top=-1.5)
    for t in range(NT):
        for carry in (False, True):
            want = _st(a, t, carry)
            assert (numpy.abs(want).max(axis=1) > 0).all()
            assert _same_bits(_st(b, t, carry), want), (t, carry)


@pytest.mark.parametrize('thick', ['scalar', 'timevarying'])
@pytest.mark.parametrize('real', ['float64', 'float32'])
def test_same_bits_for_every_window_home_out_and_copies_of_a_static_set(real, thick):
    import torch
    grid, m = GRIDS[1], 8
    s = _surf(real, grid, m, 1)
    fields = []
    for resident, copies in ((True, False), (False, False), (True, True), (False, True)):
        f = _make(real, grid, resident)
        _set_thickness(f, real, grid, resident, thick)
        _set_tracer(f, _tau(real, grid), resident)
        _set_surfaces(f, numpy.ascontiguousarray(numpy.broadcast_to(s, (NT,) + s.shape[1:])) if copies else s, resident)
        fields.append(f)
    f, host, dev_copies, host_copies = fields
    shape = (m + 2, f._rowlen)
    for t in (2, 0):
        for carry in (False, True):
            want = _st(f, t, carry)
            assert (numpy.abs(want).max(axis=1) > 0).all()
            for window in (1, 5, 32):
                with _knob(b'class_window', window, 32):
                    assert _same_bits(_st(f, t, carry), want), (t, carry, window)
                    assert _same_bits(_st(host_copies, t, carry), want), (t, carry, window)
            out = torch.full(shape, numpy.nan, dtype=torch.float64, device='cuda')
            assert _same_bits(_st(f, t, carry, out=out), want)
            assert _same_bits(out.cpu().numpy(), want)
            assert _same_bits(_st(host, t, carry), want)               # host-resident inputs, staged
            out.fill_(numpy.nan)
            assert _same_bits(_st(host, t, carry, out=out), want)
            assert _same_bits(_st(dev_copies, t, carry), want)         # (nt, ny, nx) copies of the static set
    for bad in (torch.zeros(shape, dtype=torch.float32, device='cuda'),
                torch.zeros((shape[0] + 1, shape[1]), dtype=torch.float64, device='cuda'), torch.zeros(shape, dtype=torch.float64)):
        with pytest.raises(RuntimeError, match='out must be'):
            f.computeSurfaceTransport(0, out=bad)


# ---- conservation and closure ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize('thick', THICK)
@pytest.mark.parametrize('grid', GRIDS, ids=lambda g: f'{g[0]}x{g[1]}')
@pytest.mark.parametrize('real', ['float64', 'float32'])
def test_the_rows_add_up_to_the_profile_rows_and_the_tracer_row(real, grid, thick):
    """the sum over the m + 2 rows against the sum over z of computeFluxProfile under the same thickness, and for the carried
    form against computeTracerFlux, within 1e-12 x the reference's sum |terms|"""
    resident = (grid == GRIDS[0]) == (real == 'float64')
    u, v = _uv(real, grid)
    tau = _tau(real, grid)
    f = _make(real, grid, resident, sverdrup=True)
    arrays = {'uo': u, 'vo': v, 'tracer': tau}
    arrays.update(_set_thickness(f, real, grid, resident, thick))
    _set_tracer(f, tau, resident)
    r = _reference(f, sverdrup=True, cell_thickness=thick != 'scalar')
    for k in range(len(GPU_M)):
        m, t, top, nt_s = gpu_case(k, THICK.index(thick), NT)
        _set_surfaces(f, _surf(real, grid, m, nt_s), resident, top=top)
        mags = r.step(array_values(arrays, t))
        _check(_st(f, t).sum(axis=0), _rows(f.computeFluxProfile(t)).sum(axis=0), mags['volume'][1], f'volume m={m} t={t}')
        _check(_st(f, t, True).sum(axis=0), _rows(f.computeTracerFlux(t)), mags['tracer'][1], f'carried m={m} t={t}')


@pytest.mark.parametrize('home', ['hbm', 'host'])
@pytest.mark.parametrize('thick', ['scalar', 'timevarying'])
@pytest.mark.parametrize('real', ['float64', 'float32'])
def test_two_sharded_halves_add_up_to_the_unsharded_rows(real, thick, home):
    """slab ranges that cut inside a time step: the running sum of the lower half starts at level 0 all the same; every rank's
    rows are the reference's for its levels, the halves add up to the unsharded rows, a step that a rank does not touch gives
    exact zeros"""
    from nemoflux_amd.dist import slab_range
    grid, world, resident, m = GRIDS[1], 2, home == 'hbm', 8
    u, v = _uv(real, grid)
    tau = _tau(real, grid)
    s = _surf(real, grid, m, NT)
    arrays = {'uo': u, 'vo': v, 'tracer': tau, 'surface': s}

    def make(**kw):
        f = _make(real, grid, resident, **kw)
        arrays.update(_set_thickness(f, real, grid, resident, thick))
        _set_tracer(f, tau, resident)
        _set_surfaces(f, s, resident)
        return f

    full = make()
    r = _reference(full, cell_thickness=thick != 'scalar')
    want = numpy.array([[_st(full, t, carry) for carry in (False, True)] for t in range(NT)])
    acc = numpy.zeros_like(want)
    cut_inside = untouched = False
    for rank in range(world):
        sr = slab_range(NT, NZ, rank, world)
        cut_inside = cut_inside or sr[0] % NZ != 0
        part = make(slab_range=sr)
        for t in range(NT):
            z0, z1 = max(sr[0], t * NZ) - t * NZ, min(sr[1], (t + 1) * NZ) - t * NZ
            ref = r.surface_step(surface_values(arrays, t), m, levels=(z0, z1)) if z1 > z0 else None
            for k, (carry, nm) in enumerate(((False, 'volume'), (True, 'carried'))):
                got = _st(part, t, carry)
                if ref is None:
                    untouched = True
                    assert not got.view(numpy.uint64).any(), (rank, t, carry)
                else:
                    _close(got, *ref[nm], f'rank {rank} levels [{z0}, {z1}) {nm} t={t}')
                acc[t, k] += got
    assert cut_inside and untouched
    for t in range(NT):
        ref = r.surface_step(surface_values(arrays, t), m)
        for k, nm in enumerate(('volume', 'carried')):
            _check(acc[t, k], want[t, k], ref[nm][1], f'two halves, {nm} t={t}')


@pytest.mark.parametrize('nt_s', [1, NT], ids=['static', 'timevarying'])
@pytest.mark.parametrize('real', ['float64', 'float32'])
def test_mean_eddy_split_closes_with_static_surfaces_and_carries_the_mean_of_varying_ones(real, nt_s):
    """static surfaces and a tracer constant in time: the product is linear in (uo, vo), so the eddy part is rounding -- inside
    1e-12 x (the mean over the steps of sum |share| + sum |share| of the mean state), the bar of tests/test_gpu_selected_mean.py.
    Time-varying surfaces: the mean Field carries their weighted mean over the visited steps by the tracer rule"""
    grid, resident, m = GRIDS[0], True, 3
    select, weights = [0, 2], [1., 3.]
    u, v = _uv(real, grid)
    tau = numpy.ascontiguousarray(numpy.broadcast_to(_tau(real, grid)[1], u.shape))
    s = _surf(real, grid, m, nt_s)
    f = _make(real, grid, resident, sverdrup=True)
    _set_tracer(f, tau, resident)
    _set_surfaces(f, s, resident, top=-1.5)
    for carry in (False, True):
        d = _quiet(f.meanEddySplit, 'computeSurfaceTransport', select=select, weights=weights, carry=carry)
        mean = d['meanField']
        got = mean._surfaces
        assert got['nt'] == 1 and got['top'] == -1.5 and len(got['items']) == m
        items = [x.cpu().numpy() if hasattr(x, 'cpu') else numpy.asarray(x) for x in got['items']]
        if nt_s == 1:
            for k in range(m):
                assert numpy.array_equal(items[k], s[0, k].astype(numpy.float64), equal_nan=True)
            r = _reference(f, sverdrup=True)
            rm = _reference(mean, sverdrup=True, uv_markers=tuple(x for x in mean._uv_markers if x == x))
            nm = 'carried' if carry else 'volume'
            mags = [r.surface_step(surface_values({'uo': u, 'vo': v, 'tracer': tau, 'surface': s}, t), m, top=-1.5)[nm][1]
                    for t in select]
            marr = {'uo': mean._uv[0].cpu().numpy(), 'vo': mean._uv[1].cpu().numpy(), 'tracer': tau[:1].astype(numpy.float64),
                    'surface': s.astype(numpy.float64)}
            bar = BAR * (numpy.mean(mags, axis=0) + rm.surface_step(surface_values(marr, 0), m, top=-1.5)[nm][1])
            eddy, total = _rows(d['eddy']), _rows(d['total'])
            print(f'{real} carry={carry}: max |eddy| / bar = {float((numpy.abs(eddy) / numpy.maximum(bar, 1e-300)).max()):.3g}')
            assert eddy.shape == bar.shape and numpy.abs(total).max() > 0 and bar.max() > 0
            assert numpy.all(numpy.abs(eddy) <= bar), carry
        else:
            dt = s.dtype.type
            w = numpy.array(weights)
            for k in range(m):
                x = s[select, k]
                ok = numpy.isfinite(x) | numpy.isinf(x)
                ok &= (x != dt(SFILL)) & (x != dt(SMISSING))
                num = (w[:, None, None] * numpy.where(ok, x, 0).astype(numpy.float64)).sum(axis=0)
                den = (w[:, None, None] * ok).sum(axis=0)
                with numpy.errstate(invalid='ignore', divide='ignore'):
                    want = numpy.where(den > 0, num / den, SFILL)
                assert numpy.allclose(items[k], want, rtol=1e-15, atol=0, equal_nan=True), k
            assert numpy.isfinite(_rows(d['mean'])[:m + 1]).all()


# ---- refusals and files ----------------------------------------------------------------------------------------------------
def test_the_refusals_have_the_siblings_words():
    from nemoflux_amd._lib import lib
    real, grid = 'float64', GRIDS[0]
    f = _make(real, grid, True)
    for carry in (False, True):
        with pytest.raises(RuntimeError, match='setDepthSurfaces first'):
            f.computeSurfaceTransport(0, carry=carry)
    host = numpy.zeros((4, f._rowlen))
    assert lib.nf_field_compute_surface_transport(ctypes.byref(f._h), 0, 0, host.ctypes.data_as(dp)) == 2
    assert 'nf_field_compute_surface_transport: set_depth_surfaces first' in lib.nf_last_error().decode()
    f.setDepthEdges(numpy.array([3., 9.]))                       # another set: the surface call does not see it
    with pytest.raises(RuntimeError, match='setDepthSurfaces first'):
        f.computeSurfaceTransport(0)
    _set_surfaces(f, _surf(real, grid, 2, 1), True)
    with pytest.raises(RuntimeError, match='setTracer first'):
        f.computeSurfaceTransport(0, carry=True)
    assert lib.nf_field_compute_surface_transport(ctypes.byref(f._h), NT, 0, host.ctypes.data_as(dp)) == 1
    assert b'time index' in lib.nf_last_error()
    assert not host.any() and numpy.abs(_st(f, 0)).max() > 0
    with pytest.raises(RuntimeError, match='float32, uo/vo are float64'):
        f.setDepthSurfaces([_on(_surf('float32', grid, 1, 1)[0, 0], True)])
    f.setDepthSurfaces([_surf('float32', grid, 1, 1)[0, 0]], fill_value=SFILL, missing_value=SMISSING)   # a host array is cast
    a = _st(f, 0)
    f.setDepthSurfaces([_surf('float32', grid, 1, 1)[0, 0].astype(numpy.float64)], fill_value=SFILL, missing_value=SMISSING)
    assert numpy.abs(a).max() > 0 and _same_bits(_st(f, 0), a)
    f.setDepthSurfaces(None)
    with pytest.raises(RuntimeError, match='setDepthSurfaces first'):
        f.computeSurfaceTransport(0)
    assert numpy.abs(_dt(f, 0)).max() > 0


@pytest.mark.parametrize('form', ['volume', 'carried', 'cell'])
@pytest.mark.parametrize('kind', ['npz', 'classic'])
def test_fluxplot_depth_surfaces_is_the_field_table(tmp_path, form, kind):
    from nemoflux_amd import fluxplot
    real, grid, m = 'float32', GRIDS[0], 3
    blon, blat = _case(real, grid)[:2]
    u, v = _uv(real, grid)
    tau = _tau(real, grid)
    from test_gpu_depth_remap import _e3
    e3u, e3v = _e3(real, grid, NT)
    s = _surf(real, grid, m, NT)
    names = ['mld', 'iso20', 'bottom200']
    surf = {n: numpy.ascontiguousarray(s[:, k]) for k, n in enumerate(names)}
    if kind == 'npz':
        paths = {k: str(tmp_path / f'{k}.npz') for k in 'TUVS'}
        fv = lambda name, a, b: {f'_FillValue_{name}': numpy.array(a), f'_missing_value_{name}': numpy.array(b)}   # noqa: E731
        numpy.savez(paths['T'], bounds_lon=blon, bounds_lat=blat, deptht_bounds=DB, thetao=tau, **fv('thetao', TFILL, TMISSING))
        numpy.savez(paths['U'], uo=u, e3u=e3u, **fv('uo', FILL, MISSING), **fv('e3u', THFILL, THMISSING))
        numpy.savez(paths['V'], vo=v, e3v=e3v, **fv('vo', FILL, MISSING), **fv('e3v', THFILL, THMISSING))
        marks = {}
        for n in names:
            marks.update(fv(n, SFILL, SMISSING))
        numpy.savez(paths['S'], **surf, **marks)
    else:
        from scipy.io import netcdf_file
        paths = {k: str(tmp_path / f'{k}.nc') for k in 'TUVS'}
        nx, ny = grid

        def write(path, variables):
            sizes = {'t': None, 'z': NZ, 'y': ny, 'x': nx, 'four': 4, 'two': 2}
            nc = netcdf_file(path, 'w', version=2)
            for dim in sizes:                     # the record dimension first, only where a variable has it
                if any(dim in dims for _, dims, _, _ in variables.values()):
                    nc.createDimension(dim, sizes[dim])
            if 't' in nc.dimensions:
                tc = nc.createVariable('time_counter', 'f8', ('t',))
                tc.standard_name, tc.units, tc.calendar = 'time', 'seconds since 1900-01-01 00:00:00', 'noleap'
                tc[:] = numpy.arange(NT) * 86400. * 30.5 + 1296000.
            for name, (a, dims, fill, missing) in variables.items():
                var = nc.createVariable(name, a.dtype.str[1:], dims)
                if fill is not None:
                    var._FillValue = a.dtype.type(fill)
                    var.missing_value = a.dtype.type(missing)
                var[:] = a
            nc.close()

        four = ('t', 'z', 'y', 'x')
        write(paths['T'], {'bounds_lon': (blon, ('y', 'x', 'four'), None, None), 'bounds_lat': (blat, ('y', 'x', 'four'), None, None),
                           'deptht_bounds': (DB, ('z', 'two'), None, None), 'thetao': (tau, four, TFILL, TMISSING)})
        write(paths['U'], {'uo': (u, four, FILL, MISSING), 'e3u': (e3u, four, THFILL, THMISSING)})
        write(paths['V'], {'vo': (v, four, FILL, MISSING), 'e3v': (e3v, four, THFILL, THMISSING)})
        write(paths['S'], {n: (a, ('t', 'y', 'x'), SFILL, SMISSING) for n, a in surf.items()})
    lines = '[' + T_OPEN + '],[' + T_SEAM + ']'
    out = str(tmp_path / 'surfaces.csv')
    kw = dict(tFile=paths['T'], uFile=paths['U'], vFile=paths['V'], depthSurfaces=','.join(names), surfaceFile=paths['S'],
              depthTop=-1.5)
    if form != 'volume':
        kw.update(tracer='thetao', tracerRef=1.5, tracerScale=4.1e-3)
    if form == 'cell':
        kw.update(cellThickness=True)
    totals = _quiet(fluxplot.main, lonLatPoints=lines, output=out, sverdrup=True, **kw)
    mem = _field(blon, blat, DB, u, v, fluxplot.readTargets(lines)[0], True, fill_value=FILL, missing_value=MISSING,
                 readback=False)
    if form != 'volume':
        mem.setTracer(tau, fill_value=TFILL, missing_value=TMISSING, reference=1.5)
    if form == 'cell':
        mem.setCellThickness(e3u, e3v, fill_value=THFILL, missing_value=THMISSING)
    mem.setDepthSurfaces([surf[n] for n in names], top=-1.5, fill_value=SFILL, missing_value=SMISSING)
    with open(out) as fh:
        text = fh.read().splitlines()
    title = ('# water flow by layer between surfaces [Sv]' if form == 'volume'
             else '# transport of thetao by layer between surfaces [thetao x Sv x 0.0041]')
    assert text[0] == title + (', depths from the cell thicknesses' if form == 'cell' else '')
    assert text[1] == 'time,upper,lower,line0,line1'
    assert text[2].split(',')[1:3] == ['top', 'mld'] and text[5].split(',')[1:3] == ['bottom200', 'bottom']
    assert text[6].split(',')[1:3] == ['nan', 'nan']
    assert totals.shape == (NT, m + 2, 2) and len(text) == 2 + NT * (m + 2)
    for t in range(NT):
        want = mem.computeSurfaceTransport(t, carry=form != 'volume')[0] * (1.0 if form == 'volume' else 4.1e-3)
        assert _same_bits(totals[t], want) and (numpy.abs(want).max(axis=1) > 0).all()
        row = numpy.array([float(x) for x in text[2 + t * (m + 2) + 1].split(',')[3:]])
        assert numpy.allclose(row, want[1], rtol=1e-14, atol=0)
