"""Transports in true-depth bins on the GPU (Field.computeDepthTransport, nf_field_compute_depth_transport, fluxplot
--depth-bins).  Every value of every row in all four forms -- volume or carried tracer, scalar or per-cell thickness -- is
checked against the float64 / long-double restatement of the definition in tests/depth_remap_reference.py to
1e-12 x sum |share| of that value (the A7 bar of docs/PARITY.md), no row or column left out; anchored bit for bit (edges at the
level interfaces give the profile rows; a broadcast cell thickness gives the scalar form; negated / doubled uo, vo negate /
double the rows; tau = ref + 1 gives the volume form; every class_window, out= and host inputs give the same bits); two closed
forms that share nothing with the reference; the sum over the rows against the profile rows and the tracer row; one +inf
thickness; two sharded halves against the unsharded rows; the refusals; timeMean(thicknessWeighted=True) Fields; fluxplot
--depth-bins from files.

Grids 72 x 36 x 7 x 3 and 73 x 37 x 7 x 3 with the three transects of tests/test_gpu_class_remap.py (one across the periodic
seam; two blocks of records, the second one short); seven levels leave a tail behind the batch length of the kernel.  The
thicknesses are multiples of 1/8 in [0.25, 4] with exact zeros, both markers and NaN (tests/depth_remap_reference.py), so every
interface depth is exact and lands on edges; tests/test_depth_remap_cpu.py checks without a GPU that with these inputs terms
are spread over several rows, terms have lo == hi and interface depths are exactly an edge.

Measured on an MI355X: see the figures printed by each test; docs/PARITY.md quotes the worst."""
import ctypes

import numpy
import pytest

from conftest import transect_xyz
from depth_remap_reference import EDGES, GPU_E3_SEED, GPU_TH as TH, DepthRemapReference, depth_thickness
from gpu_helpers import _field, _knob, _on, _quiet, _rows, _same_bits
from gross_reference import array_values
from test_gpu_cellthick import BAR, FILL, MISSING, T_OPEN, T_SEAM, T_TRI, TFILL, THFILL, THMISSING, TMISSING, _case
from test_gpu_gross import GRIDS, NT, NZ, REF, _tau, _uv

pytestmark = pytest.mark.gpu

LINES = [T_OPEN, T_TRI, T_SEAM]
DB = numpy.stack([numpy.concatenate([[0.], numpy.cumsum(TH)[:-1]]), numpy.cumsum(TH)], axis=1)
THICK = ['scalar', 'static', 'timevarying']
dp = ctypes.POINTER(ctypes.c_double)
_E3 = {}
WORST = {'reference': 0.0}


def _e3(real, grid, nt_th):
    if (real, grid, nt_th) not in _E3:
        _E3[real, grid, nt_th] = depth_thickness(real, (nt_th, NZ, grid[1], grid[0]), seed=GPU_E3_SEED)
    return _E3[real, grid, nt_th]


def _make(real, grid, resident, u=None, v=None, db=DB, lines=LINES, **kw):
    blon, blat = _case(real, grid)[:2]
    u0, v0 = _uv(real, grid)
    kw.setdefault('readback', False)
    kw.setdefault('fill_value', FILL)
    kw.setdefault('missing_value', MISSING)
    return _field(blon, blat, db, _on(u0 if u is None else u, resident), _on(v0 if v is None else v, resident),
                  [transect_xyz(s) for s in lines], **kw)


def _set_thickness(f, real, grid, resident, thick, e3=None):
    """thick: 'scalar' (nothing to set), 'static' or 'timevarying'; returns the arrays for the reference"""
    if thick == 'scalar':
        return {}
    e3u, e3v = _e3(real, grid, NT if thick == 'timevarying' else 1) if e3 is None else e3
    f.setCellThickness(_on(e3u, resident), _on(e3v, resident), fill_value=THFILL, missing_value=THMISSING)
    return dict(e3u=e3u, e3v=e3v)


def _set_tracer(f, tau, resident, ref=REF, wrap=True):
    f.setTracer(_on(tau, resident), fill_value=TFILL, missing_value=TMISSING, reference=ref, wrapX=wrap)


def _dt(f, t, carry=False, **kw):
    """(nedges + 2, row_length): [segments | transects] rows"""
    return _rows(f.computeDepthTransport(t, carry=carry, **kw))


def _reference(f, wrap=True, ref=REF, sverdrup=False, cell_thickness=False):
    ce, w, sg = f.getWeights()
    return DepthRemapReference(ce, w, sg, f.arcLengths, f.thickness, f._tr_off, f.nx, f.ny, uv_markers=(FILL, MISSING),
                               tracer_markers=(TFILL, TMISSING), thick_markers=(THFILL, THMISSING), reference=ref, wrap=wrap,
                               sverdrup=sverdrup, cell_thickness=cell_thickness)


def _close(got, want, mag, label):
    assert got.shape == want.shape == mag.shape, label
    err = numpy.abs(got - want)
    worst = float((err / numpy.maximum(mag, 1e-300)).max())
    print(f'{label}: max |err| / sum |share| = {worst:.3g}')
    assert numpy.all(err <= BAR * mag), (label, worst)
    return worst


def _check(got, want, mag, label):
    err = numpy.abs(got - want)
    worst = float((err / numpy.maximum(mag, 1e-300)).max())
    print(f'{label}: max |err| / sum |terms| = {worst:.3g}')
    assert want.shape == got.shape == mag.shape and numpy.abs(want).max() > 0 and numpy.all(err <= BAR * mag), (label, worst)


def _profile(f, t, carry):
    return _rows((f.computeTracerProfile if carry else f.computeFluxProfile)(t))


def _interfaces(thickness, top=0.0):
    """D_0 .. D_nz by the loop of the definition"""
    D = [float(top)]
    for h in thickness:
        D.append(D[-1] + float(h))
    return numpy.array(D)


def _broadcast(real, grid, nt_th, th):
    nx, ny = grid
    return numpy.ascontiguousarray(numpy.broadcast_to(numpy.asarray(th).astype(real)[None, :, None, None], (nt_th, NZ, ny, nx)))


# ---- 4. against the reference ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize('thick', THICK)
@pytest.mark.parametrize('wrap', [True, False], ids=['wrap-sv', 'nowrap-m2'])
@pytest.mark.parametrize('resident', [True, False], ids=['hbm', 'host'])
@pytest.mark.parametrize('grid', GRIDS, ids=lambda g: f'{g[0]}x{g[1]}')
@pytest.mark.parametrize('real', ['float64', 'float32'])
def test_against_the_reference(real, grid, resident, wrap, thick):
    """volume and carried forms; every edge count, each on one of the steps; top = -1.5 with the 16 edges"""
    u, v = _uv(real, grid)
    dt = u.dtype.type
    assert numpy.isnan(v).any() and (u == dt(FILL)).any() and (u == dt(MISSING)).any() and (u == 0).any()
    tau = _tau(real, grid)
    f = _make(real, grid, resident, sverdrup=wrap)
    ce = f.getWeights()[0]
    assert ce.size > 256 and (ce // 4 % f.nx == f.nx - 1).any()        # two blocks; the seam: east faces of the last column
    arrays = {'uo': u, 'vo': v, 'tracer': tau}
    arrays.update(_set_thickness(f, real, grid, resident, thick))
    for a in (arrays.get('e3u'), arrays.get('e3v')):
        assert a is None or (numpy.isnan(a).any() and (a == 0).any() and (a == dt(THFILL)).any() and (a == dt(THMISSING)).any()
                             and not numpy.isinf(a).any())
    _set_tracer(f, tau, resident, wrap=wrap)
    r = _reference(f, wrap=wrap, sverdrup=wrap, cell_thickness=thick != 'scalar')
    for k, (n, edges) in enumerate(EDGES.items()):
        t, top = k % NT, (-1.5 if n == 16 else 0.0)
        f.setDepthEdges(edges, top)
        want = r.depth_step(array_values(arrays, t), edges, top=top)
        vol, car = _dt(f, t), _dt(f, t, carry=True)
        assert vol.shape == car.shape == (n + 2, f._rowlen)
        label = f'{thick} n={n} t={t}'
        for got, nm in ((vol, 'volume'), (car, 'carried')):
            WORST['reference'] = max(WORST['reference'], _close(got, *want[nm], f'{nm} {label}'))
            assert not got[n + 1].view(numpy.uint64).any(), label              # every depth is finite: exactly +0.0
        assert want['spread_terms'] > 0 and want['on_edge'] > 0 and (want['flat_terms'] > 0 or thick == 'scalar')
        assert (want['volume'][1].max(axis=1) > 0).sum() >= (3 if n < 16 else 8)
    print(f'worst so far against the reference: {WORST["reference"]:.3g}')


# ---- 5. bit-for-bit identities ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize('resident', [True, False], ids=['hbm', 'host'])
@pytest.mark.parametrize('grid', GRIDS, ids=lambda g: f'{g[0]}x{g[1]}')
@pytest.mark.parametrize('real', ['float64', 'float32'])
def test_edges_at_the_level_interfaces_give_the_profile_rows(real, grid, resident):
    """scalar thickness, edges D_1 .. D_{nz-1} from a loop over the Field's own thickness: the interval of level z is
    [e[z-1], e[z]] (from `top`, or with no edge below, at the two ends), so row z gets the fraction (hi - lo) / (hi - lo) = 1
    of exactly the terms of level z, added in the order of the profile kernel, and the zero-width share of row z + 1 is
    nothing; row n + 1 is +0.0"""
    f = _make(real, grid, resident, sverdrup=True)
    _set_tracer(f, _tau(real, grid), resident)
    for top in (0.0, -1.5):
        D = _interfaces(f.thickness, top)
        f.setDepthEdges(D[1:NZ], top)
        for t in range(NT):
            for carry in (False, True):
                got, want = _dt(f, t, carry), _profile(f, t, carry)
                assert got.shape == (NZ + 1, f._rowlen) and (numpy.abs(want).max(axis=1) > 0).all()
                assert numpy.array_equal(got[:NZ], want), (top, t, carry)
                assert not got[NZ].view(numpy.uint64).any()


@pytest.mark.parametrize('nt_th', [1, NT], ids=['static', 'timevarying'])
@pytest.mark.parametrize('resident', [True, False], ids=['hbm', 'host'])
@pytest.mark.parametrize('grid', GRIDS, ids=lambda g: f'{g[0]}x{g[1]}')
@pytest.mark.parametrize('real', ['float64', 'float32'])
def test_broadcast_cell_thickness_is_the_scalar_form(real, grid, resident, nt_th):
    tau = _tau(real, grid)
    a, b = _make(real, grid, resident), _make(real, grid, resident)
    e3 = _broadcast(real, grid, nt_th, TH)
    b.setCellThickness(_on(e3, resident), _on(e3.copy(), resident))
    for f in (a, b):
        _set_tracer(f, tau, resident)
        f.setDepthEdges(EDGES[1025], -1.5)
    for t in range(NT):
        for carry in (False, True):
            want = _dt(a, t, carry)
            assert (numpy.abs(want).max(axis=1) > 0).sum() > 500
            assert _same_bits(_dt(b, t, carry), want), (t, carry)


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
        f.setDepthEdges(EDGES[1025])
    a, neg, dbl = fields
    for t in range(NT):
        for carry in (False, True):
            rows = _dt(a, t, carry)
            assert (numpy.abs(rows).max(axis=1) > 0).sum() > 500
            assert numpy.array_equal(_dt(neg, t, carry), -rows), (t, carry)
            assert numpy.array_equal(_dt(dbl, t, carry), 2. * rows), (t, carry)


@pytest.mark.parametrize('thick', ['scalar', 'timevarying'])
@pytest.mark.parametrize('grid', GRIDS, ids=lambda g: f'{g[0]}x{g[1]}')
@pytest.mark.parametrize('real', ['float64', 'float32'])
def test_tracer_one_above_the_reference_is_carried_like_the_water(real, grid, thick):
    """tau == ref + 1 everywhere: tf == 1 exactly at every face that has a value, so the carried rows are the volume rows.
    With wrapX only the north faces of the last row have no value, and no line comes near it."""
    resident = grid == GRIDS[1]
    nx, ny = grid
    tau = numpy.full((NT, NZ, ny, nx), 8., real)
    f = _make(real, grid, resident)
    assert (f.getWeights()[0] // 4 // nx).max() < ny - 1
    _set_thickness(f, real, grid, resident, thick)
    f.setTracer(_on(tau, resident), reference=7.0)
    f.setDepthEdges(EDGES[1025])
    for t in range(NT):
        vol = _dt(f, t)
        assert (numpy.abs(vol).max(axis=1) > 0).sum() > 500
        assert numpy.array_equal(_dt(f, t, carry=True), vol), t
    f.setTracer(_on(tau, resident), reference=6.0)                 # tf == 2: exactly twice
    assert numpy.array_equal(_dt(f, 1, carry=True), 2. * _dt(f, 1))


@pytest.mark.parametrize('thick', ['scalar', 'timevarying'])
@pytest.mark.parametrize('real', ['float64', 'float32'])
def test_same_bits_for_every_window_home_and_out(real, thick):
    import torch
    grid = GRIDS[1]
    fields = []
    for resident in (True, False):
        f = _make(real, grid, resident)
        _set_thickness(f, real, grid, resident, thick)
        _set_tracer(f, _tau(real, grid), resident)
        f.setDepthEdges(2. * numpy.arange(17))                     # 19 rows: one window of 32, four of 5, 19 of 1
        fields.append(f)
    f, host = fields
    shape = (19, f._rowlen)
    for t in (2, 0):
        for carry in (False, True):
            want = _dt(f, t, carry)
            assert (numpy.abs(want).max(axis=1) > 0).sum() > 10
            for window in (1, 5, 32):
                with _knob(b'class_window', window, 32):
                    assert _same_bits(_dt(f, t, carry), want), (t, carry, window)
            out = torch.full(shape, numpy.nan, dtype=torch.float64, device='cuda')
            assert _same_bits(_dt(f, t, carry, out=out), want)
            assert _same_bits(out.cpu().numpy(), want)
            assert _same_bits(_dt(host, t, carry), want)               # host-resident inputs, staged
            out.fill_(numpy.nan)
            assert _same_bits(_dt(host, t, carry, out=out), want)
    for bad in (torch.zeros(shape, dtype=torch.float32, device='cuda'),
                torch.zeros((shape[0] + 1, shape[1]), dtype=torch.float64, device='cuda'), torch.zeros(shape, dtype=torch.float64)):
        with pytest.raises(RuntimeError, match='out must be'):
            f.computeDepthTransport(0, out=bad)


# ---- 6. closed forms that share nothing with the reference -----------------------------------------------------------------
@pytest.mark.parametrize('resident', [True, False], ids=['hbm', 'host'])
@pytest.mark.parametrize('grid', GRIDS, ids=lambda g: f'{g[0]}x{g[1]}')
@pytest.mark.parametrize('real', ['float64', 'float32'])
def test_the_closed_form_of_edges_at_mid_depth_of_equal_layers(real, grid, resident):
    """h = 2 on every level and edges (k + 1/2) h, k = 0 .. nz - 1: level z covers [z h, (z + 1) h], cut in half by edge z, so
    row 0 = P_0 / 2, row k = P_{k-1} / 2 + P_k / 2, row nz = P_{nz-1} / 2 and row nz + 1 is +0.0; P: the profile rows.  The
    volume form with the thickness broadcast over the grid, the carried form with the per-level thickness (the tracer profile
    takes no cell thickness).  Nothing here comes from the reference but sum |terms| of the profile rows."""
    h = 2.0
    th = numpy.full(NZ, h)
    db = numpy.stack([h * numpy.arange(NZ), h * (numpy.arange(NZ) + 1.)], axis=1)
    u, v = _uv(real, grid)
    tau = _tau(real, grid)
    f = _make(real, grid, resident, db=db, sverdrup=True)
    _set_tracer(f, tau, resident)
    f.setDepthEdges((numpy.arange(NZ) + 0.5) * h)
    r = _reference(f, sverdrup=True)
    e3 = _broadcast(real, grid, 1, th)
    for carry, nm in ((True, 'tracer_profile'), (False, 'volume_profile')):
        if not carry:
            f.setCellThickness(_on(e3, resident), _on(e3.copy(), resident))
        for t in range(NT):
            M = r.step(array_values({'uo': u, 'vo': v, 'tracer': tau}, t))[nm][1]
            got, P = _dt(f, t, carry), _profile(f, t, carry)
            assert got.shape == (NZ + 2, f._rowlen)
            _check(got[0], 0.5 * P[0], M[0], f'row 0 {nm} t={t}')
            for k in range(1, NZ):
                _check(got[k], 0.5 * P[k - 1] + 0.5 * P[k], M[k - 1] + M[k], f'row {k} {nm} t={t}')
            _check(got[NZ], 0.5 * P[NZ - 1], M[NZ - 1], f'row {NZ} {nm} t={t}')
            assert not got[NZ + 1].view(numpy.uint64).any(), (nm, t)          # exactly +0.0


@pytest.mark.parametrize('band', [(3.0, 12.25), (5.5, 16.5), (0.0, 2.5), (11.0, 13.0), (-4.0, 40.0)], ids=str)
@pytest.mark.parametrize('real', ['float64', 'float32'])
def test_two_edges_give_the_depth_band_flux(real, band):
    """scalar thickness, edges [ztop, zbot]: row 1 is depthBandFlux(profile, ztop, zbot) -- cut levels, levels that end on
    an edge, a band inside one level and one that holds every level"""
    grid, resident = GRIDS[1], True
    ztop, zbot = band
    u, v = _uv(real, grid)
    tau = _tau(real, grid)
    f = _make(real, grid, resident, sverdrup=True)
    _set_tracer(f, tau, resident)
    f.setDepthEdges([ztop, zbot])
    r = _reference(f, sverdrup=True)
    D = _interfaces(TH)
    frac = numpy.clip(numpy.minimum(D[1:], zbot) - numpy.maximum(D[:-1], ztop), 0., None) / TH
    assert frac.max() > 0
    for t in range(NT):
        mags = r.step(array_values({'uo': u, 'vo': v, 'tracer': tau}, t))
        for carry, nm in ((False, 'volume_profile'), (True, 'tracer_profile')):
            got, P = _dt(f, t, carry), _profile(f, t, carry)
            mag = (frac[:, None] * mags[nm][1]).sum(axis=0)
            nseg = f._nseg
            _check(got[1, nseg:], f.depthBandFlux(P[:, nseg:], ztop, zbot), mag[nseg:], f'totals {nm} t={t}')
            _check(got[1, :nseg], f.depthBandFlux(P[:, :nseg], ztop, zbot), mag[:nseg], f'segments {nm} t={t}')


# ---- 7. conservation -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('thick', THICK)
@pytest.mark.parametrize('resident', [True, False], ids=['hbm', 'host'])
@pytest.mark.parametrize('grid', GRIDS, ids=lambda g: f'{g[0]}x{g[1]}')
@pytest.mark.parametrize('real', ['float64', 'float32'])
def test_the_rows_add_up_to_the_profile_rows_and_the_tracer_row(real, grid, resident, thick):
    """the sum over the n + 2 rows against the sum over z of computeFluxProfile under the same thickness, and for the carried
    form against computeTracerFlux, within 1e-12 x the reference's sum |terms|"""
    u, v = _uv(real, grid)
    tau = _tau(real, grid)
    f = _make(real, grid, resident, sverdrup=True)
    arrays = {'uo': u, 'vo': v, 'tracer': tau}
    arrays.update(_set_thickness(f, real, grid, resident, thick))
    _set_tracer(f, tau, resident)
    r = _reference(f, sverdrup=True, cell_thickness=thick != 'scalar')
    for k, (n, edges) in enumerate(EDGES.items()):
        t = k % NT
        f.setDepthEdges(edges)
        mags = r.step(array_values(arrays, t))
        _check(_dt(f, t).sum(axis=0), _rows(f.computeFluxProfile(t)).sum(axis=0), mags['volume'][1], f'volume n={n} t={t}')
        _check(_dt(f, t, True).sum(axis=0), _rows(f.computeTracerFlux(t)), mags['tracer'][1], f'carried n={n} t={t}')


# ---- 8. a depth that is not finite -----------------------------------------------------------------------------------------
@pytest.mark.parametrize('resident', [True, False], ids=['hbm', 'host'])
@pytest.mark.parametrize('real', ['float64', 'float32'])
def test_one_infinite_thickness_sends_its_face_to_the_last_row(real, resident):
    """e3u = +inf at one east face of a line at level 2: the terms of that face at and below level 2 -- the east slot of its
    cell and the west slot of the cell east of it -- go to row n + 1; every other value has the bits of the run in which those
    terms are zero because the velocity is"""
    grid, zinf = GRIDS[0], 2
    nx = grid[0]
    u, v = _uv(real, grid)
    e3u, e3v = _e3(real, grid, NT)
    probe = _make(real, grid, True)
    ce, w, sg = probe.getWeights()
    cells = numpy.unique(ce[ce % 4 == 1] // 4)             # inf x velocity is inf, or NaN where the velocity is 0 or missing
    c = int(cells[cells.size // 2])
    j, i = divmod(c, nx)
    east = c + 1 if i < nx - 1 else c + 1 - nx
    hit = ((ce % 4 == 1) & (ce // 4 == c)) | ((ce % 4 == 3) & (ce // 4 == east))
    segs = numpy.unique(numpy.asarray(sg)[hit])
    cols = numpy.concatenate([segs, [probe._nseg + numpy.searchsorted(probe._tr_off, s, side='right') - 1 for s in segs]])
    cols = numpy.unique(cols)
    bad = e3u.copy()
    bad[:, zinf, j, i] = numpy.inf
    calm = u.copy()
    calm[:, zinf:, j, i] = 0
    a, b = _make(real, grid, resident, sverdrup=True), _make(real, grid, resident, u=calm, sverdrup=True)
    _set_thickness(a, real, grid, resident, 'timevarying', e3=(bad, e3v))
    _set_thickness(b, real, grid, resident, 'timevarying')
    for f in (a, b):
        _set_tracer(f, _tau(real, grid), resident)
        f.setDepthEdges(EDGES[16])
    n = 16
    for t in range(NT):
        for carry in (False, True):
            got, want = _dt(a, t, carry), _dt(b, t, carry)
            assert numpy.array_equal(got[:n + 1], want[:n + 1]) and numpy.isfinite(want).all(), (t, carry)
            assert not want[n + 1].view(numpy.uint64).any()
            last = got[n + 1]
            assert not numpy.isfinite(last[cols]).any(), (t, carry)               # inf x velocity, and whatever lies below
            rest = numpy.delete(last, cols)
            assert not rest.view(numpy.uint64).any(), (t, carry)


# ---- 9. sharding -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('home', ['hbm', 'host'])
@pytest.mark.parametrize('thick', ['scalar', 'timevarying'])
@pytest.mark.parametrize('real', ['float64', 'float32'])
def test_two_sharded_halves_add_up_to_the_unsharded_rows(real, thick, home):
    """slab ranges that cut inside a time step: the running sum of the lower half starts at level 0 all the same -- the
    thickness above the cut is read in place in HBM, staged with the owned levels from the host -- so every term lies where
    the unsharded one does and the halves add up to the unsharded rows up to rounding; every rank's rows are the reference's
    for its levels; a step that a rank does not touch gives exact zeros"""
    from nemoflux_amd.dist import slab_range
    grid, world, resident = GRIDS[1], 2, home == 'hbm'
    u, v = _uv(real, grid)
    tau = _tau(real, grid)
    arrays = {'uo': u, 'vo': v, 'tracer': tau}
    edges = EDGES[1025]

    def make(**kw):
        f = _make(real, grid, resident, **kw)
        arrays.update(_set_thickness(f, real, grid, resident, thick))
        _set_tracer(f, tau, resident)
        f.setDepthEdges(edges)
        return f

    full = make()
    r = _reference(full, cell_thickness=thick != 'scalar')
    want = numpy.array([[_dt(full, t, carry) for carry in (False, True)] for t in range(NT)])
    acc = numpy.zeros_like(want)
    cut_inside = untouched = False
    for rank in range(world):
        sr = slab_range(NT, NZ, rank, world)
        cut_inside = cut_inside or sr[0] % NZ != 0
        part = make(slab_range=sr)
        for t in range(NT):
            z0, z1 = max(sr[0], t * NZ) - t * NZ, min(sr[1], (t + 1) * NZ) - t * NZ
            ref = r.depth_step(array_values(arrays, t), edges, levels=(z0, z1)) if z1 > z0 else None
            for k, (carry, nm) in enumerate(((False, 'volume'), (True, 'carried'))):
                got = _dt(part, t, carry)
                if ref is None:
                    untouched = True
                    assert not got.view(numpy.uint64).any(), (rank, t, carry)
                else:
                    _close(got, *ref[nm], f'rank {rank} levels [{z0}, {z1}) {nm} t={t}')
                acc[t, k] += got
    assert cut_inside and untouched
    for t in range(NT):
        ref = r.depth_step(array_values(arrays, t), edges)
        for k, nm in enumerate(('volume', 'carried')):
            _check(acc[t, k], want[t, k], ref[nm][1], f'two halves, {nm} t={t}')


# ---- 11. refusals, timeMean and fluxplot -----------------------------------------------------------------------------------
def test_the_refusals_have_the_siblings_words():
    from nemoflux_amd._lib import lib
    real, grid = 'float64', GRIDS[0]
    f = _make(real, grid, True)
    for carry in (False, True):
        with pytest.raises(RuntimeError, match='setDepthEdges first'):
            f.computeDepthTransport(0, carry=carry)
    host = numpy.zeros((4, f._rowlen))
    assert lib.nf_field_compute_depth_transport(ctypes.byref(f._h), 0, 0, host.ctypes.data_as(dp)) == 2
    assert 'nf_field_compute_depth_transport: set_depth_edges first' in lib.nf_last_error().decode()
    for bad, words in (([1.], 'need 2 <= nedges'), ([1., 1.], 'strictly increasing'), ([0., numpy.nan], 'finite')):
        with pytest.raises(RuntimeError, match=words):
            f.setDepthEdges(bad)
    with pytest.raises(RuntimeError, match='top must be a finite number'):
        f.setDepthEdges([1., 2.], numpy.inf)
    f.setClassEdges(numpy.array([1., 2., 3.]))                  # another set: the depth call does not see it
    with pytest.raises(RuntimeError, match='setDepthEdges first'):
        f.computeDepthTransport(0)
    f.setDepthEdges(numpy.array([3., 9.]))
    with pytest.raises(RuntimeError, match='setTracer first'):
        f.computeDepthTransport(0, carry=True)
    assert lib.nf_field_compute_depth_transport(ctypes.byref(f._h), 0, 1, host.ctypes.data_as(dp)) == 2
    assert 'nf_field_compute_depth_transport: set_tracer first' in lib.nf_last_error().decode()
    words = lib.nf_last_error().decode()
    gross = numpy.zeros((2 * NZ, f._rowlen))
    assert lib.nf_field_compute_gross_profile(ctypes.byref(f._h), 0, 1, gross.ctypes.data_as(dp)) == 2
    assert words.replace('nf_field_compute_depth_transport', 'nf_field_compute_gross_profile') == lib.nf_last_error().decode()
    assert lib.nf_field_compute_depth_transport(ctypes.byref(f._h), NT, 0, host.ctypes.data_as(dp)) == 1
    assert b'time index' in lib.nf_last_error()
    assert lib.nf_field_compute_depth_transport(ctypes.byref(f._h), 0, 2, host.ctypes.data_as(dp)) == 1
    assert b'carry must be 0 or 1' in lib.nf_last_error() and not host.any()
    assert numpy.abs(_dt(f, 0)).max() > 0
    # the forms that refuse a cell thickness keep refusing it; the depth form takes it
    _set_tracer(f, _tau(real, grid), True)
    _set_thickness(f, real, grid, True, 'static')
    for call in (lambda: f.computeClassTransport(0), lambda: f.computeClassRemap(0), lambda: f.computeTracerProfile(0)):
        with pytest.raises(RuntimeError, match='does not take per-cell thicknesses yet'):
            call()
    assert numpy.abs(_dt(f, 0, True)).max() > 0


@pytest.mark.parametrize('real', ['float64', 'float32'])
def test_time_mean_fields_carry_the_edges_and_give_the_rows_of_a_fresh_field(real):
    """timeMean(thicknessWeighted=True) of a time-varying thickness: the mean Field has the depth edges and `top`, and its rows
    are those of a Field built by hand from the mean Field's own arrays; classStreamfunction takes the rows as they are"""
    from nemoflux_amd.field import Field
    grid = GRIDS[1]
    blon, blat = _case(real, grid)[:2]
    f = _make(real, grid, True, sverdrup=True)
    _set_thickness(f, real, grid, True, 'timevarying')
    _set_tracer(f, _tau(real, grid), True)
    f.setDepthEdges(EDGES[16], -1.5)
    mean = _quiet(f.timeMean, thicknessWeighted=True)
    assert mean.nt == 1 and numpy.array_equal(mean._depth_edges[0], EDGES[16]) and mean._depth_edges[1] == -1.5
    fresh = _field(blon, blat, DB, mean._uv[0], mean._uv[1], [transect_xyz(s) for s in LINES], True, readback=False,
                   fill_value=mean._uv_markers[0])
    fresh.setCellThickness(*mean._e3['arrays'])
    tfill = mean._tracer['fill']
    fresh.setTracer(mean._tracer['keep'], fill_value=None if tfill != tfill else tfill, reference=REF)
    fresh.setDepthEdges(EDGES[16], -1.5)
    for carry in (False, True):
        rows = _dt(mean, 0, carry)
        assert rows.shape == (18, f._rowlen) and numpy.isfinite(rows).all() and (numpy.abs(rows).max(axis=1) > 0).sum() > 8
        assert _same_bits(rows, _dt(fresh, 0, carry)), carry
    tot = mean.computeDepthTransport(0)[0]
    psi = Field.classStreamfunction(tot)
    assert psi.shape == (16, len(LINES)) and numpy.array_equal(psi, numpy.cumsum(tot[:16], axis=0))
    # the plain mean of a Field with a static thickness carries them too
    g = _make(real, grid, True)
    _set_thickness(g, real, grid, True, 'static')
    g.setDepthEdges(EDGES[3])
    m = _quiet(g.timeMean)
    assert numpy.array_equal(m._depth_edges[0], EDGES[3]) and m._depth_edges[1] == 0.0
    assert numpy.abs(_dt(m, 0)).max() > 0


@pytest.mark.parametrize('form', ['volume', 'carried', 'cell'])
def test_fluxplot_depth_bins_is_the_field_table(tmp_path, form):
    from nemoflux_amd import fluxplot
    real, grid = 'float32', GRIDS[0]
    blon, blat = _case(real, grid)[:2]
    u, v = _uv(real, grid)
    tau = _tau(real, grid)
    e3u, e3v = _e3(real, grid, NT)
    paths = {k: str(tmp_path / f'{k}.npz') for k in 'TUV'}
    fv = lambda name, a, b: {f'_FillValue_{name}': numpy.array(a), f'_missing_value_{name}': numpy.array(b)}   # noqa: E731
    numpy.savez(paths['T'], bounds_lon=blon, bounds_lat=blat, deptht_bounds=DB, thetao=tau, **fv('thetao', TFILL, TMISSING))
    numpy.savez(paths['U'], uo=u, e3u=e3u, **fv('uo', FILL, MISSING), **fv('e3u', THFILL, THMISSING))
    numpy.savez(paths['V'], vo=v, e3v=e3v, **fv('vo', FILL, MISSING), **fv('e3v', THFILL, THMISSING))
    edges = EDGES[16]
    lines = '[' + T_OPEN + '],[' + T_SEAM + ']'
    out = str(tmp_path / 'depth.csv')
    kw = dict(tFile=paths['T'], uFile=paths['U'], vFile=paths['V'], depthBins=','.join(repr(float(e)) for e in edges),
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
    mem.setDepthEdges(edges, -1.5)
    with open(out) as fh:
        text = fh.read().splitlines()
    title = '# water flow by depth bin [Sv]' if form == 'volume' else '# transport of thetao by depth bin [thetao x Sv x 0.0041]'
    assert text[0] == title + (', depths from the cell thicknesses' if form == 'cell' else '')
    assert text[1] == 'time,ztop,zbot,line0,line1'
    assert text[2].split(',')[1:3] == ['-inf', '0'] and text[2 + edges.size + 1].split(',')[1:3] == ['nan', 'nan']
    assert totals.shape == (NT, edges.size + 2, 2) and len(text) == 2 + NT * (edges.size + 2)
    for t in range(NT):
        want = mem.computeDepthTransport(t, carry=form != 'volume')[0] * (1.0 if form == 'volume' else 4.1e-3)
        assert _same_bits(totals[t], want) and (numpy.abs(want).max(axis=1) > 0).sum() > 8
        row = numpy.array([float(x) for x in text[2 + t * (edges.size + 2) + 5].split(',')[3:]])
        assert numpy.allclose(row, want[5], rtol=1e-14, atol=0)
