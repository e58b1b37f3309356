"""Gross (inflow / outflow) transports on the GPU (Field.computeGrossProfile, nf_field_compute_gross_profile, fluxplot --gross).
Every value of all four forms -- volume or carried tracer, scalar or per-cell thickness -- is checked against the float64 /
long-double restatement of the definition in tests/gross_reference.py to 1e-12 x sum |c| of that value, no row, level or column
left out; anchored bit for bit (negating uo / vo swaps and negates the parts; tau = ref + 1 gives the volume parts; a broadcast
cell thickness is the scalar form; two sharded halves add up; every chunk length, the asynchronous form and host inputs give the
same bits); P >= 0 >= N in the volume form; P + N against the net rows; nothing else is disturbed and the handle follows its
setters; fluxplot --gross from files.

Grids 72 x 36 x 7 x 3 and 73 x 37 x 7 x 3, float64 and float32, host and HBM inputs, _FillValue, a second marker, NaN and exact
zeros in uo / vo and in the thicknesses, markers and NaN in the tracer, wrapX on and off, Sverdrup on and off, transects open,
closed, across the seam and along row 0.  The inputs keep every non-zero |q| far from underflow (tests/test_gross_cpu.py);
min_abs_q of the reference is asserted wherever a reference is formed.

Measured on an MI355X: see the figures printed by each test; docs/PARITY.md quotes the worst."""
import ctypes

import numpy
import pytest

from conftest import transect_xyz
from gpu_helpers import _field, _on, _quiet, _rows
from gross_reference import MIN_ABS_Q, GrossReference, array_values, gross_thickness, gross_velocities
from test_gpu_cellthick import (BAR, FILL, MISSING, T_OPEN, T_SEAM, T_TRI, TFILL, THFILL, THMISSING, TMISSING, _case, _resident,
                                _row)
from test_gpu_tracer_resolved import H5_LINES, _h5_arrays, _h5_files, _read_csv
from test_gross_cpu import GPU_E3_SEED, GPU_GRIDS as GRIDS, GPU_NT as NT, GPU_NZ as NZ, GPU_UV_SEED

pytestmark = pytest.mark.gpu

EPS = numpy.finfo(numpy.float64).eps
REF = 4.5
T_ROW0 = "(-20,-89),(175,-89)"                # along row 0
T_CROSS = "(150,-40),(210,30)"                # across the seam: the last column and column 0
LINES = [T_OPEN, T_TRI, T_SEAM, T_ROW0, T_CROSS]
# thicknesses >= 0.2 that float32 holds exactly, and bounds whose differences are those numbers exactly
TH = numpy.array([0.25, 0.5, 0.375, 0.75, 1.0, 0.625, 0.25])
DB = numpy.stack([numpy.concatenate([[0.], numpy.cumsum(TH)[:-1]]), numpy.cumsum(TH)], axis=1)
CHUNKS = [('float64', 2), ('float64', 4), ('float64', 8), ('float32', 4), ('float32', 8)]     # every built chunk length
_UV, _E3 = {}, {}
dp = ctypes.POINTER(ctypes.c_double)


def _uv(real, grid):
    if (real, grid) not in _UV:
        _UV[real, grid] = gross_velocities(real, (NT, NZ, grid[1], grid[0]), seed=GPU_UV_SEED)
    return _UV[real, grid]


def _e3(real, grid, nt_th):
    if (real, grid, nt_th) not in _E3:
        _E3[real, grid, nt_th] = gross_thickness(real, (nt_th, NZ, grid[1], grid[0]), seed=GPU_E3_SEED)
    return _E3[real, grid, nt_th]


def _tau(real, grid, seed=3):
    """a tracer around the reference (tf of either sign) with NaN and both markers in it"""
    nx, ny = grid
    dt = numpy.dtype(real).type
    tau = (REF + 2. * numpy.random.default_rng(seed).standard_normal((NT, NZ, ny, nx))).astype(real)
    tau[:, 1::3, 3:-2:3, 2:-2:4] = numpy.nan
    tau[:, :, 10:14, 50:60] = dt(TFILL)
    tau[:, 2:, 25:28, 5:12] = dt(TMISSING)
    return tau


def _make(real, grid, resident, u=None, v=None, lines=LINES, **kw):
    blon, blat, _, _ = _case(real, grid)
    u0, v0 = _uv(real, grid)
    kw.setdefault('readback', False)
    kw.setdefault('fill_value', FILL)
    kw.setdefault('missing_value', MISSING)
    return _field(blon, blat, DB, _on(u0 if u is None else u, resident), _on(v0 if v is None else v, resident),
                  [transect_xyz(s) for s in lines], **kw)


def _set_thickness(f, real, grid, resident, thick):
    """thick: 'scalar' (nothing to set), 'static' or 'timevarying'; returns the arrays for the reference"""
    if thick == 'scalar':
        return {}
    e3u, e3v = _e3(real, grid, NT if thick == 'timevarying' else 1)
    f.setCellThickness(_on(e3u, resident), _on(e3v, resident), fill_value=THFILL, missing_value=THMISSING)
    return dict(e3u=e3u, e3v=e3v)


def _set_tracer(f, tau, resident, ref=REF, wrap=True):
    f.setTracer(_on(tau, resident), fill_value=TFILL, missing_value=TMISSING, reference=ref, wrapX=wrap)


def _gross(f, t, carry=False, **kw):
    """(2, nz, row_length): P, N as [segments | transects] rows"""
    return _rows(f.computeGrossProfile(t, carry=carry, **kw))


def _reference(f, wrap=True, ref=REF, sverdrup=False, cell_thickness=False):
    ce, w, sg = f.getWeights()
    return GrossReference(ce, w, sg, f.arcLengths, f.thickness, f._tr_off, f.nx, f.ny, uv_markers=(FILL, MISSING),
                          tracer_markers=(TFILL, TMISSING), thick_markers=(THFILL, THMISSING), reference=ref, wrap=wrap,
                          sverdrup=sverdrup, cell_thickness=cell_thickness)


def _close(got, pair, label):
    want, mag = pair
    assert got.shape == want.shape, label
    err = numpy.abs(got - want)
    worst = float((err / numpy.maximum(mag, 1e-300)).max())
    print(f'{label}: max |err| / sum |c| = {worst:.3g}')
    assert numpy.all(err <= BAR * mag), (label, worst)


def _chunk(levels):
    from nemoflux_amd._lib import lib
    assert lib.nf_tuning_set(b'gross_chunk', levels) == 0, levels


# ---- 1. against the reference; 3. the signs of the volume form ---------------------------------------------------------------
@pytest.mark.parametrize('thick', ['scalar', 'static', 'timevarying'])
@pytest.mark.parametrize('wrap', [True, False], ids=['wrap-sv', 'nowrap-m2'])
@pytest.mark.parametrize('resident', [True, False], ids=['hbm', 'host'])
@pytest.mark.parametrize('grid', GRIDS, ids=lambda g: f'{g[0]}x{g[1]}')
@pytest.mark.parametrize('real', ['float64', 'float32'])
def test_against_the_reference(real, grid, resident, wrap, thick):
    u, v = _uv(real, grid)
    dt = u.dtype.type
    assert numpy.isnan(v).any() and (u == dt(FILL)).any() and (u == dt(MISSING)).any() and (u == 0).any()
    tau = _tau(real, grid)
    f = _make(real, grid, resident, sverdrup=wrap)
    ce = f.getWeights()[0]
    assert (ce // 4 < f.nx).any() and (ce // 4 % f.nx == 0).any() and (ce // 4 % f.nx == f.nx - 1).any()    # row 0 and the seam
    arrays = {'uo': u, 'vo': v, 'tracer': tau}
    arrays.update(_set_thickness(f, real, grid, resident, thick))
    _set_tracer(f, tau, resident, wrap=wrap)
    r = _reference(f, wrap=wrap, sverdrup=wrap, cell_thickness=thick != 'scalar')
    for t in range(NT):
        want = r.gross_step(array_values(arrays, t))
        assert want['min_abs_q'] >= MIN_ABS_Q
        for part in (0, 1):
            assert want['volume'][1][part][:, -len(LINES):].min() > 0, 'every line must flow both ways on every level'
        vol, car = _gross(f, t), _gross(f, t, carry=True)
        assert vol.shape == car.shape == (2, NZ, f._rowlen)
        _close(vol, want['volume'], f'volume t={t}')
        _close(car, want['carried'], f'carried t={t}')
        assert (vol[0] >= 0).all() and (vol[1] <= 0).all() and (vol[0] > 0).any() and (vol[1] < 0).any()
        assert (car[0] < 0).any() and (car[1] > 0).any()          # split by the water, not by the sign of the carried term


# ---- 2. bit-for-bit identities -------------------------------------------------------------------------------------------
@pytest.mark.parametrize('thick', ['scalar', 'timevarying'])
@pytest.mark.parametrize('resident', [True, False], ids=['hbm', 'host'])
@pytest.mark.parametrize('grid', GRIDS, ids=lambda g: f'{g[0]}x{g[1]}')
@pytest.mark.parametrize('real', ['float64', 'float32'])
def test_negated_velocities_swap_and_negate_the_parts(real, grid, resident, thick):
    u, v = _uv(real, grid)
    dt = u.dtype.type

    def negated(x):
        keep = numpy.isnan(x) | (x == dt(FILL)) | (x == dt(MISSING))
        return numpy.where(keep, x, -x)

    tau = _tau(real, grid)
    a, b = _make(real, grid, resident, sverdrup=True), _make(real, grid, resident, u=negated(u), v=negated(v), sverdrup=True)
    for f in (a, b):
        _set_thickness(f, real, grid, resident, thick)
        _set_tracer(f, tau, resident)
    for t in range(NT):
        for carry in (False, True):
            p, n = _gross(a, t, carry)
            pm, nm = _gross(b, t, carry)
            assert numpy.abs(p).max() > 0 and numpy.abs(n).max() > 0
            assert numpy.array_equal(pm, -n) and numpy.array_equal(nm, -p), (t, carry)


@pytest.mark.parametrize('thick', ['scalar', 'timevarying'])
@pytest.mark.parametrize('resident', [True, False], ids=['hbm', 'host'])
@pytest.mark.parametrize('grid', GRIDS, ids=lambda g: f'{g[0]}x{g[1]}')
@pytest.mark.parametrize('real', ['float64', 'float32'])
def test_tracer_one_above_the_reference_is_carried_like_the_water(real, grid, resident, thick):
    """tau == ref + 1 everywhere, ref an integer != 0: tf == 1 exactly at every face that has a value, so the carried parts are
    the volume parts bit for bit.  With wrapX only the north faces of the last row have no value, and no line comes near it."""
    nx, ny = grid
    tau = numpy.full((NT, NZ, ny, nx), 8., real)
    f = _make(real, grid, resident)
    assert (f.getWeights()[0] // 4 // nx).max() < ny - 1
    _set_thickness(f, real, grid, resident, thick)
    _set_tracer(f, tau, resident, ref=7.0)
    for t in range(NT):
        vol = _gross(f, t)
        assert numpy.abs(vol[0]).max() > 0 and numpy.abs(vol[1]).max() > 0
        assert numpy.array_equal(_gross(f, t, carry=True), vol), t
    _set_tracer(f, tau, resident, ref=6.0)                 # tf == 2: exactly twice
    assert numpy.array_equal(_gross(f, 1, carry=True), 2. * _gross(f, 1))


@pytest.mark.parametrize('nt_th', [1, NT], ids=['static', 'timevarying'])
@pytest.mark.parametrize('resident', [True, False], ids=['hbm', 'host'])
@pytest.mark.parametrize('grid', GRIDS, ids=lambda g: f'{g[0]}x{g[1]}')
@pytest.mark.parametrize('real', ['float64', 'float32'])
def test_broadcast_cell_thickness_is_the_scalar_form(real, grid, resident, nt_th):
    nx, ny = grid
    tau = _tau(real, grid)
    a, b = _make(real, grid, resident), _make(real, grid, resident)
    e3 = numpy.ascontiguousarray(numpy.broadcast_to(TH.astype(real)[None, :, None, None], (nt_th, NZ, ny, nx)))
    a.setCellThickness(_on(e3, resident), _on(e3.copy(), resident))
    for f in (a, b):
        _set_tracer(f, tau, resident)
    for t in (1, 0, 2):
        for carry in (False, True):
            want = _gross(b, t, carry)
            assert numpy.abs(want).max() > 0
            assert numpy.array_equal(_gross(a, t, carry), want), (t, carry)
    a.setCellThickness(_on(2 * e3, resident), _on(e3, resident))
    assert not numpy.array_equal(_gross(a, 1), _gross(b, 1))
    a.setCellThickness(None, None)
    assert numpy.array_equal(_gross(a, 1, True), _gross(b, 1, True))


@pytest.mark.parametrize('thick', ['scalar', 'timevarying'])
@pytest.mark.parametrize('resident', [True, False], ids=['hbm', 'host'])
@pytest.mark.parametrize('real', ['float64', 'float32'])
def test_two_sharded_halves_add_up_to_the_unsharded_rows(real, resident, thick):
    """slab ranges that cut inside a time step: every level belongs to one rank, the other gives exact zeros, so the sum of the
    two ranks' rows is the unsharded block bit for bit"""
    from nemoflux_amd.dist import slab_range
    grid, world = GRIDS[1], 2
    tau = _tau(real, grid)

    def make(**kw):
        f = _make(real, grid, resident, **kw)
        _set_thickness(f, real, grid, resident, thick)
        _set_tracer(f, tau, resident)
        return f

    full = make()
    want = numpy.array([[_gross(full, t, carry) for carry in (False, True)] for t in range(NT)])
    acc = numpy.zeros_like(want)
    cut_inside = False
    for rank in range(world):
        sr = slab_range(NT, NZ, rank, world)
        cut_inside = cut_inside or sr[0] % NZ != 0
        part = make(slab_range=sr)
        for t in range(NT):
            own = numpy.zeros(NZ, bool)
            lo, hi = max(sr[0], t * NZ), min(sr[1], (t + 1) * NZ)
            if hi > lo:
                own[lo - t * NZ:hi - t * NZ] = True
            for k, carry in enumerate((False, True)):
                got = _gross(part, t, carry)
                assert numpy.all(got[:, ~own] == 0), (rank, t, carry)
                assert numpy.array_equal(got[:, own], want[t, k][:, own]), (rank, t, carry)
                acc[t, k] += got
    assert cut_inside and numpy.abs(want).max() > 0
    assert numpy.array_equal(acc, want)


@pytest.mark.parametrize('thick', ['scalar', 'static'])
@pytest.mark.parametrize('real', ['float64', 'float32'])
def test_out_and_host_forms_give_the_same_bits(real, thick):
    import torch
    grid = GRIDS[1]
    tau = _tau(real, grid)
    fields = []
    for resident in (True, False):
        f = _make(real, grid, resident)
        _set_thickness(f, real, grid, resident, thick)
        _set_tracer(f, tau, resident)
        fields.append(f)
    f, host = fields
    shape = (2 * NZ, f._rowlen)
    for t in (2, 0):
        for carry in (False, True):
            want = _gross(f, t, carry)
            out = torch.full(shape, numpy.nan, dtype=torch.float64, device='cuda')
            assert numpy.array_equal(_gross(f, t, carry, out=out), want) and numpy.abs(want).max() > 0
            assert numpy.array_equal(out.cpu().numpy().reshape(want.shape), want)
            assert numpy.array_equal(_gross(host, t, carry), want)             # host-resident inputs, staged
            out.fill_(numpy.nan)
            assert numpy.array_equal(_gross(host, t, carry, out=out), want)
    for bad in (torch.zeros(shape, dtype=torch.float32, device='cuda'), torch.zeros((2 * NZ + 1, f._rowlen), dtype=torch.float64,
                                                                                  device='cuda'),
                torch.zeros((2, NZ, f._rowlen), dtype=torch.float64, device='cuda'), torch.zeros(shape, dtype=torch.float64),
                torch.zeros((f._rowlen, 2 * NZ), dtype=torch.float64, device='cuda').t()):
        with pytest.raises(RuntimeError, match='out must be'):
            f.computeGrossProfile(0, out=bad)


@pytest.mark.parametrize('thick', ['scalar', 'timevarying'])
@pytest.mark.parametrize('grid', GRIDS, ids=lambda g: f'{g[0]}x{g[1]}')
@pytest.mark.parametrize('real,chunk', CHUNKS)
def test_every_built_chunk_gives_the_default_bits_and_meets_the_reference(real, chunk, grid, thick):
    """the levels of a chunk do not meet before the rows are written: the chunk length changes no bit.  nz = 7 leaves the last
    chunk partial for every length."""
    from nemoflux_amd._lib import lib
    u, v = _uv(real, grid)
    tau = _tau(real, grid)
    f = _make(real, grid, True, sverdrup=True)
    arrays = {'uo': u, 'vo': v, 'tracer': tau}
    arrays.update(_set_thickness(f, real, grid, True, thick))
    _set_tracer(f, tau, True)
    t = 1
    default = [_gross(f, t, carry) for carry in (False, True)]
    want = _reference(f, sverdrup=True, cell_thickness=thick != 'scalar').gross_step(array_values(arrays, t))
    assert want['min_abs_q'] >= MIN_ABS_Q
    try:
        _chunk(chunk)
        for carry, nm in ((False, 'volume'), (True, 'carried')):
            got = _gross(f, t, carry)
            _close(got, want[nm], f'{nm} chunk={chunk}')
            assert numpy.array_equal(got, default[int(carry)]), (nm, chunk)
        if real == 'float32':        # a chunk that is not built for the dtype is an error, not another kernel
            _chunk(2)
            with pytest.raises(RuntimeError, match='gross_chunk'):
                f.computeGrossProfile(t)
    finally:
        _chunk(0)
    assert lib.nf_tuning_set(b'gross_chunk', 3) != 0
    assert numpy.array_equal(_gross(f, t), default[0])


# ---- 4. P + N against the net rows -------------------------------------------------------------------------------------------
@pytest.mark.parametrize('resident', [True, False], ids=['hbm', 'host'])
@pytest.mark.parametrize('grid', GRIDS, ids=lambda g: f'{g[0]}x{g[1]}')
@pytest.mark.parametrize('real', ['float64', 'float32'])
def test_the_parts_add_up_to_the_net_rows(real, grid, resident):
    """P + N against computeFluxProfile and computeTracerProfile (scalar thickness, then the volume profile with a cell
    thickness) per level, and against computeTracerFlux summed over z with a cell thickness: within 1e-12 x the reference's
    sum |c| of the two parts together"""
    u, v = _uv(real, grid)
    tau = _tau(real, grid)
    f = _make(real, grid, resident, sverdrup=True)
    _set_tracer(f, tau, resident)
    arrays = {'uo': u, 'vo': v, 'tracer': tau}

    def check(got, net, mag, label):
        err = numpy.abs(got - net)
        worst = float((err / numpy.maximum(mag, 1e-300)).max())
        print(f'{label}: max |P + N - net| / sum |c| = {worst:.3g}')
        assert net.shape == got.shape and numpy.abs(net).max() > 0 and numpy.all(err <= BAR * mag), (label, worst)

    r = _reference(f, sverdrup=True)
    for t in range(NT):
        want = r.gross_step(array_values(arrays, t))
        assert want['min_abs_q'] >= MIN_ABS_Q
        vol, car = _gross(f, t), _gross(f, t, carry=True)
        check(vol[0] + vol[1], _rows(f.computeFluxProfile(t)), want['volume'][1].sum(axis=0), f'volume t={t}')
        check(car[0] + car[1], _rows(f.computeTracerProfile(t)), want['carried'][1].sum(axis=0), f'carried t={t}')
    arrays.update(_set_thickness(f, real, grid, resident, 'timevarying'))
    r = _reference(f, sverdrup=True, cell_thickness=True)
    for t in range(NT):
        want = r.gross_step(array_values(arrays, t))
        assert want['min_abs_q'] >= MIN_ABS_Q
        vol, car = _gross(f, t), _gross(f, t, carry=True)
        check(vol[0] + vol[1], _rows(f.computeFluxProfile(t)), want['volume'][1].sum(axis=0), f'volume, cell thickness t={t}')
        check((car[0] + car[1]).sum(axis=0), _rows(f.computeTracerFlux(t)), want['carried'][1].sum(axis=(0, 1)),
              f'carried, cell thickness, summed over z t={t}')
        with pytest.raises(RuntimeError, match='per-cell thicknesses'):       # the net form still takes none
            f.computeTracerProfile(t)


# ---- 5. state ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('compact', [False, True], ids=['full', 'compact'])
@pytest.mark.parametrize('thick', ['scalar', 'timevarying'])
@pytest.mark.parametrize('resident', [True, False], ids=['hbm', 'host'])
def test_the_gross_profile_leaves_everything_else_alone(resident, thick, compact):
    real, grid = 'float64', GRIDS[0]
    a, b = _make(real, grid, resident, compact=compact), _make(real, grid, resident, compact=compact)
    tau = _tau(real, grid)
    for f in (a, b):
        _set_thickness(f, real, grid, resident, thick)
        _set_tracer(f, tau, resident)
    want_all, want_tr = _rows(b.computeAll()), _rows(b.computeTracerAll())
    gross1 = _gross(a, 1, True)
    for t in (1, 0, 2):
        assert a.computeFlux(t) == b.computeFlux(t)
        tr = _rows(a.computeTracerFlux(t))
        planes = _resident(a)
        _gross(a, (t + 1) % NT), _gross(a, t, True), _gross(a, t)
        assert numpy.array_equal(_row(a), _row(b)) and numpy.array_equal(_row(a), want_all[t])
        for k, (x, y, z) in enumerate(zip(_resident(a), planes, _resident(b))):
            assert numpy.array_equal(x, y), (t, k)
            assert k == 3 or numpy.array_equal(x, z), (t, k)        # (b's running max has seen every step)
        assert numpy.array_equal(_rows(a.computeTracerFlux(t)), tr) and numpy.array_equal(tr, want_tr[t])
        assert a.computeFlux(t) == b.computeFlux(t)
    _gross(a, 0)
    assert numpy.array_equal(_rows(a.computeAll()), want_all)
    _gross(a, 2, True)
    assert numpy.array_equal(_rows(a.computeAll()), want_all)           # a replayed pass where there is one
    assert numpy.array_equal(_rows(a.computeTracerAll()), want_tr)
    assert numpy.array_equal(_gross(a, 1, True), gross1)


def _handle(ny, nx, nz, u, v, lines, on_device):
    from test_gpu_reuse_products import ProductHandle
    h = ProductHandle()
    h.set_bounds(ny, nx, numpy.float64, False)
    h.set_thickness(numpy.linspace(0.25, 1.0, nz))
    h.set_uv(u, v, on_device, FILL)
    for ln in lines:
        h.add_transect(ln)
    h.call('build_weights', 16, 360.)
    return h


def _handle_gross(h, t, carry, nz):
    rows = numpy.full((2, nz, h.rowlen()), numpy.nan)
    rc = h.raw('compute_gross_profile', t, carry, rows.ctypes.data_as(dp))
    return rc, rows


@pytest.mark.parametrize('on_device', [True, False], ids=['hbm', 'host'])
def test_one_handle_follows_its_setters(on_device):
    """a second set_tracer, a cleared and re-set cell thickness and one more transect with build_weights each show in the next
    gross call on the same handle: the rows of a fresh handle given only the final state, bit for bit.  A static host thickness
    that the handle uploaded is refused after a set_bounds of another shape."""
    from test_gpu_reuse import TRANSECTS
    ny, nx, nz, nt = 24, 40, 7, 2
    shape = (nt, nz, ny, nx)
    u, v = gross_velocities('float64', shape, seed=17)
    rng = numpy.random.default_rng(19)
    tau_a, tau_b = 3. + rng.standard_normal(shape), 5. + rng.standard_normal(shape)
    e3_a, e3_b = gross_thickness('float64', (1,) + shape[1:], seed=23), gross_thickness('float64', shape, seed=29)

    def fresh(tau, e3, lines, carry, t=1):
        f = _handle(ny, nx, nz, u, v, lines, on_device)
        if tau is not None:
            f.set_tracer(tau, on_device, None)
        if e3 is not None:
            f.set_cell_thickness(e3[0], e3[1], on_device, THFILL)
        rc, rows = _handle_gross(f, t, carry, nz)
        assert rc == 0
        return rows

    h = _handle(ny, nx, nz, u, v, TRANSECTS[:2], on_device)
    rc, _ = _handle_gross(h, 1, 1, nz)
    assert rc == 2 and b'set_tracer first' in h.lib.nf_last_error()                      # carried form, no tracer yet
    seen = []

    def step(tau, e3, lines, carry):
        rc, got = _handle_gross(h, 1, carry, nz)
        assert rc == 0 and numpy.abs(got).max() > 0
        assert numpy.array_equal(got, fresh(tau, e3, lines, carry)), (len(seen), carry)
        assert all(got.shape != s.shape or not numpy.array_equal(got, s) for s in seen[-1:] if carry), len(seen)
        if carry:
            seen.append(got)

    for carry in (0, 1):
        if carry:
            h.set_tracer(tau_a, on_device, None)
        step(tau_a, None, TRANSECTS[:2], carry)
    h.set_tracer(tau_b, on_device, None)                                                   # a second set_tracer
    step(tau_b, None, TRANSECTS[:2], 1)
    h.set_cell_thickness(e3_a[0], e3_a[1], on_device, THFILL)                              # a static cell thickness
    for carry in (0, 1):
        step(tau_b, e3_a, TRANSECTS[:2], carry)
    h.set_cell_thickness(None, None, on_device, None)                                      # cleared
    step(tau_b, None, TRANSECTS[:2], 1)
    h.set_cell_thickness(e3_b[0], e3_b[1], on_device, THFILL)                              # and set again, time-varying
    step(tau_b, e3_b, TRANSECTS[:2], 1)
    h.add_transect(TRANSECTS[3])                                                           # one more transect
    rc, _ = _handle_gross(h, 1, 0, nz)
    assert rc == 2 and b'build_weights' in h.lib.nf_last_error()
    h.call('build_weights', 16, 360.)
    for carry in (0, 1):
        step(tau_b, e3_b, TRANSECTS[:2] + [TRANSECTS[3]], carry)
    if not on_device:                                                                      # an upload of the old shape
        h.set_cell_thickness(e3_a[0], e3_a[1], False, THFILL)
        step(tau_b, e3_a, TRANSECTS[:2] + [TRANSECTS[3]], 0)
        h.set_bounds(10, 20, numpy.float64, False)
        u2, v2 = gross_velocities('float64', (nt, nz, 10, 20), seed=31)
        h.set_uv(u2, v2, False, FILL)
        h.call('build_weights', 16, 360.)
        rc, rows = _handle_gross(h, 1, 0, nz)
        assert rc == 2 and b'uploaded for' in h.lib.nf_last_error() and b'compute_gross_profile' in h.lib.nf_last_error()
        assert numpy.isnan(rows).all()
        h.set_cell_thickness(None, None, False, None)
        rc, rows = _handle_gross(h, 1, 0, nz)
        assert rc == 0 and numpy.abs(rows).max() > 0


def test_time_index_and_carry_are_checked():
    from nemoflux_amd._lib import lib
    f = _make('float64', GRIDS[0], True)
    with pytest.raises(RuntimeError, match='setTracer first'):
        f.computeGrossProfile(0, carry=True)
    host = numpy.zeros((2, NZ, f._rowlen))
    assert lib.nf_field_compute_gross_profile(ctypes.byref(f._h), NT, 0, host.ctypes.data_as(dp)) == 1
    assert b'time index' in lib.nf_last_error()
    assert lib.nf_field_compute_gross_profile(ctypes.byref(f._h), 0, 2, host.ctypes.data_as(dp)) == 1
    assert b'carry must be 0 or 1' in lib.nf_last_error() and not host.any()
    assert numpy.abs(_gross(f, 0)).max() > 0


# ---- 6. files and the command line -----------------------------------------------------------------------------------------
def test_fluxplot_gross_is_the_field_table(tmp_path):
    """fluxplot --gross on the HDF5 files, alone and with a tracer from an .npz bundle, a depth band and cell thicknesses from
    another bundle: the numbers of the in-memory Field, bit for bit in the returned array and to 15 digits in the CSV"""
    from nemoflux_amd import fluxplot
    from nemoflux_amd.field import Field
    files = _h5_files()
    blon, blat, db, u, v, ufill, vfill = _h5_arrays()
    nt, nz, ny, nx = u.shape
    rng = numpy.random.default_rng(83)
    tau = (2. + rng.random(u.shape) * 4.).astype(u.dtype)
    tpath = str(tmp_path / 'tracer.npz')
    numpy.savez(tpath, thetao=tau)
    e3u, e3v = (rng.uniform(0.5, 2., u.shape).astype(u.dtype) for _ in range(2))
    epath = str(tmp_path / 'e3.npz')
    numpy.savez(epath, e3u=e3u, e3v=e3v)
    lines = fluxplot.readTargets(H5_LINES)[0]
    zband = (float(db.min()) + 0.25 * float(db.max() - db.min()), float(db.max()))
    for tracer, band, cell in ((False, False, False), (True, False, False), (True, True, True), (False, True, False)):
        mem = _field(blon, blat, db, u, v, lines, True, fill_value=ufill, readback=False)
        if cell:
            mem.setCellThickness(e3u, e3v)
        if tracer:
            mem.setTracer(tau, reference=1.5)
        out = str(tmp_path / f'gross{int(tracer)}{int(band)}{int(cell)}.csv')
        kw = dict(cellThickness=True, e3FileU=epath, e3FileV=epath) if cell else {}
        if tracer:
            kw.update(tracer='thetao', tracerFile=tpath, tracerRef=1.5, tracerScale=4.1e-3)
        if band:
            kw.update(zrange=f'{zband[0]!r},{zband[1]!r}')
        got = _quiet(fluxplot.main, lonLatPoints=H5_LINES, output=out, sverdrup=True, gross=True, **kw, **files)
        ncol = 7 if tracer else 3
        assert got.shape == (nt, 2, ncol)
        title, header, body = _read_csv(out)
        assert title.startswith('# gross water flow [Sv]') and (('thetao x Sv x 0.0041' in title) == tracer)
        assert ('between the depths' in title) == band
        assert header == 'time,transect,inflow,outflow,net' + (',carried_in,carried_out,mean_in,mean_out' if tracer else '')
        assert len(body) == nt * 2
        bkw = dict(ztop=zband[0], zbot=zband[1], bounds_depth=mem.bounds_depth) if band else {}
        for t in range(nt):
            vol = Field.grossTransport(mem.computeGrossProfile(t)[0], **bkw)
            assert numpy.array_equal(got[t, :, 0], vol[0]) and numpy.array_equal(got[t, :, 1], vol[1])
            assert numpy.array_equal(got[t, :, 2], vol[0] + vol[1])
            assert (vol[0] >= 0).all() and (vol[1] <= 0).all() and (vol[0] - vol[1] > 0).all()
            if tracer:
                car = Field.grossTransport(mem.computeGrossProfile(t, carry=True)[0], **bkw)
                assert numpy.array_equal(got[t, :, 3], car[0] * 4.1e-3) and numpy.array_equal(got[t, :, 4], car[1] * 4.1e-3)
                assert numpy.array_equal(got[t, :, 5:].T, Field.transportWeightedTracer(vol, car, 1.5))
                m = got[t, :, 5:]
                assert (numpy.isnan(m) | ((m > 2.) & (m < 6.))).all() and not numpy.isnan(m).all()    # a mean of values in [2, 6)
            for p in range(2):
                ln = body[t * 2 + p]
                assert ln[1] == f'line{p}'
                assert numpy.allclose([float(x) for x in ln[2:]], got[t, p], rtol=1e-14, atol=1e-300)
        if not band and not tracer:
            net = mem.computeAll()[0]
            assert numpy.all(numpy.abs(got[:, :, 2] - net) <= 1e-12 * (got[:, :, 0] - got[:, :, 1]))
