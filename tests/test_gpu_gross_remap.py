"""Remapped gross class transports on the GPU (Field.computeGrossClassRemap, nf_field_compute_gross_class_remap, fluxplot
--gross-remap linear).  Every value of P and N in all six forms -- volume, carried tracer that is the class field, carried tracer
with a class field of its own, each with the scalar or a per-cell thickness -- is checked against the float64 / long-double
restatement in tests/gross_remap_reference.py to 1e-12 x sum |share| of that value (the A7 bar of docs/PARITY.md), no row or
column left out; anchored bit for bit (a class field constant in z gives the parts of computeGrossClassTransport; the level index
with edges at the half-integers gives the parts of computeGrossProfile; negated uo, vo swap and negate the parts, doubled ones
double them; tau = ref + 1 gives the volume parts; a broadcast cell thickness gives the scalar rows; every class_window, out= and
host inputs give the same bits; a Sigma class field equals its series held as an array); tied to code that shares nothing with
the kernel's row rule (P + N against computeClassRemap, the sums over the rows against the sums over z of computeGrossProfile,
the closed form of tests/test_gpu_class_remap.py on the gross profile's parts); two sharded halves; re-use of one handle;
meanEddySplit; fluxplot from files.

Grids 72 x 36 x 7 x 3 and 73 x 37 x 7 x 3 with the three transects of the sibling tests (one across the periodic seam); the
class-field lattice of tests/test_gpu_class_remap.py and the thickness lattice of tests/test_gpu_depth_remap.py:
tests/test_gross_remap_cpu.py says which branches they take.

The eddy split.  P and N are not linear in (uo, vo): a face whose water changes direction in time gives its mean-state term to
one part and its steps' terms to both.  The split is therefore checked where it can close -- velocities whose sign at every face
is the same at every step (magnitudes, zeros and markers vary), for which the terms of the mean state are the means of the
steps' terms -- in every value of P and N; and with the sign-changing velocities of the other tests for P + N, which is linear."""
import contextlib
import ctypes

import numpy
import pytest

from depth_remap_reference import depth_thickness
from gpu_helpers import _field, _on, _quiet, _rows, _same_bits
from gross_reference import array_values, gross_velocities
from gross_remap_reference import GPU_EDGES as EDGES, GPU_LINES, SFILL, SMISSING, GrossRemapReference, remap_lattice
from test_gpu_cellthick import BAR, FILL, MISSING, T_OPEN, T_SEAM, T_TRI, TFILL, THFILL, THMISSING, TMISSING, _case
from test_gpu_class_remap import _configure, _lattice as _sibling_lattice, _level_field, _make, _window
from test_gpu_depth_remap import _set_thickness
from test_gpu_gross import DB, GRIDS, NT, NZ, REF, TH, _tau, _uv

pytestmark = pytest.mark.gpu

THICK = ['scalar', 'static', 'timevarying']
dp = ctypes.POINTER(ctypes.c_double)
WORST = {'reference': 0.0}


def _gr(f, t, carry=False, **kw):
    """(2, nedges + 2, row_length): P, N as [segments | transects] rows"""
    return _rows(f.computeGrossClassRemap(t, carry=carry, **kw))


def _gc(f, t, carry=False):
    return _rows(f.computeGrossClassTransport(t, carry=carry))


def _gp(f, t, carry=False):
    return _rows(f.computeGrossProfile(t, carry=carry))


def _reference(f, class_markers, wrap=True, ref=REF, sverdrup=False, cell=False):
    ce, w, sg = f.getWeights()
    return GrossRemapReference(ce, w, sg, f.arcLengths, f.thickness, f._tr_off, f.nx, f.ny, uv_markers=(FILL, MISSING),
                               tracer_markers=(TFILL, TMISSING), class_markers=class_markers, thick_markers=(THFILL, THMISSING),
                               reference=ref, wrap=wrap, sverdrup=sverdrup, cell_thickness=cell)


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


def _thick(f, real, grid, resident, thick):
    """the thickness lattice of the depth-bin tests, or none; returns the arrays for the reference"""
    if thick == 'scalar':
        f.setCellThickness(None, None)
        return {}
    return _set_thickness(f, real, grid, resident, thick)


def test_the_inputs_are_the_siblings():
    assert GPU_LINES == [T_OPEN, T_TRI, T_SEAM]
    for real in ('float64', 'float32'):
        for own in (False, True):
            nx, ny = GRIDS[1]
            mine = remap_lattice(real, (NT, NZ, ny, nx), own, (TFILL, TMISSING))
            assert _same_bits(mine.astype(numpy.float64), _sibling_lattice(real, GRIDS[1], own).astype(numpy.float64))


# ---- 1. against the reference ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize('wrap', [True, False], ids=['wrap-sv', 'nowrap-m2'])
@pytest.mark.parametrize('resident', [True, False], ids=['hbm', 'host'])
@pytest.mark.parametrize('grid', GRIDS, ids=lambda g: f'{g[0]}x{g[1]}')
@pytest.mark.parametrize('real', ['float64', 'float32'])
def test_against_the_reference(real, grid, resident, wrap):
    """all six forms; every edge count, each on one of the steps; the thickness (scalar, static, time-varying) goes round with
    the edge count, the form and the case, so that every form meets every thickness and every edge count in the matrix"""
    u, v = _uv(real, grid)
    shift = GRIDS.index(grid) + int(resident) + int(wrap)
    seen = set()
    for two in (False, True):
        f = _make(real, grid, resident, sverdrup=wrap)
        arrays = {'uo': u, 'vo': v}
        more, class_markers = _configure(f, real, grid, resident, two, wrap=wrap)
        arrays.update(more)
        for k, (n, edges) in enumerate(EDGES.items()):
            t = k % NT
            thick = THICK[(k + shift + two) % 3]
            seen.add(thick)
            a = dict(arrays, **_thick(f, real, grid, resident, thick))
            r = _reference(f, class_markers, wrap=wrap, sverdrup=wrap, cell=thick != 'scalar')
            f.setClassEdges(edges)
            want = r.gross_remap_step(array_values(a, t), edges)
            vol, car = _gr(f, t), _gr(f, t, carry=True)
            assert vol.shape == car.shape == (2, n + 2, f._rowlen)
            label = f'{"two" if two else "one"} {thick} n={n} t={t}'
            for got, nm in ((vol, 'volume'), (car, 'carried')):
                WORST['reference'] = max(WORST['reference'], _close(got, *want[nm], f'{nm} {label}'))
            assert numpy.all(vol[0] >= 0) and numpy.all(vol[1] <= 0) and vol[0].max() > 0 and vol[1].min() < 0
            assert want['min_abs_q'] >= 1e-200 and want['spread_terms'] > 100
            assert want['volume'][1][:, n + 1].max() > 0 or not two, 'the row of the faces without a class value has terms'
    assert len(seen) == 3
    print(f'worst so far against the reference: {WORST["reference"]:.3g}')


# ---- 2. bit-for-bit identities ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize('thick', THICK)
@pytest.mark.parametrize('grid', GRIDS, ids=lambda g: f'{g[0]}x{g[1]}')
@pytest.mark.parametrize('real', ['float64', 'float32'])
def test_a_class_field_constant_in_z_gives_the_gross_class_rows(real, grid, thick):
    """g_up == g_dn == f_z exactly, or the face has no value at any level: every term goes whole to the row the step rule sends
    it to, in the order of the gross class transport's bins"""
    resident = thick != 'static'
    for two in (False, True):
        lat = _sibling_lattice(real, grid, two)
        flat = numpy.ascontiguousarray(numpy.broadcast_to(lat[:, 2:3], lat.shape))
        f = _make(real, grid, resident, sverdrup=True)
        if two:
            f.setTracer(_on(_tau(real, grid), resident), fill_value=TFILL, missing_value=TMISSING, reference=REF)
            f.setClassTracer(_on(flat, resident), fill_value=SFILL, missing_value=SMISSING)
        else:
            f.setTracer(_on(flat, resident), fill_value=TFILL, missing_value=TMISSING, reference=REF)
        _thick(f, real, grid, resident, thick)
        for n in (3, 1025):
            f.setClassEdges(EDGES[n])
            t = n % NT
            for carry in (False, True):
                want = _gc(f, t, carry)
                assert (numpy.abs(want[0]).max(axis=1) > 0).sum() >= 3 and (numpy.abs(want[1]).max(axis=1) > 0).sum() >= 3
                assert numpy.array_equal(_gr(f, t, carry), want), (two, n, t, carry)


@pytest.mark.parametrize('thick', THICK)
@pytest.mark.parametrize('grid', GRIDS, ids=lambda g: f'{g[0]}x{g[1]}')
@pytest.mark.parametrize('real', ['float64', 'float32'])
def test_one_class_per_level_gives_the_gross_profile(real, grid, thick):
    """class field = level index, edges at the half-integers: row z + 1 of a part holds exactly the terms of level z of that
    part, added in the order of the gross profile's kernel"""
    resident = thick != 'timevarying'
    level = _level_field(real, grid)
    f = _make(real, grid, resident, sverdrup=True)
    f.setClassEdges(numpy.arange(NZ + 1) - 0.5)
    f.setTracer(_on(_tau(real, grid), resident), fill_value=TFILL, missing_value=TMISSING, reference=REF)
    f.setClassTracer(_on(level, resident))
    _thick(f, real, grid, resident, thick)
    for two in (True, False):
        if not two:
            f.setClassTracer(None)
            f.setTracer(_on(level, resident), reference=2.0)
        for t in range(NT):
            for carry in (False, True):
                got, want = _gr(f, t, carry), _gp(f, t, carry)
                assert got.shape == (2, NZ + 3, f._rowlen) and (numpy.abs(want).max(axis=2) > 0).sum() >= 2 * (NZ - 1)
                assert numpy.array_equal(got[:, 1:NZ + 1], want), (two, t, carry)
                assert not got[:, [0, NZ + 1, NZ + 2]].any()


@pytest.mark.parametrize('thick', ['scalar', 'timevarying'])
@pytest.mark.parametrize('grid', GRIDS, ids=lambda g: f'{g[0]}x{g[1]}')
@pytest.mark.parametrize('real', ['float64', 'float32'])
def test_negated_velocities_swap_and_negate_the_parts_and_doubled_ones_double_them(real, grid, thick):
    resident = grid == GRIDS[0]
    u, v = _uv(real, grid)
    dt = u.dtype.type

    def scaled(x, s):
        keep = numpy.isnan(x) | (x == dt(FILL)) | (x == dt(MISSING))
        return numpy.where(keep, x, dt(s) * x)

    for two in (False, True):
        fields = [_make(real, grid, resident, sverdrup=True)]
        fields += [_make(real, grid, resident, u=scaled(u, s), v=scaled(v, s), sverdrup=True) for s in (-1., 2.)]
        for f in fields:
            _configure(f, real, grid, resident, two)
            _thick(f, real, grid, resident, thick)
            f.setClassEdges(EDGES[1025])
        a, neg, dbl = fields
        t = int(two)
        for carry in (False, True):
            rows = _gr(a, t, carry)
            assert (numpy.abs(rows[0]).max(axis=1) > 0).sum() > 500 and (numpy.abs(rows[1]).max(axis=1) > 0).sum() > 500
            assert numpy.array_equal(_gr(neg, t, carry), -rows[::-1]), (two, t, carry)          # P' = -N, N' = -P
            assert numpy.array_equal(_gr(dbl, t, carry), 2. * rows), (two, t, carry)


@pytest.mark.parametrize('thick', ['scalar', 'static'])
@pytest.mark.parametrize('real', ['float64', 'float32'])
def test_tracer_one_above_the_reference_is_carried_like_the_water(real, thick):
    """tau == ref + 1 everywhere: tf == 1 exactly at every face that has a value, so the carried parts are the volume parts"""
    grid, resident = GRIDS[1], thick == 'scalar'
    nx, ny = grid
    tau = numpy.full((NT, NZ, ny, nx), 8., real)
    f = _make(real, grid, resident)
    assert (f.getWeights()[0] // 4 // nx).max() < ny - 1
    f.setTracer(_on(tau, resident), reference=7.0)
    f.setClassTracer(_on(_sibling_lattice(real, grid, True), resident), fill_value=SFILL, missing_value=SMISSING)
    f.setClassEdges(EDGES[1025])
    _thick(f, real, grid, resident, thick)
    for t in range(NT):
        vol = _gr(f, t)
        assert (numpy.abs(vol).max(axis=2) > 0).sum() > 1000
        assert numpy.array_equal(_gr(f, t, carry=True), vol), t
    f.setTracer(_on(tau, resident), reference=6.0)                 # tf == 2: exactly twice
    assert numpy.array_equal(_gr(f, 1, carry=True), 2. * _gr(f, 1))


@pytest.mark.parametrize('nt_th', [1, NT], ids=['static', 'timevarying'])
@pytest.mark.parametrize('real', ['float64', 'float32'])
def test_broadcast_cell_thickness_is_the_scalar_form(real, nt_th):
    grid, resident = GRIDS[0], nt_th == 1
    nx, ny = grid
    for two in (False, True):
        a, b = _make(real, grid, resident, sverdrup=True), _make(real, grid, resident, sverdrup=True)
        for f in (a, b):
            _configure(f, real, grid, resident, two)
            f.setClassEdges(EDGES[16])
        e3 = numpy.ascontiguousarray(numpy.broadcast_to(TH.astype(real)[None, :, None, None], (nt_th, NZ, ny, nx)))
        assert numpy.array_equal(e3[0, :, 0, 0].astype(numpy.float64), a.thickness)
        b.setCellThickness(_on(e3, resident), _on(e3.copy(), resident))
        for t in (0, 2):
            for carry in (False, True):
                want = _gr(a, t, carry)
                assert numpy.abs(want).max() > 0 and _same_bits(_gr(b, t, carry), want), (two, t, carry)


@pytest.mark.parametrize('thick', ['scalar', 'timevarying'])
@pytest.mark.parametrize('real', ['float64', 'float32'])
def test_same_bits_for_every_window_home_and_out(real, thick):
    import torch
    grid = GRIDS[1]
    fields = []
    for resident in (True, False):
        f = _make(real, grid, resident)
        _configure(f, real, grid, resident, True)
        f.setClassEdges(2. * numpy.arange(17))                     # 19 rows a part: one window of 32, four of 5, 19 of 1
        _thick(f, real, grid, resident, thick)
        fields.append(f)
    f, host = fields
    shape = (2 * 19, f._rowlen)
    for t, carry in ((2, False), (0, True)):
        want = _gr(f, t, carry)
        assert (numpy.abs(want).max(axis=2) > 0).sum() > 20
        for window in (1, 5, 32):
            with _window(window):
                assert _same_bits(_gr(f, t, carry), want), (t, carry, window)
        out = torch.full(shape, numpy.nan, dtype=torch.float64, device='cuda')
        assert _same_bits(_gr(f, t, carry, out=out), want)
        assert _same_bits(out.cpu().numpy().reshape(want.shape), want)
        assert _same_bits(_gr(host, t, carry), want)               # host-resident inputs, staged
        out.fill_(numpy.nan)
        assert _same_bits(_gr(host, t, carry, out=out), want)
    with pytest.raises(RuntimeError, match='out must be'):
        f.computeGrossClassRemap(0, out=torch.zeros((19, f._rowlen), dtype=torch.float64, device='cuda'))


def test_a_sigma_class_field_is_its_series_held_as_an_array():
    from nemoflux_amd.eos import Sigma, sigma_eos80
    real, grid = 'float32', GRIDS[1]
    nx, ny = grid
    rng = numpy.random.default_rng(5)
    shape = (NT, NZ, ny, nx)
    theta = (15. - 2. * numpy.arange(NZ)[None, :, None, None] + rng.standard_normal(shape)).astype(real)
    salt = (35. + 0.3 * rng.standard_normal(shape)).astype(real)
    edges = numpy.linspace(24., 29., 256)
    rows = []
    for sigma in (True, False):
        g = _make(real, grid, True, sverdrup=True)
        g.setTracer(Sigma(_on(theta, True), _on(salt, True), pref=0.) if sigma else sigma_eos80(_on(theta, True), _on(salt, True), 0.))
        g.setClassEdges(edges)
        _thick(g, real, grid, True, 'static')
        rows.append(_gr(g, 1))
    assert (numpy.abs(rows[0]).max(axis=2) > 0).sum() > 100 and _same_bits(rows[0], rows[1])


# ---- 3. ties to code that shares nothing with the kernel's row rule, to the bar ---------------------------------------------
@pytest.mark.parametrize('two', [False, True], ids=['one-tracer', 'class-tracer'])
@pytest.mark.parametrize('grid', GRIDS, ids=lambda g: f'{g[0]}x{g[1]}')
@pytest.mark.parametrize('real', ['float64', 'float32'])
def test_the_parts_add_up_to_the_net_remap_and_over_the_rows_to_the_gross_profile(real, grid, two):
    """P + N against computeClassRemap (scalar thickness); the sum over the rows of P and of N against the sum over z of the
    parts of computeGrossProfile (with a cell thickness too); the bar is 1e-12 x the reference's sum |share| of both parts"""
    resident = grid == GRIDS[1]
    u, v = _uv(real, grid)
    f = _make(real, grid, resident, sverdrup=True)
    arrays = {'uo': u, 'vo': v}
    more, class_markers = _configure(f, real, grid, resident, two)
    arrays.update(more)
    for k, (n, edges) in enumerate(EDGES.items()):
        t = k % NT
        f.setClassEdges(edges)
        for thick in ('scalar', THICK[1 + k % 2]):
            a = dict(arrays, **_thick(f, real, grid, resident, thick))
            mags = _reference(f, class_markers, sverdrup=True, cell=thick != 'scalar').gross_remap_step(array_values(a, t), edges)
            for carry, nm in ((False, 'volume'), (True, 'carried')):
                got, mag = _gr(f, t, carry), mags[nm][1]
                if thick == 'scalar':
                    _check(got[0] + got[1], _rows(f.computeClassRemap(t, carry=carry)), mag[0] + mag[1], f'P + N {nm} n={n} t={t}')
                _check(got.sum(axis=1), _gp(f, t, carry).sum(axis=1), mag.sum(axis=1), f'rows {nm} {thick} n={n} t={t}')
        f.setCellThickness(None, None)


@pytest.mark.parametrize('thick', ['scalar', 'static'])
@pytest.mark.parametrize('grid', GRIDS, ids=lambda g: f'{g[0]}x{g[1]}')
@pytest.mark.parametrize('real', ['float64', 'float32'])
def test_the_closed_form_of_the_level_index_between_integer_edges(real, grid, thick):
    """the closed form of tests/test_gpu_class_remap.py (its docstring has the derivation) on the parts of the gross profile:
    row 1 = P_0 + P_1 / 2; row k = P_{k-1} / 2 + P_k / 2; row nz - 1 = P_{nz-2} / 2 + P_{nz-1}; rows 0, n, n + 1 exactly +0.0.
    Nothing here comes from the reference but sum |terms| of the gross profile's parts"""
    from gross_reference import GrossReference
    resident = thick == 'scalar'
    level = _level_field(real, grid)
    n = NZ
    u, v = _uv(real, grid)
    f = _make(real, grid, resident, sverdrup=True)
    f.setClassEdges(numpy.arange(NZ, dtype=numpy.float64))
    tau = _tau(real, grid)
    f.setTracer(_on(tau, resident), fill_value=TFILL, missing_value=TMISSING, reference=REF)
    f.setClassTracer(_on(level, resident))
    arrays = dict({'uo': u, 'vo': v, 'tracer': tau}, **_thick(f, real, grid, resident, thick))
    ce, w, sg = f.getWeights()
    r = GrossReference(ce, w, sg, f.arcLengths, f.thickness, f._tr_off, f.nx, f.ny, uv_markers=(FILL, MISSING),
                       tracer_markers=(TFILL, TMISSING), thick_markers=(THFILL, THMISSING), reference=REF, sverdrup=True,
                       cell_thickness=thick != 'scalar')
    for t in range(NT):
        mags = r.gross_step(array_values(arrays, t))
        for carry, nm in ((False, 'volume'), (True, 'carried')):
            got, P, M = _gr(f, t, carry), _gp(f, t, carry), mags[nm][1]
            assert got.shape == (2, n + 2, f._rowlen)
            half = lambda k: 0.5 * P[:, k]   # noqa: E731
            _check(got[:, 1], P[:, 0] + half(1), M[:, 0] + M[:, 1], f'row 1 {nm} t={t}')
            for k in range(2, n - 1):
                _check(got[:, k], half(k - 1) + half(k), M[:, k - 1] + M[:, k], f'row {k} {nm} t={t}')
            _check(got[:, n - 1], half(n - 2) + P[:, n - 1], M[:, n - 2] + M[:, n - 1], f'row {n - 1} {nm} t={t}')
            assert not numpy.ascontiguousarray(got[:, [0, n, n + 1]]).view(numpy.uint64).any(), (nm, t)    # exactly +0.0


# ---- 4. sharding -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('home', ['hbm', 'host'])
@pytest.mark.parametrize('real', ['float64', 'float32'])
def test_two_sharded_halves_meet_the_reference_and_add_up_to_the_unsharded_rows(real, home):
    """slab ranges that cut inside a time step: each half against the reference of its levels -- the class field is read one
    level beyond the cut, in place in HBM or staged from the host with the owned levels; the thickness (time-varying, on the
    host with the host class field) at the owned levels only -- and the halves added up against the unsharded rows; a step that
    a rank does not touch gives exact zeros"""
    from nemoflux_amd.dist import slab_range
    grid, world, resident = GRIDS[1], 2, home == 'hbm'
    u, v = _uv(real, grid)
    arrays = {'uo': u, 'vo': v}
    made = {}

    def make(**kw):
        f = _make(real, grid, resident, **kw)
        more, made['markers'] = _configure(f, real, grid, resident, True)
        arrays.update(more)
        arrays.update(_thick(f, real, grid, resident, 'timevarying'))
        f.setClassEdges(EDGES[1025])
        return f

    full = make()
    r = _reference(full, made['markers'], cell=True)
    want = numpy.array([[_gr(full, t, carry) for carry in (False, True)] for t in range(NT)])
    acc = numpy.zeros_like(want)
    cut_inside = untouched = False
    for rank in range(world):
        sr = slab_range(NT, NZ, rank, world)
        cut_inside = cut_inside or sr[0] % NZ != 0
        part = make(slab_range=sr)
        for t in range(NT):
            z0, z1 = max(sr[0], t * NZ) - t * NZ, min(sr[1], (t + 1) * NZ) - t * NZ
            ref = r.gross_remap_step(array_values(arrays, t), EDGES[1025], levels=(z0, z1)) if z1 > z0 else None
            for k, (carry, nm) in enumerate(((False, 'volume'), (True, 'carried'))):
                got = _gr(part, t, carry)
                if ref is None:
                    untouched = True
                    assert not got.view(numpy.uint64).any(), (rank, t, carry)
                else:
                    _close(got, *ref[nm], f'rank {rank} levels [{z0}, {z1}) {nm} t={t}')
                acc[t, k] += got
    assert cut_inside and untouched
    for t in range(NT):
        ref = r.gross_remap_step(array_values(arrays, t), EDGES[1025])
        for k, nm in enumerate(('volume', 'carried')):
            _check(acc[t, k], want[t, k], ref[nm][1], f'two halves, {nm} t={t}')


# ---- 5. state and re-use ---------------------------------------------------------------------------------------------------
def test_the_refusals_and_what_the_call_leaves_alone():
    from nemoflux_amd._lib import lib
    real, grid = 'float64', GRIDS[0]
    f = _make(real, grid, True)
    with pytest.raises(RuntimeError, match='setClassEdges first'):
        f.computeGrossClassRemap(0)
    f.setClassEdges(numpy.array([1., 2.]))
    with pytest.raises(RuntimeError, match='setTracer first'):
        f.computeGrossClassRemap(0, carry=True)
    g = _make(real, grid, True)
    _configure(g, real, grid, True, True)
    g.setClassEdges(EDGES[16])
    host = numpy.zeros((2 * 18, g._rowlen))
    assert lib.nf_field_compute_gross_class_remap(ctypes.byref(g._h), NT, 0, host.ctypes.data_as(dp)) == 1
    assert b'time index' in lib.nf_last_error()
    assert lib.nf_field_compute_gross_class_remap(ctypes.byref(g._h), 0, 2, host.ctypes.data_as(dp)) == 1
    assert b'carry must be 0 or 1' in lib.nf_last_error() and not host.any()
    # the call changes none of the other products, with or without a cell thickness, and the net remap stays refused with one
    for thick in ('scalar', 'static'):
        _thick(g, real, grid, True, thick)
        others = lambda: [_gc(g, 1), _gc(g, 1, True), _gp(g, 1), _rows(g.computeClassArea(1)), _rows(g.computeFluxProfile(1))]   # noqa: E731
        before, flux = others(), g.computeFlux(1)
        first = _gr(g, 1), _gr(g, 2, True)
        assert numpy.abs(first[0]).max() > 0 and g.computeFlux(1) == flux
        for x, y in zip(others(), before):
            assert _same_bits(x, y), thick
        assert _same_bits(_gr(g, 1), first[0]) and _same_bits(_gr(g, 2, True), first[1])
    with pytest.raises(RuntimeError, match='does not take per-cell thicknesses yet'):
        g.computeClassRemap(0)


def test_gross_class_gross_remap_class_remap_on_one_handle_equal_fresh_handles():
    """gross class -> gross remap -> class remap -> gross remap on one handle, a cell thickness set and cleared in between (the
    class remap is called only while none is set); then another dtype, more levels and other edges: the bits of fresh handles
    that make that call alone, and the resident planes are the same bytes before and after"""
    from test_gpu_reuse import TRANSECTS
    from test_gpu_reuse_products import ProductHandle
    ny, nx, nt = 24, 40, 2

    def state(nz, dtype, seed, ec):
        shape = (nt, nz, ny, nx)
        u, v = gross_velocities(dtype, shape, seed=seed)
        rng = numpy.random.default_rng(seed + 1)
        A = (5. + 2. * rng.standard_normal(shape)).astype(dtype)
        B = (rng.integers(0, 2048, shape) / 512. + numpy.arange(nz)[None, :, None, None]).astype(dtype)
        A[:, :, 3:6, 5:9] = numpy.nan
        B[:, :, 10:12, 20:30] = numpy.nan
        e3u, e3v = depth_thickness(dtype, (1, nz, ny, nx), seed=seed + 2)
        return dict(nz=nz, u=u, v=v, A=A, B=B, ec=ec, e3u=e3u, e3v=e3v)

    def apply(h, s, first, cell):
        if first:
            h.set_bounds(ny, nx, numpy.float64, True)
        h.set_thickness(numpy.linspace(0.25, 2., s['nz']))
        h.set_uv(s['u'], s['v'], True, FILL)
        h.set_tracer(s['A'], True, None)
        h.set_class_tracer(s['B'], True, None)
        if first:
            for line in TRANSECTS[:3]:
                h.add_transect(line)
            h.call('build_weights', 128, 360.)
        h.set_class_edges(s['ec'])
        thick(h, s, cell)

    def thick(h, s, cell):
        if cell:
            h.set_cell_thickness(s['e3u'], s['e3v'], True, THFILL)
        else:
            h.set_cell_thickness(None, None, True, None)

    def rows(h, name, nrows):
        out = []
        for carry in (0, 1):
            r = numpy.full((nrows, h.rowlen()), numpy.nan)
            h.call(name, 1, carry, r.ctypes.data_as(dp))
            out.append(r)
        return numpy.array(out)

    gc = lambda h, s: rows(h, 'compute_gross_class_transport', 2 * (s['ec'].size + 2))   # noqa: E731
    gr = lambda h, s: rows(h, 'compute_gross_class_remap', 2 * (s['ec'].size + 2))       # noqa: E731
    cr = lambda h, s: rows(h, 'compute_class_remap', s['ec'].size + 2)                   # noqa: E731
    lin = numpy.linspace
    states = [state(3, numpy.float64, 71, lin(0., 6., 5)), state(7, numpy.float32, 73, lin(0., 10., 1025)),
              state(5, numpy.float64, 79, lin(0., 8., 40))]
    plan = [(gc, True), (gr, True), (cr, False), (gr, False), (gr, True)]
    h = ProductHandle()
    for k, s in enumerate(states):
        apply(h, s, k == 0, True)
        planes = h.compute('flux', 1, ny * nx)[1:]
        for call, cell in plan:
            thick(h, s, cell)
            got = call(h, s)
            fresh = ProductHandle()
            apply(fresh, s, True, cell)
            assert numpy.isfinite(got).all() and numpy.abs(got).max() > 0, (k, cell)
            assert _same_bits(got, call(fresh, s)), (k, cell)
            for x, y in zip(h.planes(ny * nx), planes):
                assert _same_bits(x, y), (k, cell)
        assert not numpy.array_equal(gr(h, s), gc(h, s))


# ---- 6. higher layers ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('real', ['float64', 'float32'])
def test_the_eddy_part_is_rounding_where_only_the_velocities_vary(real):
    """the module docstring says why the parts need velocities of constant sign; the bar is that of
    tests/test_gpu_selected_mean.py: 1e-12 x (the mean over the steps of the reference's sum |share| + that of the mean state)"""
    from nemoflux_amd.field import Field
    grid, resident = GRIDS[0], True
    nx, ny = grid
    u, v = _uv(real, grid)
    dt = u.dtype.type
    rng = numpy.random.default_rng(29)
    sign = [rng.choice([-1., 1.], (1, NZ, ny, nx)).astype(real) for _ in range(2)]

    def steady(x, s):
        keep = numpy.isnan(x) | (x == dt(FILL)) | (x == dt(MISSING))
        return numpy.where(keep, x, numpy.abs(x) * s)

    def mean_of(x):
        """the velocities of the mean state for the bar's sum |share|: a missing value counts as 0 at every step"""
        keep = numpy.isnan(x) | (x == dt(FILL)) | (x == dt(MISSING))
        return numpy.where(keep, 0., x.astype(numpy.float64)).mean(axis=0, keepdims=True).astype(real)

    lat, tau = _sibling_lattice(real, grid, True), _tau(real, grid)
    const =lambda a: numpy.ascontiguousarray(numpy.broadcast_to(a[1], a.shape))   # noqa: E731
    e3u, e3v = depth_thickness(real, (1, NZ, ny, nx), seed=31)
    for name, (uu, vv) in (('steady', (steady(u, sign[0]), steady(v, sign[1]))), ('any', (u, v))):
        f = _make(real, grid, resident, u=uu, v=vv, sverdrup=True)
        f.setTracer(_on(const(tau), resident), fill_value=TFILL, missing_value=TMISSING, reference=REF)
        f.setClassTracer(_on(const(lat), resident), fill_value=SFILL, missing_value=SMISSING)
        f.setCellThickness(_on(e3u, resident), _on(e3v, resident), fill_value=THFILL, missing_value=THMISSING)
        f.setClassEdges(EDGES[16])
        arrays = {'uo': uu, 'vo': vv, 'tracer': const(tau), 'class': const(lat), 'e3u': e3u, 'e3v': e3v}
        r = _reference(f, (SFILL, SMISSING), sverdrup=True, cell=True)
        steps = [r.gross_remap_step(array_values(arrays, t), EDGES[16]) for t in range(NT)]
        state = r.gross_remap_step(array_values(dict(arrays, uo=mean_of(uu), vo=mean_of(vv)), 0), EDGES[16])
        for carry, nm in ((False, 'volume'), (True, 'carried')):
            d = _quiet(f.meanEddySplit, 'computeGrossClassRemap', carry=carry)
            eddy, total = _rows(d['eddy']), _rows(d['total'])
            bar = BAR * (numpy.mean([s[nm][1] for s in steps], axis=0) + state[nm][1])
            assert eddy.shape == bar.shape == (2, 18, f._rowlen) and numpy.abs(total).max() > 0 and bar.max() > 0
            if name == 'any':                                     # P + N is linear whatever the signs do
                eddy, bar = eddy[0] + eddy[1], bar[0] + bar[1]
            print(f'{real} {name} {nm}: max |eddy| / bar = {float((numpy.abs(eddy) / numpy.maximum(bar, 1e-300)).max()):.3g} x 1e-12')
            assert numpy.all(numpy.abs(eddy) <= bar), (name, nm)
        mean = d['meanField']
        assert isinstance(mean, Field) and mean.nt == 1 and numpy.array_equal(mean._class_edges, EDGES[16])
    psi = Field.classStreamfunction(total[0][:, -3:] + total[1][:, -3:])
    assert psi.shape == (16, 3) and numpy.isfinite(psi).all() and numpy.abs(psi).max() > 0
    assert Field.grossTransport(total[:, :, -3:]).shape == (2, 3)


@pytest.mark.parametrize('carry', [False, True], ids=['volume', 'carried'])
def test_fluxplot_gross_remap_is_the_field_table(tmp_path, carry):
    from nemoflux_amd import fluxplot
    real, grid = 'float32', GRIDS[0]
    nx, ny = grid
    blon, blat = _case(real, grid)[:2]
    u, v = _uv(real, grid)
    tau, sig = _tau(real, grid), _sibling_lattice(real, grid, True)
    e3u, e3v = depth_thickness(real, (NT, NZ, ny, nx), seed=5)
    paths = {k: str(tmp_path / f'{k}.npz') for k in 'TUVS'}
    fv = lambda name, a, b: {f'_FillValue_{name}': numpy.array(a), f'_missing_value_{name}': numpy.array(b)}   # noqa: E731
    numpy.savez(paths['T'], bounds_lon=blon, bounds_lat=blat, deptht_bounds=DB, thetao=tau, **fv('thetao', TFILL, TMISSING))
    numpy.savez(paths['S'], sigma0=sig, **fv('sigma0', SFILL, SMISSING))
    numpy.savez(paths['U'], uo=u, e3u=e3u, **fv('uo', FILL, MISSING), **fv('e3u', THFILL, THMISSING))
    numpy.savez(paths['V'], vo=v, e3v=e3v, **fv('vo', FILL, MISSING), **fv('e3v', THFILL, THMISSING))
    edges = EDGES[16]
    lines = '[' + T_OPEN + '],[' + T_SEAM + ']'
    out = str(tmp_path / 'gross_remap.csv')
    kw = dict(tFile=paths['T'], uFile=paths['U'], vFile=paths['V'], tracer='sigma0', tracerFile=paths['S'],
              grossClasses=','.join(repr(float(e)) for e in edges), grossRemap='linear', cellThickness=True)
    if carry:
        kw.update(carry='thetao', carryRef=1.5, carryScale=4.1e-3)
    totals = _quiet(fluxplot.main, lonLatPoints=lines, output=out, sverdrup=True, **kw)
    mem = _field(blon, blat, DB, u, v, fluxplot.readTargets(lines)[0], True, fill_value=FILL, missing_value=MISSING,
                 readback=False)
    if carry:
        mem.setTracer(tau, fill_value=TFILL, missing_value=TMISSING, reference=1.5)
        mem.setClassTracer(sig, fill_value=SFILL, missing_value=SMISSING)
    else:
        mem.setTracer(sig, fill_value=SFILL, missing_value=SMISSING)
    mem.setCellThickness(e3u, e3v, fill_value=THFILL, missing_value=THMISSING)
    mem.setClassEdges(edges)
    with open(out) as fh:
        text = fh.read().splitlines()
    assert text[0] == ('# gross transport of thetao by sigma0 class [thetao x Sv x 0.0041], conservative remapping' if carry
                       else '# gross water flow by sigma0 class [Sv], conservative remapping')
    assert text[1] == 'time,transect,lower,upper,inflow,outflow,net'
    assert totals.shape == (NT, 2, edges.size + 2, 2) and len(text) == 2 + NT * 2 * (edges.size + 2)
    scale = 4.1e-3 if carry else 1.0
    for t in range(NT):
        want = mem.computeGrossClassRemap(t, carry=carry)[0] * scale
        assert _same_bits(totals[t], want) and (numpy.abs(want).max(axis=2) > 0).sum() > 20
        assert not numpy.array_equal(want, mem.computeGrossClassTransport(t, carry=carry)[0] * scale)
