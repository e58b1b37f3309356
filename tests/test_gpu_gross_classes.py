"""Gross (inflow / outflow) transports in tracer classes on the GPU (Field.computeGrossClassTransport,
nf_field_compute_gross_class_transport, fluxplot --gross-classes).  Every value of P and N in all forms -- volume, carried
tracer that is the class field, carried tracer with a class field of its own, each with the scalar or a per-cell thickness --
is checked against the float64 / long-double restatement of tests/gross_class_reference.py to 1e-12 x sum |c| of that value
(the A7 bar of docs/PARITY.md), no row or column left out; anchored bit for bit (negating uo / vo swaps and negates the parts;
one class per level gives the rows of computeGrossProfile; tau = ref + 1 gives the volume parts; a broadcast cell thickness is
the scalar form; every joint_window / joint_skip, out= and host inputs give the same bits); P + N against the net class rows,
the sum over the classes against the gross profile, two sharded halves against the unsharded rows, to the bar on sum |c| of
both parts; nothing else is disturbed, the shared term table follows joint -> gross class -> joint on one handle, the
thickness-weighted mean state works, the refusals; fluxplot --gross-classes from files.

Grids 72 x 36 x 7 x 3 and 73 x 37 x 7 x 3 with three transects (one across the periodic seam): 265 to 325 records, two blocks
of the kernels; seven levels leave a tail behind every batch length.  The inputs are those of tests/test_gpu_gross.py, which
keep every non-zero |q| far from underflow; min_abs_q of the reference is asserted wherever a reference is formed.

Measured on an MI355X: worst |error| 4.1e-16 x sum |c| against the reference, 2.0e-16 for the two sharded halves; 131 tests in
4.6 s."""
import ctypes

import numpy
import pytest

from conftest import transect_xyz
from gpu_helpers import _field, _on, _quiet, _rows, _same_bits
from gross_class_reference import GrossClassReference
from gross_reference import MIN_ABS_Q, array_values, gross_thickness, gross_velocities
from test_gpu_cellthick import (BAR, FILL, MISSING, T_OPEN, T_SEAM, T_TRI, TFILL, THFILL, THMISSING, TMISSING, _case, _resident,
                                _row)
from test_gpu_gross import DB, GRIDS, NT, NZ, REF, TH, _gross, _make as _make_gross, _set_thickness, _tau, _uv
from test_gpu_joint_classes import _skip, _window

pytestmark = pytest.mark.gpu

LINES = [T_OPEN, T_TRI, T_SEAM]
SFILL, SMISSING = -8888., 5.e15
SIG0, SIGS = 27., 1.2                                   # the class tracer: SIG0 + SIGS x a standard normal
dp = ctypes.POINTER(ctypes.c_double)


def _edges(n, centre, scale):
    """n class edges around the centre of a field of that scale; one of them (n >= 3) is a value the field takes"""
    return centre + scale * (numpy.array([-0.5, 0.5]) if n == 2 else numpy.linspace(-2., 2., n))


EDGE_COUNTS = (2, 3, 16, 1025)                          # 16: 36 rows, two windows of 32; 1025: the most there can be
_SIG = {}


def _sigma(real, grid, seed=41):
    """a class tracer with NaN and both of its own markers in it, and values that sit on a class edge"""
    if (real, grid) not in _SIG:
        nx, ny = grid
        rng = numpy.random.default_rng(seed)
        dt = numpy.dtype(real).type
        shape = (NT, NZ, ny, nx)
        sig = (SIG0 + SIGS * rng.standard_normal(shape)).astype(real)
        sig[rng.random(shape) < 0.04] = dt(SIG0)              # on the middle edge of every odd edge count
        sig[:, ::2, 2:-2:3, 3:-2:5] = numpy.nan
        sig[:, :, 12:17, 40:58] = dt(SFILL)
        sig[:, 3:, 24:29, 3:14] = dt(SMISSING)
        _SIG[real, grid] = sig
    return _SIG[real, grid]


def _make(real, grid, resident, **kw):
    return _make_gross(real, grid, resident, lines=LINES, **kw)


def _configure(f, real, grid, resident, two, wrap=True, ref=REF):
    """two = False: the tracer is the class field (and the carried tracer); True: a class tracer of its own.  Returns the
    arrays of the reference, its class markers and the centre / scale of the class field."""
    tau = _tau(real, grid)
    f.setTracer(_on(tau, resident), fill_value=TFILL, missing_value=TMISSING, reference=ref, wrapX=wrap)
    if not two:
        return {'tracer': tau, 'class': tau}, (TFILL, TMISSING), (REF, 2.)
    sig = _sigma(real, grid)
    f.setClassTracer(_on(sig, resident), fill_value=SFILL, missing_value=SMISSING)
    return {'tracer': tau, 'class': sig}, (SFILL, SMISSING), (SIG0, SIGS)


def _gc(f, t, carry=False, **kw):
    """(2, nedges + 2, row_length): P, N as [segments | transects] rows"""
    return _rows(f.computeGrossClassTransport(t, carry=carry, **kw))


def _reference(f, class_markers, wrap=True, ref=REF, sverdrup=False, cell_thickness=False):
    ce, w, sg = f.getWeights()
    return GrossClassReference(ce, w, sg, f.arcLengths, f.thickness, f._tr_off, f.nx, f.ny, uv_markers=(FILL, MISSING),
                               tracer_markers=(TFILL, TMISSING), class_markers=class_markers, thick_markers=(THFILL, THMISSING),
                               reference=ref, wrap=wrap, sverdrup=sverdrup, cell_thickness=cell_thickness)


def _close(got, want, mag, label):
    assert got.shape == want.shape == mag.shape, label
    err = numpy.abs(got - want)
    worst = float((err / numpy.maximum(mag, 1e-300)).max())
    print(f'{label}: max |err| / sum |c| = {worst:.3g}')
    assert numpy.all(err <= BAR * mag), (label, worst)


# ---- 1. against the reference; the signs of the volume form --------------------------------------------------------------
@pytest.mark.parametrize('thick', ['scalar', 'static', 'timevarying'])
@pytest.mark.parametrize('wrap', [True, False], ids=['wrap-sv', 'nowrap-m2'])
@pytest.mark.parametrize('resident', [True, False], ids=['hbm', 'host'])
@pytest.mark.parametrize('grid', GRIDS, ids=lambda g: f'{g[0]}x{g[1]}')
@pytest.mark.parametrize('real', ['float64', 'float32'])
def test_against_the_reference(real, grid, resident, wrap, thick):
    """volume, carried-one and carried-two forms; every edge count, each on one of the steps"""
    u, v = _uv(real, grid)
    dt = u.dtype.type
    assert numpy.isnan(v).any() and (u == dt(FILL)).any() and (u == dt(MISSING)).any() and (u == 0).any()
    seen_no_value = False
    for two in (False, True):
        f = _make(real, grid, resident, sverdrup=wrap)
        ce = f.getWeights()[0]
        assert ce.size > 256 and (ce // 4 % f.nx == f.nx - 1).any()        # the seam: east faces of the last column
        arrays = {'uo': u, 'vo': v}
        arrays.update(_set_thickness(f, real, grid, resident, thick))
        more, class_markers, (centre, scale) = _configure(f, real, grid, resident, two, wrap=wrap)
        arrays.update(more)
        r = _reference(f, class_markers, wrap=wrap, sverdrup=wrap, cell_thickness=thick != 'scalar')
        for k, n in enumerate(EDGE_COUNTS):
            t = k % NT
            edges = _edges(n, centre, scale)
            f.setClassEdges(edges)
            want = r.gross_class_step(array_values(arrays, t), edges)
            assert want['min_abs_q'] >= MIN_ABS_Q
            vol, car = _gc(f, t), _gc(f, t, carry=True)
            assert vol.shape == car.shape == (2, n + 2, f._rowlen)
            label = f'{"two" if two else "one"} n={n} t={t}'
            _close(vol, *want['volume'], 'volume ' + label)
            _close(car, *want['carried'], 'carried ' + label)
            assert (vol[0] >= 0).all() and (vol[1] <= 0).all() and (vol[0] > 0).any() and (vol[1] < 0).any()
            assert (car[0] < 0).any() and (car[1] > 0).any()          # split by the water, not by the sign of the carried term
            seen_no_value = seen_no_value or want['volume'][1][:, n + 1].max() > 0
    assert seen_no_value, 'the row of the faces without a class value has terms'


# ---- 2. bit-for-bit identities -------------------------------------------------------------------------------------------
@pytest.mark.parametrize('thick', ['scalar', 'timevarying'])
@pytest.mark.parametrize('grid', GRIDS, ids=lambda g: f'{g[0]}x{g[1]}')
@pytest.mark.parametrize('real', ['float64', 'float32'])
def test_negated_velocities_swap_and_negate_the_parts(real, grid, thick):
    resident = grid == GRIDS[0]
    u, v = _uv(real, grid)
    dt = u.dtype.type

    def negated(x):
        keep = numpy.isnan(x) | (x == dt(FILL)) | (x == dt(MISSING))
        return numpy.where(keep, x, -x)

    for two in (False, True):
        a, b = _make(real, grid, resident, sverdrup=True), _make(real, grid, resident, u=negated(u), v=negated(v), sverdrup=True)
        for f in (a, b):
            _set_thickness(f, real, grid, resident, thick)
            _, _, (centre, scale) = _configure(f, real, grid, resident, two)
            f.setClassEdges(_edges(16, centre, scale))
        for t in range(NT):
            for carry in (False, True):
                p, n = _gc(a, t, carry)
                pm, nm = _gc(b, t, carry)
                assert numpy.abs(p).max() > 0 and numpy.abs(n).max() > 0
                assert numpy.array_equal(pm, -n) and numpy.array_equal(nm, -p), (two, t, carry)


@pytest.mark.parametrize('thick', ['scalar', 'static', 'timevarying'])
@pytest.mark.parametrize('resident', [True, False], ids=['hbm', 'host'])
@pytest.mark.parametrize('grid', GRIDS, ids=lambda g: f'{g[0]}x{g[1]}')
@pytest.mark.parametrize('real', ['float64', 'float32'])
def test_one_class_per_level_gives_the_gross_profile_bit_for_bit(real, grid, resident, thick):
    """a class field equal to the level index, edges at the half-integers: row z holds exactly the terms of level z, added
    into +0.0 in the same order as computeGrossProfile adds them; the row of the faces without a class value stays +0.0"""
    nx, ny = grid
    level = numpy.ascontiguousarray(numpy.broadcast_to(numpy.arange(NZ, dtype=real)[None, :, None, None], (NT, NZ, ny, nx)))
    edges = numpy.arange(NZ - 1) + 0.5
    f = _make(real, grid, resident, sverdrup=True)
    _set_thickness(f, real, grid, resident, thick)
    f.setClassEdges(edges)
    # the level index as the class tracer of another carried tracer, then as the one tracer, carried itself
    f.setTracer(_on(_tau(real, grid), resident), fill_value=TFILL, missing_value=TMISSING, reference=REF)
    f.setClassTracer(_on(level, resident))
    for two in (True, False):
        if not two:
            f.setClassTracer(None)
            f.setTracer(_on(level, resident), reference=2.0)
        for t in range(NT):
            for carry in (False, True):
                got, want = _gc(f, t, carry), _gross(f, t, carry)
                assert got.shape == (2, NZ + 1, f._rowlen) and numpy.abs(want[0]).max() > 0 and numpy.abs(want[1]).max() > 0
                assert _same_bits(got[:, :NZ], want), (two, t, carry)
                assert not got[:, NZ].view(numpy.uint64).any()


@pytest.mark.parametrize('thick', ['scalar', 'timevarying'])
@pytest.mark.parametrize('grid', GRIDS, ids=lambda g: f'{g[0]}x{g[1]}')
@pytest.mark.parametrize('real', ['float64', 'float32'])
def test_tracer_one_above_the_reference_is_carried_like_the_water(real, grid, thick):
    """tau == ref + 1 everywhere, ref an integer != 0: tf == 1 exactly at every face that has a value, so the carried parts are
    the volume parts bit for bit.  With wrapX only the north faces of the last row have no value, and no line comes near it."""
    resident = grid == GRIDS[1]
    nx, ny = grid
    tau = numpy.full((NT, NZ, ny, nx), 8., real)
    f = _make(real, grid, resident)
    assert (f.getWeights()[0] // 4 // nx).max() < ny - 1
    _set_thickness(f, real, grid, resident, thick)
    f.setTracer(_on(tau, resident), reference=7.0)
    f.setClassEdges(numpy.array([7.5, 8.5]))                       # the tracer is the class field: everything in row 1
    for t in range(NT):
        vol = _gc(f, t)
        assert numpy.abs(vol[0, 1]).max() > 0 and numpy.abs(vol[1, 1]).max() > 0 and not vol[:, [0, 2, 3]].any()
        assert numpy.array_equal(_gc(f, t, carry=True), vol), t
    f.setClassTracer(_on(_sigma(real, grid), resident), fill_value=SFILL, missing_value=SMISSING)     # a class field of its own
    f.setClassEdges(_edges(16, SIG0, SIGS))
    for t in range(NT):
        vol = _gc(f, t)
        assert (numpy.abs(vol).max(axis=2) > 0).sum() > 20
        assert numpy.array_equal(_gc(f, t, carry=True), vol), t
    f.setTracer(_on(tau, resident), reference=6.0)                 # tf == 2: exactly twice
    assert numpy.array_equal(_gc(f, 1, carry=True), 2. * _gc(f, 1))


@pytest.mark.parametrize('nt_th', [1, NT], ids=['static', 'timevarying'])
@pytest.mark.parametrize('grid', GRIDS, ids=lambda g: f'{g[0]}x{g[1]}')
@pytest.mark.parametrize('real', ['float64', 'float32'])
def test_broadcast_cell_thickness_is_the_scalar_form(real, grid, nt_th):
    resident = grid == GRIDS[0]
    nx, ny = grid
    e3 = numpy.ascontiguousarray(numpy.broadcast_to(TH.astype(real)[None, :, None, None], (nt_th, NZ, ny, nx)))
    for two in (False, True):
        a, b = _make(real, grid, resident), _make(real, grid, resident)
        a.setCellThickness(_on(e3, resident), _on(e3.copy(), resident))
        for f in (a, b):
            _, _, (centre, scale) = _configure(f, real, grid, resident, two)
            f.setClassEdges(_edges(16, centre, scale))
        for t in (1, 0, 2):
            for carry in (False, True):
                want = _gc(b, t, carry)
                assert numpy.abs(want).max() > 0
                assert _same_bits(_gc(a, t, carry), want), (two, t, carry)
        a.setCellThickness(_on(2 * e3, resident), _on(e3, resident))
        assert not numpy.array_equal(_gc(a, 1), _gc(b, 1))
        a.setCellThickness(None, None)
        assert _same_bits(_gc(a, 1, True), _gc(b, 1, True))


@pytest.mark.parametrize('thick', ['scalar', 'static'])
@pytest.mark.parametrize('real', ['float64', 'float32'])
def test_same_bits_for_every_window_skip_home_and_out(real, thick):
    import torch
    grid = GRIDS[1]
    fields = []
    for resident in (True, False):
        f = _make(real, grid, resident)
        _set_thickness(f, real, grid, resident, thick)
        _, _, (centre, scale) = _configure(f, real, grid, resident, True)
        f.setClassEdges(_edges(16, centre, scale))                 # 36 rows: two windows of 32, eight of 5, 36 of 1
        fields.append(f)
    f, host = fields
    shape = (2 * 18, f._rowlen)
    for t in (2, 0):
        for carry in (False, True):
            want = _gc(f, t, carry)
            assert numpy.abs(want[0]).max() > 0 and numpy.abs(want[1]).max() > 0
            for window in (1, 5, 32):
                for skip in (0, 1):
                    with _window(window), _skip(skip):
                        assert _same_bits(_gc(f, t, carry), want), (t, carry, window, skip)
            out = torch.full(shape, numpy.nan, dtype=torch.float64, device='cuda')
            assert _same_bits(_gc(f, t, carry, out=out), want)
            assert _same_bits(out.cpu().numpy().reshape(want.shape), want)
            assert _same_bits(_gc(host, t, carry), want)               # host-resident inputs, staged
            out.fill_(numpy.nan)
            assert _same_bits(_gc(host, t, carry, out=out), want)
    for bad in (torch.zeros(shape, dtype=torch.float32, device='cuda'),
                torch.zeros((shape[0] + 1, shape[1]), dtype=torch.float64, device='cuda'),
                torch.zeros((2, 18, f._rowlen), dtype=torch.float64, device='cuda'), torch.zeros(shape, dtype=torch.float64),
                torch.zeros(shape[::-1], dtype=torch.float64, device='cuda').t()):
        with pytest.raises(RuntimeError, match='out must be'):
            f.computeGrossClassTransport(0, out=bad)


# ---- 3. to the bar on sum |c| of both parts ---------------------------------------------------------------------------------
def _check(got, net, mag, label):
    err = numpy.abs(got - net)
    worst = float((err / numpy.maximum(mag, 1e-300)).max())
    print(f'{label}: max |err| / sum |c| = {worst:.3g}')
    assert net.shape == got.shape == mag.shape and numpy.abs(net).max() > 0 and numpy.all(err <= BAR * mag), (label, worst)


@pytest.mark.parametrize('two', [False, True], ids=['one-tracer', 'class-tracer'])
@pytest.mark.parametrize('resident', [True, False], ids=['hbm', 'host'])
@pytest.mark.parametrize('grid', GRIDS, ids=lambda g: f'{g[0]}x{g[1]}')
@pytest.mark.parametrize('real', ['float64', 'float32'])
def test_the_parts_add_up_to_the_net_class_rows_and_to_the_gross_profile(real, grid, resident, two):
    """P + N against computeClassTransport and computeClassTracerTransport (scalar thickness); the sum over the classes of P and
    of N against the sum over z of computeGrossProfile's parts, with a cell thickness too: within 1e-12 x the reference's
    sum |c| of the two parts together"""
    u, v = _uv(real, grid)
    f = _make(real, grid, resident, sverdrup=True)
    arrays = {'uo': u, 'vo': v}
    more, class_markers, (centre, scale) = _configure(f, real, grid, resident, two)
    arrays.update(more)
    edges = _edges(16, centre, scale)
    f.setClassEdges(edges)
    for thick in ('scalar', 'timevarying'):
        arrays.update(_set_thickness(f, real, grid, resident, thick))
        r = _reference(f, class_markers, sverdrup=True, cell_thickness=thick != 'scalar')
        for t in range(NT):
            want = r.gross_class_step(array_values(arrays, t), edges)
            assert want['min_abs_q'] >= MIN_ABS_Q
            for carry, nm in ((False, 'volume'), (True, 'carried')):
                got, both = _gc(f, t, carry), want[nm][1].sum(axis=0)
                if thick == 'scalar':
                    net = _rows((f.computeClassTracerTransport if carry else f.computeClassTransport)(t))
                    _check(got[0] + got[1], net, both, f'P + N, {nm} t={t}')
                else:
                    with pytest.raises(RuntimeError, match='per-cell thicknesses'):       # the net forms still take none
                        (f.computeClassTracerTransport if carry else f.computeClassTransport)(t)
                prof = _gross(f, t, carry)
                total = numpy.broadcast_to(both.sum(axis=0), got[:, 0].shape)
                _check(got.sum(axis=1), prof.sum(axis=1), total, f'sum over the classes, {nm} {thick} t={t}')


@pytest.mark.parametrize('thick', ['scalar', 'timevarying'])
@pytest.mark.parametrize('real', ['float64', 'float32'])
def test_two_sharded_halves_add_up_to_the_unsharded_rows(real, thick):
    """slab ranges that cut inside a time step: a class row takes terms from the levels of both ranks, so the halves add up to
    the unsharded rows up to rounding -- within the bar on the reference's sum |c| of both parts; a step that a rank does not
    touch gives exact zeros"""
    from nemoflux_amd.dist import slab_range
    grid, world, resident = GRIDS[1], 2, True
    u, v = _uv(real, grid)
    arrays = {'uo': u, 'vo': v}
    made = {}

    def make(**kw):
        f = _make(real, grid, resident, **kw)
        arrays.update(_set_thickness(f, real, grid, resident, thick))
        more, made['markers'], (centre, scale) = _configure(f, real, grid, resident, True)
        arrays.update(more)
        made['edges'] = _edges(16, centre, scale)
        f.setClassEdges(made['edges'])
        return f

    full = make()
    r = _reference(full, made['markers'], cell_thickness=thick != 'scalar')
    want = numpy.array([[_gc(full, t, carry) for carry in (False, True)] for t in range(NT)])
    acc = numpy.zeros_like(want)
    cut_inside = untouched = False
    for rank in range(world):
        sr = slab_range(NT, NZ, rank, world)
        cut_inside = cut_inside or sr[0] % NZ != 0
        part = make(slab_range=sr)
        for t in range(NT):
            owns = min(sr[1], (t + 1) * NZ) > max(sr[0], t * NZ)
            for k, carry in enumerate((False, True)):
                got = _gc(part, t, carry)
                if not owns:
                    untouched = True
                    assert not got.view(numpy.uint64).any(), (rank, t, carry)
                acc[t, k] += got
    assert cut_inside and untouched
    for t in range(NT):
        ref = r.gross_class_step(array_values(arrays, t), made['edges'])
        assert ref['min_abs_q'] >= MIN_ABS_Q
        for k, nm in enumerate(('volume', 'carried')):
            both = numpy.broadcast_to(ref[nm][1].sum(axis=0), want[t, k].shape)
            _check(acc[t, k], want[t, k], both, f'two halves, {nm} t={t}')


# ---- 4. state and re-use -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('thick', ['scalar', 'timevarying'])
@pytest.mark.parametrize('resident', [True, False], ids=['hbm', 'host'])
def test_the_call_leaves_everything_else_alone(resident, thick):
    real, grid = 'float64', GRIDS[0]
    a, b = _make(real, grid, resident), _make(real, grid, resident)
    eA, eB = _edges(3, REF, 2.), _edges(5, SIG0, SIGS)
    for f in (a, b):
        _configure(f, real, grid, resident, True)
        f.setClassEdges(eB)
        f.setJointClassEdges(eA, eB)
    # the net class and joint rows take no cell thickness: theirs are taken before it is set, and after it is cleared
    cls0 = [_rows(a.computeClassTransport(1)), _rows(a.computeClassTracerTransport(1))]
    joint0 = [_rows(a.computeJointClassTransport(1, carry=c)) for c in (False, True)]
    for f in (a, b):
        _set_thickness(f, real, grid, resident, thick)
    want_all, want_tr = _rows(b.computeAll()), _rows(b.computeTracerAll())
    first = _gc(a, 1, True)
    for t in (1, 0, 2):
        assert a.computeFlux(t) == b.computeFlux(t)
        tr = _rows(a.computeTracerFlux(t))
        planes = _resident(a)
        _gc(a, (t + 1) % NT), _gc(a, t, True), _gc(a, t)
        assert numpy.array_equal(_row(a), _row(b)) and numpy.array_equal(_row(a), want_all[t])
        for k, (x, y, z) in enumerate(zip(_resident(a), planes, _resident(b))):
            assert numpy.array_equal(x, y), (t, k)
            assert k == 3 or numpy.array_equal(x, z), (t, k)        # (b's running max has seen every step)
        assert numpy.array_equal(_rows(a.computeTracerFlux(t)), tr) and numpy.array_equal(tr, want_tr[t])
        assert a.computeFlux(t) == b.computeFlux(t)
    _gc(a, 0)
    assert numpy.array_equal(_rows(a.computeAll()), want_all)
    _gc(a, 2, True)
    assert numpy.array_equal(_rows(a.computeAll()), want_all)           # a replayed pass where there is one
    assert numpy.array_equal(_rows(a.computeTracerAll()), want_tr)
    assert _same_bits(_gc(a, 1, True), first)
    if thick != 'scalar':
        with pytest.raises(RuntimeError, match='per-cell thicknesses'):
            a.computeClassTransport(1)
        a.setCellThickness(None, None)
    assert _same_bits(_rows(a.computeClassTransport(1)), cls0[0])
    assert _same_bits(_rows(a.computeClassTracerTransport(1)), cls0[1])
    for c in (False, True):
        assert _same_bits(_rows(a.computeJointClassTransport(1, carry=c)), joint0[c])


def test_joint_then_gross_classes_then_joint_on_one_handle_equal_fresh_handles():
    """the term table, the block flags and the run sums are shared with the joint classes and sized by the records, the owned
    levels and the rows: joint -> gross class -> joint, each with other edges, more levels and the other dtype, give the bits
    of a fresh handle that makes that call alone"""
    from test_gpu_reuse import TRANSECTS
    from test_gpu_reuse_products import ProductHandle
    ny, nx, nt = 24, 40, 2

    def state(nz, dtype, seed, ea, eb, ec):
        shape = (nt, nz, ny, nx)
        u, v = gross_velocities(dtype, shape, seed=seed)
        rng = numpy.random.default_rng(seed + 1)
        A = (5. + 2. * rng.standard_normal(shape)).astype(dtype)
        B = (5. + rng.standard_normal(shape)).astype(dtype)
        A[:, :, 3:6, 5:9] = numpy.nan
        e3 = gross_thickness(dtype, shape, seed=seed + 2)
        return dict(nz=nz, u=u, v=v, A=A, B=B, e3=e3, ea=ea, eb=eb, ec=ec)

    def apply(h, s, first):
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
        h.call('set_joint_class_edges', s['ea'].ctypes.data_as(dp), s['ea'].size, s['eb'].ctypes.data_as(dp), s['eb'].size)
        h.set_class_edges(s['ec'])

    def joint(h, s):
        out = []
        for carry in (0, 1):
            r = numpy.full(((s['ea'].size + 2) * (s['eb'].size + 2), h.rowlen()), numpy.nan)
            h.call('compute_joint_class_transport', 1, carry, r.ctypes.data_as(dp))
            out.append(r)
        return numpy.array(out)

    def gross(h, s, cell):
        h.set_cell_thickness(*(s['e3'] if cell else (None, None)), True, THFILL if cell else None)
        out = []
        for carry in (0, 1):
            r = numpy.full((2 * (s['ec'].size + 2), h.rowlen()), numpy.nan)
            h.call('compute_gross_class_transport', 1, carry, r.ctypes.data_as(dp))
            out.append(r)
        h.set_cell_thickness(None, None, True, None)
        return numpy.array(out)

    lin = numpy.linspace
    states = [state(3, numpy.float64, 71, lin(3., 7., 2), lin(4., 6., 3), lin(3., 7., 5)),
              state(7, numpy.float32, 73, lin(1., 9., 33), lin(3., 7., 9), lin(3., 7., 40)),        # more levels, more rows
              state(5, numpy.float64, 79, lin(2., 8., 4), lin(4., 6., 2), lin(3., 7., 1025))]      # fewer levels, 2054 rows
    h = ProductHandle()
    for k, s in enumerate(states):
        apply(h, s, k == 0)
        got = [joint(h, s), gross(h, s, False), gross(h, s, True), joint(h, s)]
        want = []
        for call in (lambda x: joint(x, s), lambda x: gross(x, s, False), lambda x: gross(x, s, True)):
            fresh = ProductHandle()
            apply(fresh, s, True)
            want.append(call(fresh))
        for g, w, what in zip(got, want + want[:1], ('joint', 'gross class', 'gross class, cell thickness', 'joint again')):
            assert numpy.isfinite(g).all() and numpy.abs(g).max() > 0, (k, what)
            assert _same_bits(g, w), (k, what)
        assert not numpy.array_equal(got[1], got[2])


def test_the_thickness_weighted_mean_state_gives_the_rows_of_its_arrays():
    """timeMean(thicknessWeighted=True) always carries a cell thickness: the net class forms refuse its Field, this one gives
    the rows of a Field built from the same mean arrays"""
    real, grid = 'float32', GRIDS[1]
    src = _make(real, grid, True, sverdrup=True)
    _set_thickness(src, real, grid, True, 'timevarying')
    _configure(src, real, grid, True, True)
    edges = _edges(16, SIG0, SIGS)
    src.setClassEdges(edges)
    mean = _quiet(src.timeMean, None, thicknessWeighted=True)
    assert mean.nt == 1 and mean._e3 is not None and numpy.array_equal(mean._class_edges, edges)
    with pytest.raises(RuntimeError, match='per-cell thicknesses'):
        mean.computeClassTransport(0)
    fill = mean._uv_markers[0]
    blon, blat = _case(real, grid)[:2]
    want = _field(blon, blat, DB, mean._uv[0], mean._uv[1], [transect_xyz(s) for s in LINES], True,
                  fill_value=fill, readback=False)
    tr, ct = mean._tracer, mean._class_tracer
    want.setTracer(tr['keep'], fill_value=None if tr['fill'] != tr['fill'] else tr['fill'], reference=REF)
    want.setClassTracer(ct['keep'], fill_value=None if ct['fill'] != ct['fill'] else ct['fill'])
    want.setCellThickness(*mean._e3['arrays'])
    want.setClassEdges(edges)
    for carry in (False, True):
        got = _gc(mean, 0, carry)
        assert numpy.abs(got[0]).max() > 0 and numpy.abs(got[1]).max() > 0
        assert _same_bits(got, _gc(want, 0, carry)), carry
    # MOC(sigma) of the thickness-weighted mean state: P + N, accumulated over the classes
    from nemoflux_amd.field import Field
    tot = mean.computeGrossClassTransport(0)[0]
    psi = Field.classStreamfunction(tot[0] + tot[1])
    assert psi.shape == (16, len(LINES)) and numpy.isfinite(psi).all()


def test_the_refusals_have_the_siblings_words():
    from nemoflux_amd._lib import lib
    real, grid = 'float64', GRIDS[0]
    f = _make(real, grid, True)
    for carry in (False, True):
        with pytest.raises(RuntimeError, match='setClassEdges first'):
            f.computeGrossClassTransport(0, carry=carry)
    f.setClassEdges(numpy.array([1., 2.]))
    for carry in (False, True):
        with pytest.raises(RuntimeError, match='setTracer first'):
            f.computeGrossClassTransport(0, carry=carry)
    host = numpy.zeros((2, 4, f._rowlen))
    for name, args in (('nf_field_compute_class_transport', (0,)), ('nf_field_compute_gross_class_transport', (0, 0))):
        assert getattr(lib, name)(ctypes.byref(f._h), *args, host.ctypes.data_as(dp)) == 2
        assert (name + ': set_tracer first') in lib.nf_last_error().decode()
    g = _make(real, grid, True)
    _configure(g, real, grid, True, False)
    assert lib.nf_field_compute_gross_class_transport(ctypes.byref(g._h), 0, 0, host.ctypes.data_as(dp)) == 2
    assert 'nf_field_compute_gross_class_transport: set_class_edges first' in lib.nf_last_error().decode()
    g.setClassEdges(numpy.array([3., 5.]))
    assert lib.nf_field_compute_gross_class_transport(ctypes.byref(g._h), NT, 0, host.ctypes.data_as(dp)) == 1
    assert b'time index' in lib.nf_last_error()
    assert lib.nf_field_compute_gross_class_transport(ctypes.byref(g._h), 0, 2, host.ctypes.data_as(dp)) == 1
    assert b'carry must be 0 or 1' in lib.nf_last_error() and not host.any()
    assert numpy.abs(_gc(g, 0)).max() > 0
    # a cell thickness: this call takes it, the net class form still refuses
    _set_thickness(g, real, grid, True, 'static')
    assert numpy.abs(_gc(g, 0, True)).max() > 0
    with pytest.raises(RuntimeError, match='does not take per-cell thicknesses yet'):
        g.computeClassTransport(0)
    with pytest.raises(RuntimeError, match='does not take per-cell thicknesses yet'):
        g.computeClassTracerTransport(0)


# ---- 5. files and the command line -----------------------------------------------------------------------------------------
@pytest.mark.parametrize('carry', [False, True], ids=['volume', 'carried'])
@pytest.mark.parametrize('cell', [False, True], ids=['scalar', 'cell'])
def test_fluxplot_gross_classes_is_the_field_table(tmp_path, carry, cell):
    from nemoflux_amd import fluxplot
    from nemoflux_amd.field import Field
    real, grid = 'float32', GRIDS[0]
    nx, ny = grid
    blon, blat = _case(real, grid)[:2]
    u, v = _uv(real, grid)
    tau, sig = _tau(real, grid), _sigma(real, grid)
    e3u, e3v = gross_thickness(real, (NT, NZ, ny, nx), seed=5)
    paths = {k: str(tmp_path / f'{k}.npz') for k in 'TUVS'}
    fv = lambda name, a, b: {f'_FillValue_{name}': numpy.array(a), f'_missing_value_{name}': numpy.array(b)}   # noqa: E731
    numpy.savez(paths['T'], bounds_lon=blon, bounds_lat=blat, deptht_bounds=DB, thetao=tau, **fv('thetao', TFILL, TMISSING))
    numpy.savez(paths['S'], sigma0=sig, **fv('sigma0', SFILL, SMISSING))
    numpy.savez(paths['U'], uo=u, e3u=e3u, **fv('uo', FILL, MISSING), **fv('e3u', THFILL, THMISSING))
    numpy.savez(paths['V'], vo=v, e3v=e3v, **fv('vo', FILL, MISSING), **fv('e3v', THFILL, THMISSING))
    edges = _edges(3, SIG0, SIGS)
    lines = '[' + T_OPEN + '],[' + T_SEAM + ']'
    out = str(tmp_path / 'gross_classes.csv')
    kw = dict(tFile=paths['T'], uFile=paths['U'], vFile=paths['V'], tracer='sigma0', tracerFile=paths['S'],
              grossClasses=','.join(repr(float(e)) for e in edges))
    if carry:
        kw.update(carry='thetao', carryRef=1.5, carryScale=4.1e-3)
    if cell:
        kw.update(cellThickness=True)
    totals = _quiet(fluxplot.main, lonLatPoints=lines, output=out, sverdrup=True, **kw)
    mem = _field(blon, blat, DB, u, v, fluxplot.readTargets(lines)[0], True, fill_value=FILL, missing_value=MISSING,
                 readback=False)
    if carry:
        mem.setTracer(tau, fill_value=TFILL, missing_value=TMISSING, reference=1.5)
        mem.setClassTracer(sig, fill_value=SFILL, missing_value=SMISSING)
    else:
        mem.setTracer(sig, fill_value=SFILL, missing_value=SMISSING)
    if cell:
        mem.setCellThickness(e3u, e3v, fill_value=THFILL, missing_value=THMISSING)
    mem.setClassEdges(edges)
    with open(out) as fh:
        text = fh.read().splitlines()
    assert text[0] == ('# gross transport of thetao by sigma0 class [thetao x Sv x 0.0041]' if carry
                       else '# gross water flow by sigma0 class [Sv]')
    assert text[1] == 'time,transect,lower,upper,inflow,outflow,net'
    body = [ln.split(',') for ln in text[2:]]
    nrows = edges.size + 2
    assert totals.shape == (NT, 2, nrows, 2) and len(body) == NT * 2 * nrows
    bounds = [(-numpy.inf, edges[0])] + list(zip(edges[:-1], edges[1:])) + [(edges[-1], numpy.inf)]
    scale = 4.1e-3 if carry else 1.0
    for t in range(NT):
        want = mem.computeGrossClassTransport(t, carry=carry)[0] * scale
        assert _same_bits(totals[t], want) and numpy.abs(want[0]).max() > 0 and numpy.abs(want[1]).max() > 0
        for p in range(2):
            for k in range(nrows):
                ln = body[(t * 2 + p) * nrows + k]
                assert ln[1] == f'line{p}'
                if k < nrows - 1:
                    assert (float(ln[2]), float(ln[3])) == bounds[k]
                else:
                    assert numpy.isnan(float(ln[2])) and numpy.isnan(float(ln[3]))
                row = [want[0, k, p], want[1, k, p], want[0, k, p] + want[1, k, p]]
                assert numpy.allclose([float(x) for x in ln[4:]], row, rtol=1e-14, atol=1e-300)
    if not carry:
        assert (totals[:, 0] >= 0).all() and (totals[:, 1] <= 0).all()
        assert numpy.array_equal(Field.grossTransport(totals[0]), totals[0].sum(axis=1))
