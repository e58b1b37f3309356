"""Conservative (piecewise-linear) remapping of the class transport on the GPU (Field.computeClassRemap,
nf_field_compute_class_remap, fluxplot --remap linear).  Every value of every row in all three forms -- volume, carried tracer
that is the class field, carried tracer with a class field of its own -- is checked against the float64 / long-double
restatement of the definition in tests/class_remap_reference.py to 1e-12 x sum |share| of that value (the A7 bar of
docs/PARITY.md), no row or column left out; anchored bit for bit (a class field constant in z gives the rows of the step rule;
the level index with edges at the half-integers gives the profile rows; negated / doubled uo, vo negate / double the rows;
tau = ref + 1 gives the volume form; every class_window, out= and host inputs give the same bits); a closed form that shares
nothing with the reference; the sum over the rows against the sum over z of the profile rows; two sharded halves against the
unsharded rows; the refusals; class -> remap -> joint -> remap on one handle against fresh handles; fluxplot --remap from files.

Grids 72 x 36 x 7 x 3 and 73 x 37 x 7 x 3 with the three transects of tests/test_gpu_gross_classes.py (one across the periodic
seam; 265 to 325 records: two blocks, the second one short); seven levels leave a tail behind both batch lengths of the kernel.
The class field lies on a 2^-10 lattice in [-2, 32] and so do the class edges, so that lo == hi, interface values exactly on an
edge and zero-width rows really occur; it has NaN, both of its markers and, where it is not carried, +-inf.

The closed form.  Class field = level index, edges at the integers 0 .. nz - 1 (n = nz).  The interfaces of level z are
z - 1/2 and z + 1/2, except g_up = 0 for level 0 and g_dn = nz - 1 for the last level (there is no level beyond: the
definition takes f_z).  So level 0, [0, 1/2], lies inside row 1 and goes to it whole; an inner level z gives half to row z and
half to row z + 1; the last level, [nz - 3/2, nz - 1], goes whole to row nz - 1 and its zero-width share of row n is nothing:
    row 1 = P_0 + P_1 / 2;   row k = P_{k-1} / 2 + P_k / 2 for 2 <= k <= nz - 2;   row nz - 1 = P_{nz-2} / 2 + P_{nz-1};
    rows 0, n and n + 1 are exactly +0.0.
(The issue's sketch of this check gave rows 1 and n half a level each; that contradicts its own definition of the end
interfaces and its conservation check -- half of level 0 would be lost -- so the end rows here follow the definition.)

Measured on an MI355X: see the figures printed by each test; docs/PARITY.md quotes the worst."""
import contextlib
import ctypes

import numpy
import pytest

from class_remap_reference import ClassRemapReference
from gpu_helpers import _field, _on, _quiet, _rows, _same_bits
from gross_reference import array_values, gross_velocities
from test_gpu_cellthick import BAR, FILL, MISSING, T_OPEN, T_SEAM, T_TRI, TFILL, TMISSING, _case
from test_gpu_gross import DB, GRIDS, NT, NZ, REF, _make as _make_gross, _set_thickness, _tau, _uv

pytestmark = pytest.mark.gpu

LINES = [T_OPEN, T_TRI, T_SEAM]
SFILL, SMISSING = -8888., 5.e15
EDGES = {2: numpy.array([10., 20.]), 3: numpy.array([8., 16., 24.]), 16: 2. * numpy.arange(16), 1025: numpy.arange(1025) / 32.}
dp = ctypes.POINTER(ctypes.c_double)
_LAT = {}
WORST = {'reference': 0.0}


def _lattice(real, grid, own):
    """The class field: values on a 2^-10 lattice in [-2, 32] that grow with z, so that a layer spans up to ~200 of the 1025
    classes; columns that are constant in z (lo == hi); values on an edge of every edge count; NaN and both markers -- the
    tracer's (own = False: the field is the carried tracer too) or its own with +-inf as well (own = True)"""
    if (real, grid, own) not in _LAT:
        nx, ny = grid
        rng = numpy.random.default_rng(17 + own)
        dt = numpy.dtype(real).type
        shape = (NT, NZ, ny, nx)
        x = rng.integers(0, 6 * 1024, shape) / 1024. + 4.5 * numpy.arange(NZ)[None, :, None, None] - 2.
        x = numpy.clip(x, -2., 32.).astype(real)
        x[:, :, ::3, ::4] = x[:, 3:4, ::3, ::4]                 # constant in z
        x[rng.random(shape) < 0.05] = dt(16.)                   # an edge of all four edge sets
        marks = (SFILL, SMISSING, numpy.inf, -numpy.inf) if own else (TFILL, TMISSING)
        for m in marks + (numpy.nan,):
            x[rng.random(shape) < 0.03] = dt(m)
        x[:, :, 12:15, 40:50] = dt(marks[0])                    # a block of land
        _LAT[real, grid, own] = x
    return _LAT[real, grid, own]


def _make(real, grid, resident, **kw):
    return _make_gross(real, grid, resident, lines=LINES, **kw)


def _configure(f, real, grid, resident, two, wrap=True, ref=REF):
    """two = False: the lattice is the tracer, carried and class field at once; True: it is the class tracer of the tracer of
    tests/test_gpu_gross.py.  Returns the arrays of the reference and the class markers."""
    if not two:
        lat = _lattice(real, grid, False)
        f.setTracer(_on(lat, resident), fill_value=TFILL, missing_value=TMISSING, reference=ref, wrapX=wrap)
        return {'tracer': lat, 'class': lat}, (TFILL, TMISSING)
    tau, lat = _tau(real, grid), _lattice(real, grid, True)
    f.setTracer(_on(tau, resident), fill_value=TFILL, missing_value=TMISSING, reference=ref, wrapX=wrap)
    f.setClassTracer(_on(lat, resident), fill_value=SFILL, missing_value=SMISSING)
    return {'tracer': tau, 'class': lat}, (SFILL, SMISSING)


def _rm(f, t, carry=False, **kw):
    """(nedges + 2, row_length): [segments | transects] rows"""
    return _rows(f.computeClassRemap(t, carry=carry, **kw))


def _reference(f, class_markers, wrap=True, ref=REF, sverdrup=False):
    ce, w, sg = f.getWeights()
    return ClassRemapReference(ce, w, sg, f.arcLengths, f.thickness, f._tr_off, f.nx, f.ny, uv_markers=(FILL, MISSING),
                               tracer_markers=(TFILL, TMISSING), class_markers=class_markers, reference=ref, wrap=wrap,
                               sverdrup=sverdrup)


def _close(got, want, mag, label):
    assert got.shape == want.shape == mag.shape, label
    err = numpy.abs(got - want)
    worst = float((err / numpy.maximum(mag, 1e-300)).max())
    print(f'{label}: max |err| / sum |share| = {worst:.3g}')
    assert numpy.all(err <= BAR * mag), (label, worst)
    return worst


@contextlib.contextmanager
def _window(w):
    from nemoflux_amd._lib import lib, check
    check(lib.nf_tuning_set(b'class_window', int(w)))
    try:
        yield
    finally:
        check(lib.nf_tuning_set(b'class_window', 32))


def _level_field(real, grid):
    nx, ny = grid
    return numpy.ascontiguousarray(numpy.broadcast_to(numpy.arange(NZ, dtype=real)[None, :, None, None], (NT, NZ, ny, nx)))


def _profile(f, t, carry):
    return _rows((f.computeTracerProfile if carry else f.computeFluxProfile)(t))


# ---- 1. against the reference ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize('wrap', [True, False], ids=['wrap-sv', 'nowrap-m2'])
@pytest.mark.parametrize('resident', [True, False], ids=['hbm', 'host'])
@pytest.mark.parametrize('grid', GRIDS, ids=lambda g: f'{g[0]}x{g[1]}')
@pytest.mark.parametrize('real', ['float64', 'float32'])
def test_against_the_reference(real, grid, resident, wrap):
    """volume, carried-one and carried-two forms; every edge count, each on one of the steps"""
    u, v = _uv(real, grid)
    dt = u.dtype.type
    assert numpy.isnan(v).any() and (u == dt(FILL)).any() and (u == dt(MISSING)).any()
    seen_no_value = seen_spread = False
    for two in (False, True):
        f = _make(real, grid, resident, sverdrup=wrap)
        ce = f.getWeights()[0]
        assert ce.size > 256 and (ce // 4 % f.nx == f.nx - 1).any()        # two blocks; the seam: east faces of the last column
        arrays = {'uo': u, 'vo': v}
        more, class_markers = _configure(f, real, grid, resident, two, wrap=wrap)
        arrays.update(more)
        cls = arrays['class']
        assert numpy.isnan(cls).any() and (cls == dt(class_markers[0])).any() and (cls == dt(class_markers[1])).any()
        assert not two or (numpy.isposinf(cls).any() and numpy.isneginf(cls).any())
        r = _reference(f, class_markers, wrap=wrap, sverdrup=wrap)
        for k, (n, edges) in enumerate(EDGES.items()):
            t = k % NT
            f.setClassEdges(edges)
            want = r.remap_step(array_values(arrays, t), edges)
            vol, car = _rm(f, t), _rm(f, t, carry=True)
            assert vol.shape == car.shape == (n + 2, f._rowlen)
            label = f'{"two" if two else "one"} n={n} t={t}'
            for got, nm in ((vol, 'volume'), (car, 'carried')):
                WORST['reference'] = max(WORST['reference'], _close(got, *want[nm], f'{nm} {label}'))
            seen_no_value = seen_no_value or want['volume'][1][n + 1].max() > 0
            seen_spread = seen_spread or (n == 1025 and want['rows_per_term'] > 20)
            print(f'{label}: {want["rows_per_term"]:.1f} rows per term, {want["spread_terms"]} terms spread')
    assert seen_no_value, 'the row of the faces without a class value has terms'
    assert seen_spread, 'with 1025 edges a term is spread over many rows'
    print(f'worst so far against the reference: {WORST["reference"]:.3g}')


# ---- 2. bit-for-bit identities ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize('resident', [True, False], ids=['hbm', 'host'])
@pytest.mark.parametrize('grid', GRIDS, ids=lambda g: f'{g[0]}x{g[1]}')
@pytest.mark.parametrize('real', ['float64', 'float32'])
def test_a_class_field_constant_in_z_gives_the_rows_of_the_step_rule(real, grid, resident):
    """g_up == g_dn == f_z exactly (0.5 (f + f) = f), or the face has no value at any level: every term goes whole to the row
    the step rule sends it to, in the same order"""
    for two in (False, True):
        lat = _lattice(real, grid, two)
        flat = numpy.ascontiguousarray(numpy.broadcast_to(lat[:, 2:3], lat.shape))
        f = _make(real, grid, resident, sverdrup=True)
        if two:
            f.setTracer(_on(_tau(real, grid), resident), fill_value=TFILL, missing_value=TMISSING, reference=REF)
            f.setClassTracer(_on(flat, resident), fill_value=SFILL, missing_value=SMISSING)
        else:
            f.setTracer(_on(flat, resident), fill_value=TFILL, missing_value=TMISSING, reference=REF)
        for n in (3, 1025):
            f.setClassEdges(EDGES[n])
            for t in range(NT):
                want_v, want_c = _rows(f.computeClassTransport(t)), _rows(f.computeClassTracerTransport(t))
                assert (numpy.abs(want_v).max(axis=1) > 0).sum() >= 3 and numpy.abs(want_c).max() > 0
                assert numpy.array_equal(_rm(f, t), want_v), (two, n, t)
                assert numpy.array_equal(_rm(f, t, carry=True), want_c), (two, n, t)


@pytest.mark.parametrize('resident', [True, False], ids=['hbm', 'host'])
@pytest.mark.parametrize('grid', GRIDS, ids=lambda g: f'{g[0]}x{g[1]}')
@pytest.mark.parametrize('real', ['float64', 'float32'])
def test_one_class_per_level_gives_the_profile_rows(real, grid, resident):
    """class field = level index, edges at the half-integers -0.5 .. nz - 0.5: the interfaces of level z are edges (or z itself
    at the two ends), so its interval lies in row z + 1 -- fraction 1 / 1, or a half over a half -- and the zero-width share of
    the next row is nothing: row z + 1 holds exactly the terms of level z, added in the order of the profile kernel"""
    level = _level_field(real, grid)
    edges = numpy.arange(NZ + 1) - 0.5
    f = _make(real, grid, resident, sverdrup=True)
    f.setClassEdges(edges)
    f.setTracer(_on(_tau(real, grid), resident), fill_value=TFILL, missing_value=TMISSING, reference=REF)
    f.setClassTracer(_on(level, resident))
    for two in (True, False):
        if not two:
            f.setClassTracer(None)
            f.setTracer(_on(level, resident), reference=2.0)
        for t in range(NT):
            for carry in (False, True):
                got, want = _rm(f, t, carry), _profile(f, t, carry)
                assert got.shape == (NZ + 3, f._rowlen) and (numpy.abs(want).max(axis=1) > 0).sum() >= NZ - 1   # (tf == 0 on level 2)
                assert numpy.array_equal(got[1:NZ + 1], want), (two, t, carry)
                assert not got[[0, NZ + 1, NZ + 2]].any()


@pytest.mark.parametrize('grid', GRIDS, ids=lambda g: f'{g[0]}x{g[1]}')
@pytest.mark.parametrize('real', ['float64', 'float32'])
def test_negated_and_doubled_velocities_negate_and_double_the_rows(real, grid):
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
            f.setClassEdges(EDGES[1025])
        a, neg, dbl = fields
        for t in range(NT):
            for carry in (False, True):
                rows = _rm(a, t, carry)
                assert (numpy.abs(rows).max(axis=1) > 0).sum() > 500
                assert numpy.array_equal(_rm(neg, t, carry), -rows), (two, t, carry)
                assert numpy.array_equal(_rm(dbl, t, carry), 2. * rows), (two, t, carry)


@pytest.mark.parametrize('grid', GRIDS, ids=lambda g: f'{g[0]}x{g[1]}')
@pytest.mark.parametrize('real', ['float64', 'float32'])
def test_tracer_one_above_the_reference_is_carried_like_the_water(real, grid):
    """tau == ref + 1 everywhere: tf == 1 exactly at every face that has a value, so the carried rows are the volume rows.
    With wrapX only the north faces of the last row have no value, and no line comes near it."""
    resident = grid == GRIDS[1]
    nx, ny = grid
    tau = numpy.full((NT, NZ, ny, nx), 8., real)
    f = _make(real, grid, resident)
    assert (f.getWeights()[0] // 4 // nx).max() < ny - 1
    f.setTracer(_on(tau, resident), reference=7.0)
    f.setClassTracer(_on(_lattice(real, grid, True), resident), fill_value=SFILL, missing_value=SMISSING)
    f.setClassEdges(EDGES[1025])
    for t in range(NT):
        vol = _rm(f, t)
        assert (numpy.abs(vol).max(axis=1) > 0).sum() > 500
        assert numpy.array_equal(_rm(f, t, carry=True), vol), t
    f.setTracer(_on(tau, resident), reference=6.0)                 # tf == 2: exactly twice
    assert numpy.array_equal(_rm(f, 1, carry=True), 2. * _rm(f, 1))
    f.setClassTracer(None)                                         # the tracer is the class field: everything in one row
    f.setClassEdges(numpy.array([7.5, 8.5]))
    f.setTracer(_on(tau, resident), reference=7.0)
    vol = _rm(f, 0)
    assert numpy.abs(vol[1]).max() > 0 and not vol[[0, 2, 3]].any()
    assert numpy.array_equal(_rm(f, 0, carry=True), vol)


@pytest.mark.parametrize('real', ['float64', 'float32'])
def test_same_bits_for_every_window_home_and_out(real):
    import torch
    grid = GRIDS[1]
    fields = []
    for resident in (True, False):
        f = _make(real, grid, resident)
        _configure(f, real, grid, resident, True)
        f.setClassEdges(2. * numpy.arange(17))                     # 19 rows: one window of 32, four of 5, 19 of 1
        fields.append(f)
    f, host = fields
    shape = (19, f._rowlen)
    for t in (2, 0):
        for carry in (False, True):
            want = _rm(f, t, carry)
            assert (numpy.abs(want).max(axis=1) > 0).sum() > 10
            for window in (1, 5, 32):
                with _window(window):
                    assert _same_bits(_rm(f, t, carry), want), (t, carry, window)
            out = torch.full(shape, numpy.nan, dtype=torch.float64, device='cuda')
            assert _same_bits(_rm(f, t, carry, out=out), want)
            assert _same_bits(out.cpu().numpy(), want)
            assert _same_bits(_rm(host, t, carry), want)               # host-resident inputs, staged
            out.fill_(numpy.nan)
            assert _same_bits(_rm(host, t, carry, out=out), want)
    for bad in (torch.zeros(shape, dtype=torch.float32, device='cuda'),
                torch.zeros((shape[0] + 1, shape[1]), dtype=torch.float64, device='cuda'), torch.zeros(shape, dtype=torch.float64)):
        with pytest.raises(RuntimeError, match='out must be'):
            f.computeClassRemap(0, out=bad)


# ---- 3. to the bar ---------------------------------------------------------------------------------------------------------
def _check(got, want, mag, label):
    err = numpy.abs(got - want)
    worst = float((err / numpy.maximum(mag, 1e-300)).max())
    print(f'{label}: max |err| / sum |terms| = {worst:.3g}')
    assert want.shape == got.shape == mag.shape and numpy.abs(want).max() > 0 and numpy.all(err <= BAR * mag), (label, worst)


@pytest.mark.parametrize('resident', [True, False], ids=['hbm', 'host'])
@pytest.mark.parametrize('grid', GRIDS, ids=lambda g: f'{g[0]}x{g[1]}')
@pytest.mark.parametrize('real', ['float64', 'float32'])
def test_the_closed_form_of_the_level_index_between_integer_edges(real, grid, resident):
    """the module docstring has the derivation; nothing here comes from the reference but sum |terms| of the profile rows"""
    level = _level_field(real, grid)
    edges = numpy.arange(NZ, dtype=numpy.float64)
    n = NZ
    u, v = _uv(real, grid)
    f = _make(real, grid, resident, sverdrup=True)
    f.setClassEdges(edges)
    tau = _tau(real, grid)
    f.setTracer(_on(tau, resident), fill_value=TFILL, missing_value=TMISSING, reference=REF)
    f.setClassTracer(_on(level, resident))
    r = _reference(f, ())
    for t in range(NT):
        mags = r.step(array_values({'uo': u, 'vo': v, 'tracer': tau}, t))
        for carry, nm in ((False, 'volume_profile'), (True, 'tracer_profile')):
            got, P, M = _rm(f, t, carry), _profile(f, t, carry), mags[nm][1]
            assert got.shape == (n + 2, f._rowlen)
            half = lambda k: 0.5 * P[k]   # noqa: E731
            _check(got[1], P[0] + half(1), M[0] + M[1], f'row 1 {nm} t={t}')
            for k in range(2, n - 1):
                _check(got[k], half(k - 1) + half(k), M[k - 1] + M[k], f'row {k} {nm} t={t}')
            _check(got[n - 1], half(n - 2) + P[n - 1], M[n - 2] + M[n - 1], f'row {n - 1} {nm} t={t}')
            assert not got[[0, n, n + 1]].view(numpy.uint64).any(), (nm, t)          # exactly +0.0


@pytest.mark.parametrize('two', [False, True], ids=['one-tracer', 'class-tracer'])
@pytest.mark.parametrize('resident', [True, False], ids=['hbm', 'host'])
@pytest.mark.parametrize('grid', GRIDS, ids=lambda g: f'{g[0]}x{g[1]}')
@pytest.mark.parametrize('real', ['float64', 'float32'])
def test_the_rows_add_up_to_the_profile_rows(real, grid, resident, two):
    """conservation: the sum over the n + 2 rows against the sum over z of computeFluxProfile / computeTracerProfile, within
    1e-12 x the reference's sum |terms|"""
    u, v = _uv(real, grid)
    f = _make(real, grid, resident, sverdrup=True)
    arrays = {'uo': u, 'vo': v}
    more, class_markers = _configure(f, real, grid, resident, two)
    arrays.update(more)
    r = _reference(f, class_markers, sverdrup=True)
    for k, (n, edges) in enumerate(EDGES.items()):
        t = k % NT
        f.setClassEdges(edges)
        mags = r.step(array_values(arrays, t))
        for carry, nm in ((False, 'volume_profile'), (True, 'tracer_profile')):
            _check(_rm(f, t, carry).sum(axis=0), _profile(f, t, carry).sum(axis=0), mags[nm][1].sum(axis=0), f'{nm} n={n} t={t}')


@pytest.mark.parametrize('resident', [True, False], ids=['hbm', 'host'])
@pytest.mark.parametrize('real', ['float64', 'float32'])
def test_two_sharded_halves_add_up_to_the_unsharded_rows(real, resident):
    """slab ranges that cut inside a time step: the first and the last owned level read the class field one level beyond the
    cut -- in place in HBM, staged with the owned levels from the host -- so every term is the unsharded one and the halves add
    up to the unsharded rows up to rounding; a step that a rank does not touch gives exact zeros"""
    from nemoflux_amd.dist import slab_range
    grid, world = GRIDS[1], 2
    u, v = _uv(real, grid)
    arrays = {'uo': u, 'vo': v}
    made = {}

    def make(**kw):
        f = _make(real, grid, resident, **kw)
        more, made['markers'] = _configure(f, real, grid, resident, True)
        arrays.update(more)
        f.setClassEdges(EDGES[1025])
        return f

    full = make()
    r = _reference(full, made['markers'])
    want = numpy.array([[_rm(full, t, carry) for carry in (False, True)] for t in range(NT)])
    acc = numpy.zeros_like(want)
    cut_inside = untouched = False
    for rank in range(world):
        sr = slab_range(NT, NZ, rank, world)
        cut_inside = cut_inside or sr[0] % NZ != 0
        part = make(slab_range=sr)
        for t in range(NT):
            owns = min(sr[1], (t + 1) * NZ) > max(sr[0], t * NZ)
            for k, carry in enumerate((False, True)):
                got = _rm(part, t, carry)
                if not owns:
                    untouched = True
                    assert not got.view(numpy.uint64).any(), (rank, t, carry)
                acc[t, k] += got
    assert cut_inside and untouched
    for t in range(NT):
        ref = r.remap_step(array_values(arrays, t), EDGES[1025])
        for k, nm in enumerate(('volume', 'carried')):
            _check(acc[t, k], want[t, k], ref[nm][1], f'two halves, {nm} t={t}')


# ---- 4. state and re-use ---------------------------------------------------------------------------------------------------
def test_the_refusals_have_the_siblings_words():
    from nemoflux_amd._lib import lib
    real, grid = 'float64', GRIDS[0]
    f = _make(real, grid, True)
    for carry in (False, True):
        with pytest.raises(RuntimeError, match='setClassEdges first'):
            f.computeClassRemap(0, carry=carry)
    f.setClassEdges(numpy.array([1., 2.]))
    for carry in (False, True):
        with pytest.raises(RuntimeError, match='setTracer first'):
            f.computeClassRemap(0, carry=carry)
    host = numpy.zeros((4, f._rowlen))
    assert lib.nf_field_compute_class_remap(ctypes.byref(f._h), 0, 0, host.ctypes.data_as(dp)) == 2
    assert 'nf_field_compute_class_remap: set_tracer first' in lib.nf_last_error().decode()
    g = _make(real, grid, True)
    _configure(g, real, grid, True, False)
    assert lib.nf_field_compute_class_remap(ctypes.byref(g._h), 0, 0, host.ctypes.data_as(dp)) == 2
    assert 'nf_field_compute_class_remap: set_class_edges first' in lib.nf_last_error().decode()
    g.setClassEdges(numpy.array([3., 5.]))
    assert lib.nf_field_compute_class_remap(ctypes.byref(g._h), NT, 0, host.ctypes.data_as(dp)) == 1
    assert b'time index' in lib.nf_last_error()
    assert lib.nf_field_compute_class_remap(ctypes.byref(g._h), 0, 2, host.ctypes.data_as(dp)) == 1
    assert b'carry must be 0 or 1' in lib.nf_last_error() and not host.any()
    assert numpy.abs(_rm(g, 0)).max() > 0
    # a cell thickness: refused with the code and the words of the sibling forms
    _set_thickness(g, real, grid, True, 'static')
    messages = []
    for call in (lambda: g.computeClassRemap(0), lambda: g.computeClassRemap(0, carry=True), lambda: g.computeClassTransport(0)):
        with pytest.raises(RuntimeError, match='does not take per-cell thicknesses yet') as e:
            call()
        messages.append(str(e.value))
    assert lib.nf_field_compute_class_remap(ctypes.byref(g._h), 0, 0, host.ctypes.data_as(dp)) == 2
    words = lib.nf_last_error().decode()
    assert lib.nf_field_compute_class_transport(ctypes.byref(g._h), 0, host.ctypes.data_as(dp)) == 2
    assert words.replace('nf_field_compute_class_remap', 'nf_field_compute_class_transport') == lib.nf_last_error().decode()
    g.setCellThickness(None, None)
    assert numpy.abs(_rm(g, 0, True)).max() > 0


def test_the_call_leaves_the_other_products_alone():
    real, grid, resident = 'float64', GRIDS[0], False
    a, b = _make(real, grid, resident), _make(real, grid, resident)
    eA, eB = numpy.array([3., 4.5, 6.]), EDGES[16]
    for f in (a, b):
        _configure(f, real, grid, resident, True)
        f.setClassEdges(eB)
        f.setJointClassEdges(eA, eB)
    want_all, want_tr = _rows(b.computeAll()), _rows(b.computeTracerAll())
    for t in (1, 0, 2):
        others = lambda f: [_rows(f.computeClassTransport(t)), _rows(f.computeClassTracerTransport(t)),   # noqa: E731
                            _rows(f.computeJointClassTransport(t, carry=True)), _rows(f.computeGrossClassTransport(t)),
                            _rows(f.computeClassArea(t)), _rows(f.computeFluxProfile(t))]
        before = others(a)
        flux = a.computeFlux(t)
        first = _rm(a, t), _rm(a, (t + 1) % NT, True)
        assert a.computeFlux(t) == flux == b.computeFlux(t)
        for x, y, z in zip(others(a), before, others(b)):
            assert _same_bits(x, y) and _same_bits(x, z), t
        assert _same_bits(_rm(a, t), first[0]) and _same_bits(_rm(a, (t + 1) % NT, True), first[1])
    assert numpy.array_equal(_rows(a.computeAll()), want_all) and numpy.array_equal(_rows(a.computeTracerAll()), want_tr)


def test_class_remap_joint_remap_on_one_handle_equal_fresh_handles():
    """the run sums of the class forms are shared by the step rule and the remapping and sized by the records and the window;
    the class edges and the tracer slots are the handle's: class -> remap -> joint -> remap, then another dtype, more levels and
    other edges, give the bits of a fresh handle that makes that call alone"""
    from test_gpu_reuse import TRANSECTS
    from test_gpu_reuse_products import ProductHandle
    ny, nx, nt = 24, 40, 2

    def state(nz, dtype, seed, ea, eb, ec):
        shape = (nt, nz, ny, nx)
        u, v = gross_velocities(dtype, shape, seed=seed)
        rng = numpy.random.default_rng(seed + 1)
        A = (5. + 2. * rng.standard_normal(shape)).astype(dtype)
        B = (rng.integers(0, 2048, shape) / 512. + numpy.arange(nz)[None, :, None, None]).astype(dtype)
        A[:, :, 3:6, 5:9] = numpy.nan
        B[:, :, 10:12, 20:30] = numpy.nan
        return dict(nz=nz, u=u, v=v, A=A, B=B, ea=ea, eb=eb, ec=ec)

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

    def rows(h, name, nrows):
        """the volume and the carried form of a call that takes a carry flag"""
        out = []
        for carry in (0, 1):
            r = numpy.full((nrows, h.rowlen()), numpy.nan)
            h.call(name, 1, carry, r.ctypes.data_as(dp))
            out.append(r)
        return numpy.array(out)

    def klass(h, s):
        out = []
        for name in ('compute_class_transport', 'compute_class_tracer_transport'):
            r = numpy.full((s['ec'].size + 2, h.rowlen()), numpy.nan)
            h.call(name, 1, r.ctypes.data_as(dp))
            out.append(r)
        return numpy.array(out)

    def remap(h, s):
        return rows(h, 'compute_class_remap', s['ec'].size + 2)

    def joint(h, s):
        return rows(h, 'compute_joint_class_transport', (s['ea'].size + 2) * (s['eb'].size + 2))

    lin = numpy.linspace
    states = [state(3, numpy.float64, 71, lin(3., 7., 2), lin(1., 5., 3), lin(0., 6., 5)),
              state(7, numpy.float32, 73, lin(1., 9., 33), lin(1., 9., 9), lin(0., 10., 1025)),     # more levels, more rows
              state(5, numpy.float64, 79, lin(2., 8., 4), lin(2., 6., 2), lin(0., 8., 40))]         # fewer levels, other edges
    h = ProductHandle()
    for k, s in enumerate(states):
        apply(h, s, k == 0)
        got = [klass(h, s), remap(h, s), joint(h, s), remap(h, s), klass(h, s)]
        want = []
        for call in (klass, remap, joint):
            fresh = ProductHandle()
            apply(fresh, s, True)
            want.append(call(fresh, s))
        for g, w, what in zip(got, want + want[1::-1], ('class', 'remap', 'joint', 'remap again', 'class again')):
            assert numpy.isfinite(g).all() and numpy.abs(g).max() > 0, (k, what)
            assert _same_bits(g, w), (k, what)
        assert not numpy.array_equal(got[0], got[1])


def test_the_rows_go_into_the_class_space_helpers_and_the_time_mean():
    """classStreamfunction of the remapped rows; the Field of timeMean carries the edges and gives remapped rows of its own; a
    Sigma class field goes through the one-step buffer"""
    from nemoflux_amd.eos import Sigma
    from nemoflux_amd.field import Field
    real, grid = 'float32', GRIDS[1]
    f = _make(real, grid, True, sverdrup=True)
    _configure(f, real, grid, True, False)
    f.setClassEdges(EDGES[16])
    tot = f.computeClassRemap(0)[0]
    psi = Field.classStreamfunction(tot)
    assert psi.shape == (16, len(LINES)) and numpy.isfinite(psi).all() and numpy.abs(psi).max() > 0
    mean = _quiet(f.timeMean)
    assert mean.nt == 1 and numpy.array_equal(mean._class_edges, EDGES[16])
    rows = _rm(mean, 0, True)
    assert rows.shape == (18, f._rowlen) and numpy.isfinite(rows).all() and numpy.abs(rows).max() > 0
    # a Sigma(theta, S, pref) as the class field: the rows of the same sigma held as an array
    nx, ny = grid
    rng = numpy.random.default_rng(5)
    shape = (NT, NZ, ny, nx)
    theta = (15. - 2. * numpy.arange(NZ)[None, :, None, None] + rng.standard_normal(shape)).astype(real)
    salt = (35. + 0.3 * rng.standard_normal(shape)).astype(real)
    g = _make(real, grid, True, sverdrup=True)
    g.setTracer(Sigma(_on(theta, True), _on(salt, True), pref=0.))
    edges = numpy.linspace(24., 29., 256)
    g.setClassEdges(edges)
    got = _rm(g, 1)
    from nemoflux_amd.eos import sigma_eos80
    sig = sigma_eos80(_on(theta, True), _on(salt, True), 0.)
    k = _make(real, grid, True, sverdrup=True)
    k.setTracer(sig)
    k.setClassEdges(edges)
    assert (numpy.abs(got).max(axis=1) > 0).sum() > 50 and _same_bits(got, _rm(k, 1))


# ---- 5. files and the command line -----------------------------------------------------------------------------------------
@pytest.mark.parametrize('carry', [False, True], ids=['volume', 'carried'])
def test_fluxplot_remap_is_the_field_table(tmp_path, carry):
    from nemoflux_amd import fluxplot
    real, grid = 'float32', GRIDS[0]
    blon, blat = _case(real, grid)[:2]
    u, v = _uv(real, grid)
    tau, sig = _tau(real, grid), _lattice(real, grid, True)
    paths = {k: str(tmp_path / f'{k}.npz') for k in 'TUVS'}
    fv = lambda name, a, b: {f'_FillValue_{name}': numpy.array(a), f'_missing_value_{name}': numpy.array(b)}   # noqa: E731
    numpy.savez(paths['T'], bounds_lon=blon, bounds_lat=blat, deptht_bounds=DB, thetao=tau, **fv('thetao', TFILL, TMISSING))
    numpy.savez(paths['S'], sigma0=sig, **fv('sigma0', SFILL, SMISSING))
    numpy.savez(paths['U'], uo=u, **fv('uo', FILL, MISSING))
    numpy.savez(paths['V'], vo=v, **fv('vo', FILL, MISSING))
    edges = EDGES[16]
    lines = '[' + T_OPEN + '],[' + T_SEAM + ']'
    out = str(tmp_path / 'remap.csv')
    kw = dict(tFile=paths['T'], uFile=paths['U'], vFile=paths['V'], tracer='sigma0', tracerFile=paths['S'],
              classes=','.join(repr(float(e)) for e in edges), remap='linear')
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
    mem.setClassEdges(edges)
    with open(out) as fh:
        text = fh.read().splitlines()
    assert text[0] == ('# transport of thetao by sigma0 class [thetao x Sv x 0.0041], conservative remapping' if carry
                       else '# water flow by sigma0 class [Sv], conservative remapping')
    assert text[1] == 'time,lower,upper,line0,line1'
    assert totals.shape == (NT, edges.size + 2, 2) and len(text) == 2 + NT * (edges.size + 2)
    step = numpy.array([(mem.computeClassTracerTransport if carry else mem.computeClassTransport)(t)[0] for t in range(NT)])
    for t in range(NT):
        want = mem.computeClassRemap(t, carry=carry)[0] * (4.1e-3 if carry else 1.0)
        assert _same_bits(totals[t], want) and (numpy.abs(want).max(axis=1) > 0).sum() > 10
    assert not numpy.array_equal(totals, step * (4.1e-3 if carry else 1.0))
