"""Section area in tracer classes on the GPU (Field.computeClassArea, nf_field_compute_class_area, Field.classMeanTracer,
Field.classInterfaceDepth, Field.decomposeTracerTransportByClass, fluxplot --class-area).  Every value of A and B in both
forms -- the tracer binned by itself, a class field of its own -- each with the scalar or a per-cell thickness, is checked
against the float64 / long-double restatement of tests/class_area_reference.py to 1e-12 x the sum of |terms| of that value (the
A7 bar of docs/PARITY.md), no row or column left out; anchored bit for bit (one class per level gives the rows of
computeAreaProfile; tau = ref + 1 gives B = A; doubled velocities change nothing; a broadcast cell thickness is the scalar
form; every joint_window / joint_skip, out= and host inputs give the same bits); cross-checked against code that shares nothing
with it (P - N of computeGrossClassTransport on velocities of 1; the depth sum of computeAreaProfile); two sharded halves
against the unsharded rows; a Sigma as the class field; the interface depths and the class-space decomposition from device
rows; nothing else is disturbed, the shared term table follows joint -> class area -> gross class -> joint on one handle; the
refusals; fluxplot --class-area from files.

The inputs are those of tests/test_gpu_gross_classes.py: grids 72 x 36 x 7 x 3 and 73 x 37 x 7 x 3 with three transects (one
across the periodic seam), 265 to 325 records, two blocks of the kernel; seven levels leave a tail behind the batch of four.

Measured on an MI355X: worst |error| 4.1e-16 x sum |terms| against the reference, 5.6e-16 over every comparison of this file;
136 tests in 4.3 s."""
import ctypes

import numpy
import pytest

from class_area_reference import ClassAreaReference
from gpu_helpers import _field, _on, _quiet, _rows, _same_bits
from gross_reference import array_values, gross_thickness, gross_velocities
from test_gpu_cellthick import (BAR, FILL, MISSING, T_OPEN, T_SEAM, TFILL, THFILL, THMISSING, TMISSING, _case, _resident, _row)
from test_gpu_gross import DB, GRIDS, NT, NZ, REF, TH, _set_thickness, _tau, _uv
from test_gpu_gross_classes import (EDGE_COUNTS, LINES, SFILL, SIG0, SIGS, SMISSING, _configure, _edges, _gc, _make, _sigma)
from test_gpu_joint_classes import _skip, _window
from test_gpu_section import _area

pytestmark = pytest.mark.gpu

dp = ctypes.POINTER(ctypes.c_double)


def _ca(f, t, **kw):
    """(2, nedges + 2, row_length): A, B as [segments | transects] rows"""
    return _rows(f.computeClassArea(t, **kw))


def _reference(f, class_markers, wrap=True, ref=REF, cell_thickness=False):
    ce, w, sg = f.getWeights()
    return ClassAreaReference(ce, w, sg, f.arcLengths, f.thickness, f._tr_off, f.nx, f.ny, uv_markers=(FILL, MISSING),
                              tracer_markers=(TFILL, TMISSING), class_markers=class_markers, thick_markers=(THFILL, THMISSING),
                              reference=ref, wrap=wrap, cell_thickness=cell_thickness)


def _close(got, want, mag, label):
    assert got.shape == want.shape == mag.shape, label
    err = numpy.abs(got - want)
    worst = float((err / numpy.maximum(mag, 1e-300)).max())
    print(f'{label}: max |err| / sum |terms| = {worst:.3g}')
    assert numpy.abs(want).max() > 0 and numpy.all(err <= BAR * mag), (label, worst)


# ---- 1. against the reference ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize('thick', ['scalar', 'static', 'timevarying'])
@pytest.mark.parametrize('wrap', [True, False], ids=['wrap', 'nowrap'])
@pytest.mark.parametrize('resident', [True, False], ids=['hbm', 'host'])
@pytest.mark.parametrize('grid', GRIDS, ids=lambda g: f'{g[0]}x{g[1]}')
@pytest.mark.parametrize('real', ['float64', 'float32'])
def test_against_the_reference(real, grid, resident, wrap, thick):
    """both forms; every edge count, each on one of the steps"""
    u, v = _uv(real, grid)
    dt = u.dtype.type
    assert numpy.isnan(v).any() and (u == dt(FILL)).any() and (u == dt(MISSING)).any()
    for two in (False, True):
        f = _make(real, grid, resident, sverdrup=wrap)                    # the Sverdrup scale does not enter
        ce = f.getWeights()[0]
        assert ce.size > 256 and (ce // 4 % f.nx == f.nx - 1).any()        # the seam: east faces of the last column
        arrays = {'uo': u, 'vo': v}
        e3 = _set_thickness(f, real, grid, resident, thick)
        assert all(numpy.isnan(a).any() and (a == dt(THFILL)).any() and (a == dt(THMISSING)).any() for a in e3.values())
        arrays.update(e3)
        more, class_markers, (centre, scale) = _configure(f, real, grid, resident, two, wrap=wrap)
        arrays.update(more)
        for a, marks in ((more['tracer'], (TFILL, TMISSING)), (more['class'], class_markers)):
            assert numpy.isnan(a).any() and all((a == dt(m)).any() for m in marks)
        r = _reference(f, class_markers, wrap=wrap, cell_thickness=thick != 'scalar')
        for k, n in enumerate(EDGE_COUNTS):
            t = k % NT
            edges = _edges(n, centre, scale)
            f.setClassEdges(edges)
            want, mag = r.class_area_step(array_values(arrays, t), edges)
            got = _ca(f, t)
            assert got.shape == (2, n + 2, f._rowlen)
            _close(got, want, mag, f'{"two" if two else "one"} n={n} t={t}')
            assert (got[0] >= 0).all() and (got[1] < 0).any() and (got[1] > 0).any()
            assert (numpy.abs(got[0]).max(axis=1) > 0).sum() >= min(n, 4)
            if two:
                assert mag[0, n + 1].max() > 0 and got[0, n + 1].max() > 0, 'the row of the faces without a class value has terms'
            else:
                assert not got[:, n + 1].view(numpy.uint64).any()      # a face counts only where the class field has a value


@pytest.mark.parametrize('real', ['float64', 'float32'])
def test_a_face_value_that_is_not_finite_does_not_count(real):
    """the tracer of tests/test_gpu_section.py: +inf, and +inf beside -inf, in the carried tracer"""
    from test_gpu_section import REF as SREF, _tau as section_tau
    grid, resident = GRIDS[1], True
    tau = section_tau(real, grid)
    assert numpy.isinf(tau).any()
    u, v = _uv(real, grid)
    for cls, marks, (centre, scale) in ((None, (TFILL, TMISSING), (4.5, 0.25)), (_sigma(real, grid), (SFILL, SMISSING), (SIG0, SIGS))):
        f = _make(real, grid, resident)
        f.setTracer(_on(tau, resident), fill_value=TFILL, missing_value=TMISSING, reference=SREF)
        if cls is not None:
            f.setClassTracer(_on(cls, resident), fill_value=SFILL, missing_value=SMISSING)
        edges = _edges(16, centre, scale)
        f.setClassEdges(edges)
        r = _reference(f, marks, ref=SREF)
        arrays = {'uo': u, 'vo': v, 'tracer': tau, 'class': tau if cls is None else cls}
        for t in range(NT):
            got = _ca(f, t)
            assert numpy.isfinite(got).all()
            _close(got, *r.class_area_step(array_values(arrays, t), edges), f'inf in the tracer, class field {cls is not None} t={t}')


# ---- 2. bit-for-bit identities -------------------------------------------------------------------------------------------
@pytest.mark.parametrize('thick', ['scalar', 'static', 'timevarying'])
@pytest.mark.parametrize('grid', GRIDS, ids=lambda g: f'{g[0]}x{g[1]}')
@pytest.mark.parametrize('real', ['float64', 'float32'])
def test_one_class_per_level_gives_the_area_profile_bit_for_bit(real, grid, thick):
    """a class field equal to the level index, edges at the half-integers: row z holds exactly the terms of level z, added
    into +0.0 in the same order as computeAreaProfile adds them; the row of the faces without a class value stays +0.0"""
    resident = grid == GRIDS[0]
    nx, ny = grid
    level = numpy.ascontiguousarray(numpy.broadcast_to(numpy.arange(NZ, dtype=real)[None, :, None, None], (NT, NZ, ny, nx)))
    f = _make(real, grid, resident)
    _set_thickness(f, real, grid, resident, thick)
    f.setClassEdges(numpy.arange(NZ - 1) + 0.5)
    # the level index as the class tracer of another carried tracer, then as the one tracer, carried itself
    f.setTracer(_on(_tau(real, grid), resident), fill_value=TFILL, missing_value=TMISSING, reference=REF)
    f.setClassTracer(_on(level, resident))
    for two in (True, False):
        if not two:
            f.setClassTracer(None)
            f.setTracer(_on(level, resident), reference=2.0)
        for t in range(NT):
            got, want = _ca(f, t), _area(f, t)
            assert got.shape == (2, NZ + 1, f._rowlen) and want[0].max() > 0 and numpy.abs(want[1]).max() > 0
            assert numpy.array_equal(got[:, :NZ], want), (two, t)
            assert not got[:, NZ].view(numpy.uint64).any()


@pytest.mark.parametrize('thick', ['scalar', 'timevarying'])
@pytest.mark.parametrize('grid', GRIDS, ids=lambda g: f'{g[0]}x{g[1]}')
@pytest.mark.parametrize('real', ['float64', 'float32'])
def test_tracer_one_above_the_reference_gives_b_equal_a(real, grid, thick):
    """tau == ref + 1 everywhere, ref an integer: x - ref == 1 exactly at every face that counts"""
    resident = grid == GRIDS[1]
    nx, ny = grid
    tau = numpy.full((NT, NZ, ny, nx), 8., real)
    f = _make(real, grid, resident)
    _set_thickness(f, real, grid, resident, thick)
    f.setTracer(_on(tau, resident), reference=7.0)
    f.setClassEdges(numpy.array([7.5, 8.5]))                       # the tracer is the class field: everything in row 1
    for t in range(NT):
        a, b = _ca(f, t)
        assert a[1].max() > 0 and not a[[0, 2, 3]].any()
        assert numpy.array_equal(b, a), t
    f.setClassTracer(_on(_sigma(real, grid), resident), fill_value=SFILL, missing_value=SMISSING)     # a class field of its own
    f.setClassEdges(_edges(16, SIG0, SIGS))
    for t in range(NT):
        a, b = _ca(f, t)
        assert (a.max(axis=1) > 0).sum() > 10 and a[17].max() > 0
        assert numpy.array_equal(b, a), t
    f.setTracer(_on(tau, resident), reference=6.0)                 # x - ref == 2: exactly twice
    a, b = _ca(f, 1)
    assert numpy.array_equal(b, 2. * a)


@pytest.mark.parametrize('two', [False, True], ids=['one-tracer', 'class-tracer'])
@pytest.mark.parametrize('thick', ['scalar', 'timevarying'])
@pytest.mark.parametrize('real', ['float64', 'float32'])
def test_only_the_presence_of_the_velocities_counts(real, thick, two):
    grid = GRIDS[0]
    resident = thick == 'scalar'
    u, v = _uv(real, grid)
    dt = u.dtype.type

    def doubled(x):
        keep = numpy.isnan(x) | (x == dt(FILL)) | (x == dt(MISSING))
        return numpy.where(keep, x, dt(2) * x)

    a, b = _make(real, grid, resident), _make(real, grid, resident, u=doubled(u), v=doubled(v))
    for f in (a, b):
        _set_thickness(f, real, grid, resident, thick)
        _, _, (centre, scale) = _configure(f, real, grid, resident, two)
        f.setClassEdges(_edges(16, centre, scale))
    for t in range(NT):
        want = _ca(a, t)
        assert want[0].max() > 0 and _same_bits(_ca(b, t), want), t
        assert not numpy.array_equal(_gc(b, t), _gc(a, t))           # the transports do see the velocities


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
            want = _ca(b, t)
            assert want[0].max() > 0
            assert _same_bits(_ca(a, t), want), (two, t)
        a.setCellThickness(_on(2 * e3, resident), _on(e3, resident))
        assert not numpy.array_equal(_ca(a, 1), _ca(b, 1))
        a.setCellThickness(None, None)
        assert _same_bits(_ca(a, 1), _ca(b, 1))


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
        want = _ca(f, t)
        assert want[0].max() > 0 and numpy.abs(want[1]).max() > 0
        for window in (1, 5, 32):
            for skip in (0, 1):
                with _window(window), _skip(skip):
                    assert _same_bits(_ca(f, t), want), (t, window, skip)
        out = torch.full(shape, numpy.nan, dtype=torch.float64, device='cuda')
        assert _same_bits(_ca(f, t, out=out), want)
        assert _same_bits(out.cpu().numpy().reshape(want.shape), want)
        assert _same_bits(_ca(host, t), want)                          # host-resident inputs, staged
        out.fill_(numpy.nan)
        assert _same_bits(_ca(host, t, out=out), want)
    for bad in (torch.zeros(shape, dtype=torch.float32, device='cuda'),
                torch.zeros((shape[0] + 1, shape[1]), dtype=torch.float64, device='cuda'),
                torch.zeros((2, 18, f._rowlen), dtype=torch.float64, device='cuda'), torch.zeros(shape, dtype=torch.float64),
                torch.zeros(shape[::-1], dtype=torch.float64, device='cuda').t()):
        with pytest.raises(RuntimeError, match='out must be'):
            f.computeClassArea(0, out=bad)


@pytest.mark.parametrize('thick', ['scalar', 'timevarying'])
@pytest.mark.parametrize('real', ['float64', 'float32'])
def test_two_sharded_halves_add_up_to_the_unsharded_rows(real, thick):
    """slab ranges that cut inside a time step: a class row takes terms from the levels of both ranks, so the halves add up to
    the unsharded rows up to rounding -- within the bar on the reference's sum of |terms|; a step that a rank does not touch
    gives exact zeros"""
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
    want = numpy.array([_ca(full, t) for t in range(NT)])
    acc = numpy.zeros_like(want)
    cut_inside = untouched = False
    for rank in range(world):
        sr = slab_range(NT, NZ, rank, world)
        cut_inside = cut_inside or sr[0] % NZ != 0
        part = make(slab_range=sr)
        for t in range(NT):
            owns = min(sr[1], (t + 1) * NZ) > max(sr[0], t * NZ)
            got = _ca(part, t)
            if not owns:
                untouched = True
                assert not got.view(numpy.uint64).any(), (rank, t)
            acc[t] += got
    assert cut_inside and untouched
    for t in range(NT):
        mag = r.class_area_step(array_values(arrays, t), made['edges'])[1]
        _close(acc[t], want[t], mag, f'two halves t={t}')


# ---- 3. cross-checks that share no new code -------------------------------------------------------------------------------
@pytest.mark.parametrize('two', [False, True], ids=['one-tracer', 'class-tracer'])
@pytest.mark.parametrize('thick', ['scalar', 'timevarying'])
@pytest.mark.parametrize('grid', GRIDS, ids=lambda g: f'{g[0]}x{g[1]}')
@pytest.mark.parametrize('real', ['float64', 'float32'])
def test_gross_class_parts_of_unit_velocities_and_the_area_profile(real, grid, thick, two):
    """uo / vo replaced by 1 wherever they are present, Sverdrup off: every water term is +-|w| th arc, so P - N of
    computeGrossClassTransport is A (carry=False) and B (carry=True) -- other kernel, other operand order, hence the bar on the
    reference's sum of |terms|.  The gross form also counts the faces whose carried tracer has no value, which the area leaves
    out: the carried tracer of this test has a value everywhere (the class field keeps its NaN and markers, so the row of the
    faces without a class value is compared too).  The sum over the classes against the depth sum of computeAreaProfile, with
    the tracer that has NaN and markers."""
    resident = grid == GRIDS[0]
    u, v = _uv(real, grid)
    dt = u.dtype.type

    def ones(x):
        keep = numpy.isnan(x) | (x == dt(FILL)) | (x == dt(MISSING))
        return numpy.where(keep, x, dt(1))

    u1, v1 = ones(u), ones(v)
    nx, ny = grid
    tau = (REF + 2. * numpy.random.default_rng(17).standard_normal((NT, NZ, ny, nx))).astype(real)      # a value everywhere
    f = _make(real, grid, resident, u=u1, v=v1, sverdrup=False)
    arrays = {'uo': u1, 'vo': v1, 'tracer': tau}
    arrays.update(_set_thickness(f, real, grid, resident, thick))
    f.setTracer(_on(tau, resident), fill_value=TFILL, missing_value=TMISSING, reference=REF)
    if two:
        sig = _sigma(real, grid)
        f.setClassTracer(_on(sig, resident), fill_value=SFILL, missing_value=SMISSING)
        arrays['class'], marks, (centre, scale) = sig, (SFILL, SMISSING), (SIG0, SIGS)
    else:
        arrays['class'], marks, (centre, scale) = tau, (TFILL, TMISSING), (REF, 2.)
    edges = _edges(16, centre, scale)
    f.setClassEdges(edges)
    r = _reference(f, marks, cell_thickness=thick != 'scalar')
    for t in range(NT):
        mag = r.class_area_step(array_values(arrays, t), edges)[1]
        got = _ca(f, t)
        vol, car = _gc(f, t), _gc(f, t, carry=True)
        assert (vol[0] > 0).any() and (vol[1] < 0).any()
        _close(vol[0] - vol[1], got[0], mag[0], f'P - N, volume t={t}')
        _close(car[0] - car[1], got[1], mag[1], f'P - N, carried t={t}')
        assert not two or got[0, 17].max() > 0
    # the sum over the classes is the depth sum of the area profile: the inputs of the other tests
    g = _make(real, grid, resident)
    arrays = {'uo': u, 'vo': v}
    arrays.update(_set_thickness(g, real, grid, resident, thick))
    more, marks, (centre, scale) = _configure(g, real, grid, resident, two)
    arrays.update(more)
    edges = _edges(16, centre, scale)
    g.setClassEdges(edges)
    r = _reference(g, marks, cell_thickness=thick != 'scalar')
    for t in range(NT):
        mag = r.class_area_step(array_values(arrays, t), edges)[1]
        _close(_ca(g, t).sum(axis=1), _area(g, t).sum(axis=1), mag.sum(axis=1), f'sum over the classes t={t}')


# ---- 4. through the stack ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('pref', [0., 2000.])
@pytest.mark.parametrize('home', ['hbm', 'host'])
@pytest.mark.parametrize('real', ['float64', 'float32'])
def test_a_sigma_as_the_class_field_gives_the_rows_of_the_restatements_series(real, home, pref, tmp_path):
    from nemoflux_amd.eos import Sigma
    from test_gpu_eos import _homes, _sigma_ref
    grid = GRIDS[1]
    thetao, so, kw, arrs = _homes(real, grid, home, tmp_path)
    resident = home == 'hbm'
    sig = _sigma_ref(arrs, pref)
    ok = numpy.isfinite(sig)
    centre, scale = float(numpy.median(sig[ok])), float(sig[ok].std())
    tau = _tau(real, grid)
    f, g = _make(real, grid, resident), _make(real, grid, resident)
    for x in (f, g):
        x.setTracer(_on(tau, resident), fill_value=TFILL, missing_value=TMISSING, reference=REF)
    f.setClassTracer(Sigma(thetao, so, pref, **kw))
    g.setClassTracer(_on(sig, resident))
    for k, t in enumerate((2, 0, 1)):
        edges = _edges((2, 16, 1025)[k], centre, scale)
        for x in (f, g):
            x.setClassEdges(edges)
        want = _ca(g, t)
        assert want[0].max() > 0 and (want[0].max(axis=1) > 0).sum() >= min(edges.size, 8)
        assert numpy.array_equal(_ca(f, t), want), (k, t)
        for x in (f, g):
            _set_thickness(x, real, grid, resident, 'timevarying')
        assert numpy.array_equal(_ca(f, t), _ca(g, t)), (k, t)
        for x in (f, g):
            x.setCellThickness(None, None)
    # the Sigma as the one tracer, carried itself
    f.setClassTracer(None)
    g.setClassTracer(None)
    f.setTracer(Sigma(thetao, so, pref, **kw), reference=0.0)
    g.setTracer(_on(sig, resident), reference=0.0)
    want = _ca(g, 1)
    assert want[0].max() > 0 and numpy.array_equal(_ca(f, 1), want)


@pytest.mark.parametrize('thick', ['scalar', 'timevarying'])
@pytest.mark.parametrize('two', [False, True], ids=['one-tracer', 'class-tracer'])
@pytest.mark.parametrize('real', ['float64', 'float32'])
def test_interface_depths_and_the_decomposition_from_device_rows(real, two, thick):
    from nemoflux_amd.field import Field
    grid, resident = GRIDS[0], True
    f = _make(real, grid, resident, sverdrup=True)
    _set_thickness(f, real, grid, resident, thick)
    _, _, (centre, scale) = _configure(f, real, grid, resident, two)
    edges = _edges(16, centre, scale)
    f.setClassEdges(edges)
    for t in range(NT):
        parts = _ca(f, t)
        depth = Field.classInterfaceDepth(parts[0], _area(f, t)[0], f.bounds_depth)
        assert depth.shape == (16, f._rowlen)
        live = (parts[0, :17].sum(axis=0) > 0) & (_area(f, t)[0].sum(axis=0) > 0)
        assert live[-len(LINES):].all() and numpy.array_equal(numpy.isfinite(depth).all(axis=0), live)
        assert numpy.isnan(depth[:, ~live]).all()
        d = depth[:, live]
        assert numpy.all(numpy.diff(d, axis=0) >= 0) and d.min() >= DB[0, 0] and d.max() <= DB[-1, 1]
        assert (numpy.diff(d[:, -len(LINES):], axis=0) > 0).any()
        mean = Field.classMeanTracer(parts, REF)
        assert numpy.array_equal(numpy.isnan(mean), parts[0] == 0)
        # the decomposition in class space: closes, and its total is the tracer transport
        got = f.decomposeTracerTransportByClass(t)
        H = f.computeTracerFlux(t)[0]
        assert numpy.array_equal(got['total'], H) and got['mean'].shape == (18, len(LINES))
        if thick == 'scalar':
            V = f.computeClassTransport(t)[0]
        else:
            pn = f.computeGrossClassTransport(t)[0]
            V = pn[0] + pn[1]
        A, B = f.computeClassArea(t)[0]
        M = B.sum(axis=0) / A.sum(axis=0)
        terms = numpy.abs(H) + numpy.abs(V.sum(axis=0) * M) + (numpy.abs(V) * numpy.abs(got['mean'] - M)).sum(axis=0)
        assert numpy.abs(got['overturning']).max() > 0 and numpy.abs(got['gyre']).max() > 0
        assert numpy.all(numpy.abs(got['throughflow'] + got['overturning'] + got['gyre'] - got['total']) <= BAR * terms)
        want = Field.overturningGyre(V, (A, B), H)
        for key in want:
            assert numpy.array_equal(got[key], want[key]), key


# ---- 5. state and re-use -----------------------------------------------------------------------------------------------------
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
    first = _ca(a, 1)
    gross0 = [_gc(a, 1, c) for c in (False, True)]
    for t in (1, 0, 2):
        assert a.computeFlux(t) == b.computeFlux(t)
        tr = _rows(a.computeTracerFlux(t))
        planes = _resident(a)
        _ca(a, (t + 1) % NT), _ca(a, t)
        assert numpy.array_equal(_row(a), _row(b)) and numpy.array_equal(_row(a), want_all[t])
        for k, (x, y, z) in enumerate(zip(_resident(a), planes, _resident(b))):
            assert numpy.array_equal(x, y), (t, k)
            assert k == 3 or numpy.array_equal(x, z), (t, k)        # (b's running max has seen every step)
        assert numpy.array_equal(_rows(a.computeTracerFlux(t)), tr) and numpy.array_equal(tr, want_tr[t])
        assert a.computeFlux(t) == b.computeFlux(t)
    _ca(a, 0)
    assert numpy.array_equal(_rows(a.computeAll()), want_all)
    _ca(a, 2)
    assert numpy.array_equal(_rows(a.computeAll()), want_all)           # a replayed pass where there is one
    assert numpy.array_equal(_rows(a.computeTracerAll()), want_tr)
    assert _same_bits(_ca(a, 1), first)
    for c in (False, True):
        assert _same_bits(_gc(a, 1, c), gross0[c])
    if thick != 'scalar':
        a.setCellThickness(None, None)
    assert _same_bits(_rows(a.computeClassTransport(1)), cls0[0])
    assert _same_bits(_rows(a.computeClassTracerTransport(1)), cls0[1])
    for c in (False, True):
        assert _same_bits(_rows(a.computeJointClassTransport(1, carry=c)), joint0[c])


def test_joint_class_area_gross_class_joint_on_one_handle_equal_fresh_handles():
    """the term table, the block flags and the run sums are shared with the joint classes and the gross class transport and
    sized by the records, the owned levels and the rows -- the class area takes twice the table of the others: joint -> class
    area -> gross class -> joint, then other edges, more levels and the other dtype, give the bits of a fresh handle that makes
    that call alone"""
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
        B[:, :, 8:12, 20:30] = numpy.nan
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

    def area(h, s, cell):
        h.set_cell_thickness(*(s['e3'] if cell else (None, None)), True, THFILL if cell else None)
        r = numpy.full((2 * (s['ec'].size + 2), h.rowlen()), numpy.nan)
        h.call('compute_class_area', 1, r.ctypes.data_as(dp))
        h.set_cell_thickness(None, None, True, None)
        return r

    def gross(h, s):
        out = []
        for carry in (0, 1):
            r = numpy.full((2 * (s['ec'].size + 2), h.rowlen()), numpy.nan)
            h.call('compute_gross_class_transport', 1, carry, r.ctypes.data_as(dp))
            out.append(r)
        return numpy.array(out)

    lin = numpy.linspace
    states = [state(3, numpy.float64, 71, lin(3., 7., 2), lin(4., 6., 3), lin(3., 7., 5)),
              state(7, numpy.float32, 73, lin(1., 9., 33), lin(3., 7., 9), lin(3., 7., 40)),        # more levels, more rows
              state(5, numpy.float64, 79, lin(2., 8., 4), lin(4., 6., 2), lin(3., 7., 1025))]      # fewer levels, 2054 rows
    h = ProductHandle()
    for k, s in enumerate(states):
        apply(h, s, k == 0)
        got = [joint(h, s), area(h, s, False), area(h, s, True), gross(h, s), joint(h, s)]
        want = []
        for call in (lambda x: joint(x, s), lambda x: area(x, s, False), lambda x: area(x, s, True), lambda x: gross(x, s)):
            fresh = ProductHandle()
            apply(fresh, s, True)
            want.append(call(fresh))
        names = ('joint', 'class area', 'class area, cell thickness', 'gross class', 'joint again')
        for g, w, what in zip(got, want + want[:1], names):
            assert numpy.isfinite(g).all() and numpy.abs(g).max() > 0, (k, what)
            assert _same_bits(g, w), (k, what)
        assert not numpy.array_equal(got[1], got[2])


def test_the_refusals_have_the_siblings_words():
    from nemoflux_amd._lib import lib
    real, grid = 'float64', GRIDS[0]
    f = _make(real, grid, True)
    with pytest.raises(RuntimeError, match='setClassEdges first'):
        f.computeClassArea(0)
    with pytest.raises(RuntimeError, match='setClassEdges first'):
        f.decomposeTracerTransportByClass(0)
    f.setClassEdges(numpy.array([1., 2.]))
    with pytest.raises(RuntimeError, match='setTracer first'):
        f.computeClassArea(0)
    host = numpy.zeros((2, 4, f._rowlen))
    for name in ('nf_field_compute_class_transport', 'nf_field_compute_class_area'):
        assert getattr(lib, name)(ctypes.byref(f._h), 0, host.ctypes.data_as(dp)) == 2
        assert (name + ': set_tracer first') in lib.nf_last_error().decode()
    g = _make(real, grid, True)
    _configure(g, real, grid, True, False)
    assert lib.nf_field_compute_class_area(ctypes.byref(g._h), 0, host.ctypes.data_as(dp)) == 2
    assert 'nf_field_compute_class_area: set_class_edges first' in lib.nf_last_error().decode()
    g.setClassEdges(numpy.array([3., 5.]))
    assert lib.nf_field_compute_class_area(ctypes.byref(g._h), NT, host.ctypes.data_as(dp)) == 1
    assert b'time index' in lib.nf_last_error() and not host.any()
    assert lib.nf_field_compute_class_area(ctypes.byref(g._h), 0, None) == 1
    assert b'null' in lib.nf_last_error()
    assert lib.nf_field_compute_class_area_async(ctypes.byref(g._h), 0, None) == 1
    assert _ca(g, 0)[0].max() > 0
    # a cell thickness: this call takes it, the net class form still refuses
    _set_thickness(g, real, grid, True, 'static')
    assert _ca(g, 0)[0].max() > 0
    with pytest.raises(RuntimeError, match='does not take per-cell thicknesses yet'):
        g.computeClassTransport(0)


# ---- 6. files and the command line -----------------------------------------------------------------------------------------
@pytest.mark.parametrize('carry', [False, True], ids=['one-tracer', 'carried'])
@pytest.mark.parametrize('cell', [False, True], ids=['scalar', 'cell'])
def test_fluxplot_class_area_is_the_field_table(tmp_path, carry, cell):
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
    out = str(tmp_path / 'class_area.csv')
    kw = dict(tFile=paths['T'], uFile=paths['U'], vFile=paths['V'], tracer='sigma0', tracerFile=paths['S'],
              classArea=','.join(repr(float(e)) for e in edges))
    if carry:
        kw.update(carry='thetao', carryRef=1.5)
    if cell:
        kw.update(cellThickness=True)
    totals = _quiet(fluxplot.main, lonLatPoints=lines, output=out, **kw)
    mem = _field(blon, blat, DB, u, v, fluxplot.readTargets(lines)[0], fill_value=FILL, missing_value=MISSING, readback=False)
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
    assert text[0].startswith('# section area by sigma0 class') and ('mean thetao' if carry else 'mean sigma0') in text[0]
    assert text[1] == 'time,transect,lower,upper,area,mean,depth'
    body = [ln.split(',') for ln in text[2:]]
    nrows = edges.size + 2
    assert totals.shape == (NT, 3, nrows, 2) and len(body) == NT * 2 * nrows
    bounds = [(-numpy.inf, edges[0])] + list(zip(edges[:-1], edges[1:])) + [(edges[-1], numpy.inf)]
    for t in range(NT):
        parts = mem.computeClassArea(t)[0]
        mean = Field.classMeanTracer(parts, 1.5 if carry else 0.0)
        depth = Field.classInterfaceDepth(parts[0], mem.computeAreaProfile(t)[0][0], mem.bounds_depth)
        assert parts[0].max() > 0 and numpy.isfinite(depth).all() and (not carry or parts[0, nrows - 1].max() > 0)
        assert _same_bits(totals[t, 0], parts[0]) and numpy.array_equal(totals[t, 1], mean, equal_nan=True)
        assert numpy.array_equal(totals[t, 2, :edges.size], depth) and numpy.isnan(totals[t, 2, edges.size:]).all()
        for p in range(2):
            for k in range(nrows):
                ln = body[(t * 2 + p) * nrows + k]
                assert ln[1] == f'line{p}'
                if k < nrows - 1:
                    assert (float(ln[2]), float(ln[3])) == bounds[k]
                else:
                    assert numpy.isnan(float(ln[2])) and numpy.isnan(float(ln[3]))
                row = [parts[0, k, p], mean[k, p], depth[k, p] if k < edges.size else numpy.nan]
                assert numpy.allclose([float(x) for x in ln[4:]], row, rtol=1e-14, atol=1e-300, equal_nan=True)
