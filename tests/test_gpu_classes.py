"""Volume transport in tracer classes (Field.setClassEdges / computeClassTransport, nf_field_compute_class_transport*): every
per-level term of the depth profile goes to the row of its face's class.  Anchored bit for bit to the profile rows (tau =
level index), checked for conservation against the volume row, against a float64 numpy restatement on odd grids (markers,
wrap, values on the edges, +-inf), against K1 + K3 on class-masked uo / vo; determinism, sharding, unchanged state,
file-backed inputs and fluxplot --classes."""
import contextlib
import os

import numpy
import pytest

from conftest import GOLDEN, transect_xyz
from gpu_helpers import _field, _on, _quiet, _resident, _rows

pytestmark = pytest.mark.gpu

PSI_ZT = "(1+10*z)*(t+1)*(cos(2*pi*y/360) + sin(2*pi*x/360))"
T_TRI = "(-100,-80),(100,-80),(0,80),(-100,-80)"
T_OPEN = "(-100,-80),(100,-80),(0,80)"
T_SEAM = "(150,-30),(179.5,-20),(179.9,10),(175,40)"     # crosses the periodic seam: east faces of the last column
NX, NY, NZ, NT = 72, 36, 7, 3
FILL, MISSING = 1.e20, -999.
TFILL, TMISSING = -32768., 12345.
R_SV = 6371000.0 / 1.e6
EPS = numpy.finfo(numpy.float64).eps
LEVEL_EDGES = numpy.arange(NZ + 1) - 0.5          # -0.5, 0.5, ..., NZ - 0.5


_CASES = {}


def _case(real, fill=True):
    """host u, v (nt, nz, ny, nx) of the PSI_ZT case; with `fill`, land blocks marked by _FillValue, NaN and a second
    missing value"""
    key = (real, fill)
    if key not in _CASES:
        from nemoflux_amd.datagen import DataGen
        dg = DataGen(real=real)
        dg.setSizes(NX, NY, NZ, NT)
        dg.setBoundingBox(-180., 180., -90., 90., 0., 1.)
        dg.build()
        dg.applyStreamFunction(PSI_ZT)
        dg.computeUVFromPotential()
        u, v = dg.u.cpu().numpy().copy(), dg.v.cpu().numpy().copy()
        v[:, :, -1, :] = 0                     # datagen's pole row is 1e13-sized garbage
        if fill:
            dt = u.dtype.type
            u[:, 3:, 4:9, 10:20] = dt(FILL)
            v[:, 3:, 4:9, 10:20] = numpy.nan
            u[:, :2, 20:24, 30:40] = dt(MISSING)
            v[:, 5:, 20:24, 30:40] = dt(MISSING)
        _CASES[key] = (dg.bounds_lon.cpu().numpy(), dg.bounds_lat.cpu().numpy(), dg.deptht_bounds, u, v)
    return _CASES[key]


def _args(real, resident, fill=True):
    blon, blat, db, u, v = _case(real, fill)
    return (blon, blat, db, _on(u, resident), _on(v, resident),
            [transect_xyz(T_OPEN), transect_xyz(T_TRI), transect_xyz(T_SEAM)])


def _kw(sverdrup, fill=True, **kw):
    kw.update(sverdrup=sverdrup, readback=False)
    if fill:
        kw.update(fill_value=FILL, missing_value=MISSING)
    return kw


def _class_rows(f, t, out=None):
    return _rows(f.computeClassTransport(t, out=out))


def _volume_row(f, t):
    f.computeFlux(t)
    return numpy.array(f._row[:f._rowlen])


def _level_tau(shape, dtype):
    return numpy.broadcast_to(numpy.arange(shape[1], dtype=dtype)[None, :, None, None], shape).copy()


DEFAULT_WINDOW = 32     # nf_tuning_set("class_window") default


@contextlib.contextmanager
def _window(w):
    from nemoflux_amd._lib import lib, check
    check(lib.nf_tuning_set(b'class_window', int(w)))
    try:
        yield
    finally:
        check(lib.nf_tuning_set(b'class_window', DEFAULT_WINDOW))


@pytest.mark.parametrize('resident', [True, False], ids=['hbm', 'host'])
@pytest.mark.parametrize('fill', [True, False], ids=['markers', 'nomarkers'])
@pytest.mark.parametrize('sverdrup', [False, True], ids=['m2', 'sv'])
@pytest.mark.parametrize('real', ['float64', 'float32'])
def test_level_index_classes_are_the_profile_bit_for_bit(real, sverdrup, fill, resident):
    """tau = z, edges -0.5, 0.5, ..., nz - 0.5: class row z + 1 is profile row z bit for bit; rows 0, nz + 1 and nz + 2 are
    exact zeros"""
    f = _field(*_args(real, resident, fill), **_kw(sverdrup, fill))
    u = _case(real, fill)[3]
    f.setTracer(_on(_level_tau(u.shape, u.dtype), resident), reference=7.5)     # the reference is not used for classes
    f.setClassEdges(LEVEL_EDGES)
    for t in (2, 0, 1):
        rows = _class_rows(f, t)
        prof = _rows(f.computeFluxProfile(t))
        assert rows.shape == (NZ + 3, f._rowlen)
        assert numpy.abs(prof).max() > 0
        assert numpy.array_equal(rows[1:NZ + 1], prof), t
        assert not rows[0].any() and not rows[NZ + 1:].any(), t


def test_level_index_holds_for_every_window():
    """the rows do not depend on how many of them one pass over the fields builds"""
    f = _field(*_args('float64', True), **_kw(False))
    u = _case('float64')[3]
    f.setTracer(_on(_level_tau(u.shape, u.dtype), True))
    f.setClassEdges(LEVEL_EDGES)
    prof = _rows(f.computeFluxProfile(1))
    want = _class_rows(f, 1)
    for w in (1, 3, 16):
        with _window(w):
            got = _class_rows(f, 1)
        assert numpy.array_equal(got, want), w
        assert numpy.array_equal(got[1:NZ + 1], prof), w


# ---- the definition, restated in float64 numpy -----------------------------------------------------------------------------
def _restated_class_rows(f, u, v, tau, umark, tmark, wrap, sverdrup, edges):
    """rows (nedges + 2, row_length) of one step and the bound sum |terms| per value: u, v, tau (nz, ny, nx) in their own
    dtype, markers compared in that dtype"""
    dt = tau.dtype.type
    um = [dt(m) for m in umark if m == m]
    tm = [dt(m) for m in tmark if m == m]

    def present(x):
        ok = ~numpy.isnan(x)
        for m in tm:
            ok &= x != m
        return ok

    def fixed(x):
        bad = numpy.isnan(x)
        for m in um:
            bad |= x == m
        return numpy.where(bad, 0.0, x.astype(numpy.float64))

    def face_row(a, b, has_b):
        pa, pb = present(a), has_b & present(b)
        a64, b64 = a.astype(numpy.float64), b.astype(numpy.float64)
        with numpy.errstate(invalid='ignore', over='ignore'):
            x = numpy.where(pa & pb, 0.5 * (a64 + b64), numpy.where(pa, a64, b64))
        row = numpy.searchsorted(edges, numpy.where(numpy.isnan(x), 0.0, x), side='right')   # edges <= x
        return numpy.where((pa | pb) & ~numpy.isnan(x), row, len(edges) + 1)

    nz, ny, nx = tau.shape
    has_e = numpy.ones((nz, ny, nx), bool)
    if not wrap:
        has_e[:, :, -1] = False
    has_n = numpy.ones((nz, ny, nx), bool)
    has_n[:, -1, :] = False
    rowE = face_row(tau, numpy.roll(tau, -1, axis=2), has_e).reshape(nz, -1)   # class row of the east face of every cell
    rowN = face_row(tau, numpy.roll(tau, -1, axis=1), has_n).reshape(nz, -1)   # ... of the north face
    arc = f.arcLengths
    aE, aN = arc[:, 1], arc[:, 2]
    th = f.thickness
    ce, w, sg = f.getWeights()
    c, slot = ce // 4, ce % 4
    j, i = c // nx, c % nx
    cw = numpy.where(i > 0, c - 1, c - 1 + nx)
    cs = numpy.where(j > 0, c - nx, c)
    keep = (slot != 0) | (j > 0)               # row 0's south slots carry nothing
    cell = numpy.select([slot == 0, slot == 1, slot == 2], [cs, c, c], cw)
    nrow = len(edges) + 2
    rows = numpy.zeros((nrow, f._nseg))
    mag = numpy.zeros((nrow, f._nseg))
    for z in range(nz):
        U, V = fixed(u[z]).reshape(-1), fixed(v[z]).reshape(-1)
        d = numpy.where((slot == 1) | (slot == 3), th[z] * U[cell] * aE[cell], -(th[z] * V[cell]) * aN[cell])
        if sverdrup:
            d = d * R_SV
        r = numpy.where((slot == 1) | (slot == 3), rowE[z][cell], rowN[z][cell])
        terms = numpy.where(keep, w * d, 0.0)
        numpy.add.at(rows, (r, sg), terms)
        numpy.add.at(mag, (r, sg), numpy.abs(terms))
    o = f._tr_off
    tot = numpy.stack([rows[:, o[p]:o[p + 1]].sum(axis=1) for p in range(len(o) - 1)], axis=1)
    tmag = numpy.stack([mag[:, o[p]:o[p + 1]].sum(axis=1) for p in range(len(o) - 1)], axis=1)
    return numpy.concatenate([rows, tot], axis=1), numpy.concatenate([mag, tmag], axis=1)


def _small_grid(real, nx, ny, nz, nt, seed):
    """bounds of a regular 1-degree grid on [0, nx] x [0, ny], random u, v with markers, a random tau with markers (faces
    with one and with both sides missing), neighbour pairs that put face values exactly on the edges, and +-inf"""
    from nemoflux_amd.datagen import DataGen
    dg = DataGen(real=real)
    dg.setSizes(nx, ny, nz, nt)
    dg.setBoundingBox(0., float(nx), 0., float(ny), 0., 1.)
    dg.build()
    rng = numpy.random.default_rng(seed)
    dt = numpy.dtype(real).type
    shape = (nt, nz, ny, nx)
    u = rng.standard_normal(shape).astype(dt)
    v = rng.standard_normal(shape).astype(dt)
    u.reshape(-1)[rng.choice(u.size, u.size // 9, replace=False)] = dt(FILL)
    v.reshape(-1)[rng.choice(v.size, v.size // 9, replace=False)] = numpy.nan
    u.reshape(-1)[rng.choice(u.size, u.size // 11, replace=False)] = dt(MISSING)
    tau = (10. + 5. * rng.standard_normal(shape)).astype(dt)
    tau.reshape(-1)[rng.choice(tau.size, tau.size // 5, replace=False)] = rng.choice([8., 12.], tau.size // 5)
    tau.reshape(-1)[rng.choice(tau.size, tau.size // 25, replace=False)] = numpy.inf
    tau.reshape(-1)[rng.choice(tau.size, tau.size // 25, replace=False)] = -numpy.inf
    for m in (TFILL, TMISSING, numpy.nan):
        tau.reshape(-1)[rng.choice(tau.size, tau.size // 7, replace=False)] = dt(m)
    return dg.bounds_lon.cpu().numpy(), dg.bounds_lat.cpu().numpy(), dg.deptht_bounds, u, v, tau


def _small_lines(nx, ny):
    x1, y1 = nx - 0.37, ny - 0.41
    return [transect_xyz(f"(0.3,0.2),({x1},{0.6 * ny}),({0.5 * nx},{y1})"),
            transect_xyz(f"({x1},0.45),({x1 - 0.02},{y1})"),
            transect_xyz(f"(0.61,{y1}),({x1},{y1 - 0.03})")]


SMALL_EDGES = numpy.array([0., 5., 8., 10., 12., 15., 20.])


@pytest.mark.parametrize('wrap', [True, False], ids=['wrap', 'nowrap'])
@pytest.mark.parametrize('grid', [(37, 11), (38, 12), (1, 11), (37, 1), (5, 3)], ids=lambda g: f'{g[0]}x{g[1]}')
@pytest.mark.parametrize('real', ['float64', 'float32'])
def test_against_the_numpy_restatement(real, grid, wrap):
    nx, ny = grid
    nz, nt = 5, 2
    blon, blat, db, u, v, tau = _small_grid(real, nx, ny, nz, nt, seed=nx * 100 + ny + wrap)
    sverdrup = nx % 2 == 1
    f = _field(blon, blat, db, u, v, _small_lines(nx, ny), sverdrup=sverdrup, readback=False, fill_value=FILL,
               missing_value=MISSING, periodX=0.)
    f.setTracer(tau, fill_value=TFILL, missing_value=TMISSING, reference=3.25, wrapX=wrap)
    f.setClassEdges(SMALL_EDGES)
    nrow = SMALL_EDGES.size + 2
    for t in range(nt):
        want, mag = _restated_class_rows(f, u[t], v[t], tau[t], (FILL, MISSING), (TFILL, TMISSING), wrap, sverdrup,
                                         SMALL_EDGES)
        got = _class_rows(f, t)
        assert got.shape == (nrow, f._rowlen)
        assert numpy.all(numpy.abs(got - want) <= 1e-12 * mag), (t, numpy.abs(got - want).max())
        assert mag[-1].max() > 0, 'faces without a class value must carry flux'
        assert mag[SMALL_EDGES.size].max() > 0, 'the top class (+inf) must carry flux'
        # conservation: all rows add up to the volume row
        vol = _volume_row(f, t)
        assert numpy.all(numpy.abs(got.sum(axis=0) - vol) <= 32 * EPS * mag.sum(axis=0)), t


def test_face_values_on_an_edge_go_to_the_upper_class():
    """a tracer made only of the edge values themselves (both sides equal): every face lies exactly on an edge"""
    nx, ny, nz, nt = 9, 7, 3, 1
    blon, blat, db, u, v, _ = _small_grid('float64', nx, ny, nz, nt, seed=5)
    rng = numpy.random.default_rng(5)
    tau = numpy.repeat(rng.choice(SMALL_EDGES, (nt, nz, ny, 1)), nx, axis=3)      # rows of one edge value: E and W faces
    f = _field(blon, blat, db, u, v, _small_lines(nx, ny), readback=False, fill_value=FILL, missing_value=MISSING, periodX=0.)
    f.setTracer(tau)
    f.setClassEdges(SMALL_EDGES)
    got = _class_rows(f, 0)
    want, mag = _restated_class_rows(f, u[0], v[0], tau[0], (FILL, MISSING), (), True, False, SMALL_EDGES)
    assert numpy.all(numpy.abs(got - want) <= 1e-12 * mag)
    assert not mag[0].any(), 'nothing lies below the first edge'
    assert mag[1:SMALL_EDGES.size + 1].any(axis=1).sum() >= 4


def test_class_masked_volume_rows_are_the_class_rows():
    """independent of the profile terms: for every class, K1 + K3 (computeFlux) of uo / vo with the faces of the other
    classes set to zero gives that class row (to rounding)"""
    import torch
    real = 'float64'
    blon, blat, db, u, v = _case(real)
    rng = numpy.random.default_rng(17)
    tau = (10. + 6. * rng.standard_normal(u.shape)).astype(u.dtype)
    tau.reshape(-1)[rng.choice(tau.size, tau.size // 6, replace=False)] = numpy.nan
    edges = numpy.array([4., 7., 9., 10., 11., 13., 16.])
    ut, vt = _on(u, True), _on(v, True)
    f = _field(blon, blat, db, ut, vt, [transect_xyz(T_OPEN), transect_xyz(T_TRI), transect_xyz(T_SEAM)], **_kw(False))
    f.setTracer(_on(tau, True), wrapX=True)
    f.setClassEdges(edges)

    def face_rows(a, b, has_b):
        pa, pb = ~numpy.isnan(a), has_b & ~numpy.isnan(b)
        x = numpy.where(pa & pb, 0.5 * (a + b), numpy.where(pa, a, b))
        return numpy.where(pa | pb, numpy.searchsorted(edges, numpy.where(pa | pb, x, 0.), side='right'), edges.size + 1)

    has_n = numpy.ones(tau.shape, bool)
    has_n[:, :, -1, :] = False
    rowE = face_rows(tau, numpy.roll(tau, -1, axis=3), numpy.ones(tau.shape, bool))
    rowN = face_rows(tau, numpy.roll(tau, -1, axis=2), has_n)
    for t in (0, 2):
        got = _class_rows(f, t)
        _, mag = _restated_class_rows(f, u[t], v[t], tau[t], (FILL, MISSING), (), True, False, edges)
        for k in range(edges.size + 2):
            ut.copy_(torch.from_numpy(numpy.where(rowE == k, u, 0.)))
            vt.copy_(torch.from_numpy(numpy.where(rowN == k, v, 0.)))
            want = _volume_row(f, t)
            assert numpy.all(numpy.abs(got[k] - want) <= 1e-12 * mag[k]), (t, k)
        ut.copy_(torch.from_numpy(u))
        vt.copy_(torch.from_numpy(v))
        assert numpy.abs(got[:edges.size + 1]).max() > 0


@pytest.mark.parametrize('real', ['float64', 'float32'])
def test_rows_are_reproducible_and_the_same_for_host_and_hbm_inputs(real):
    u = _case(real)[3]
    rng = numpy.random.default_rng(23)
    tau = (10. + 5. * rng.standard_normal(u.shape)).astype(u.dtype)
    edges = numpy.linspace(-5., 25., 64)
    got = []
    for resident in (True, False):
        f = _field(*_args(real, resident), **_kw(True))
        f.setTracer(_on(tau, resident))
        f.setClassEdges(edges)
        a = _class_rows(f, 1)
        assert numpy.array_equal(_class_rows(f, 1), a)
        got.append(a)
    for w in (1, 7, 16):          # 66 rows: windows of 32 (more than 64 KiB of LDS), 16, 7 and 1 rows
        with _window(w):
            assert numpy.array_equal(_class_rows(f, 1), a), w
    assert numpy.array_equal(got[0], got[1])
    assert (numpy.abs(got[0][1:-2]).max(axis=1) > 0).sum() > 20


def test_out_tensors_are_checked_by_all_four_calls():
    """computeAll, computeFluxProfile, computeTracerAll and computeClassTransport write (rows, row_length) doubles through
    the pointer of `out`: each refuses a float32 and a mis-shaped tensor and accepts the right one"""
    import torch
    u = _case('float64')[3]
    f = _field(*_args('float64', True), **_kw(False))
    f.setTracer(_on(_level_tau(u.shape, u.dtype), True))
    f.setClassEdges(LEVEL_EDGES)
    calls = [(NT, lambda out: f.computeAll(out=out)),
             (NZ, lambda out: f.computeFluxProfile(1, out=out)),
             (NT, lambda out: f.computeTracerAll(out=out)),
             (LEVEL_EDGES.size + 2, lambda out: f.computeClassTransport(1, out=out))]
    for nrows, call in calls:
        want = _rows(call(None))
        assert want.shape == (nrows, f._rowlen)
        for shape, dtype in (((nrows, f._rowlen), torch.float32), ((nrows + 1, f._rowlen), torch.float64),
                             ((nrows, f._rowlen + 1), torch.float64), ((nrows * f._rowlen,), torch.float64)):
            with pytest.raises(RuntimeError, match='out must be'):
                call(torch.zeros(shape, dtype=dtype, device='cuda'))
        with pytest.raises(RuntimeError, match='out must be'):
            call(torch.zeros((nrows, f._rowlen), dtype=torch.float64))                      # not on the GPU
        with pytest.raises(RuntimeError, match='out must be'):
            call(torch.zeros((f._rowlen, nrows), dtype=torch.float64, device='cuda').t())   # not contiguous
        out = torch.full((nrows, f._rowlen), numpy.nan, dtype=torch.float64, device='cuda')
        assert numpy.array_equal(_rows(call(out)), want)
        assert numpy.array_equal(out.cpu().numpy(), want)


@pytest.mark.parametrize('compact', [False, True])
@pytest.mark.parametrize('resident', [True, False], ids=['hbm', 'host'])
def test_class_calls_leave_everything_else_alone(compact, resident):
    """class calls between computeFlux, computeAll, tracer rows and read-backs: rows, planes, |.| arrays, the running max and
    the tracer rows equal those of a field that never saw a class call, bit for bit"""
    args = _args('float64', resident)
    a = _field(*args, compact=compact, **_kw(False))
    b = _field(*args, compact=compact, **_kw(False))
    rng = numpy.random.default_rng(7)
    tau = _on((4. + rng.random(_case('float64')[3].shape)), resident)
    for f in (a, b):
        f.setTracer(tau, reference=4.)
    a.setClassEdges(numpy.linspace(4., 5., 9))
    p0 = _class_rows(a, 1)
    for step in ('flux1', 'all', 'tracer0', 'flux0', 'read', 'all', 'flux2', 'read', 'tracer2'):
        _class_rows(a, 2)
        if step == 'all':
            assert all(numpy.array_equal(x, y) for x, y in zip(a.computeAll(), b.computeAll()))
        elif step == 'read':
            for x, y in zip(_resident(a), _resident(b)):
                assert numpy.array_equal(x, y)
        elif step.startswith('tracer'):
            t = int(step[-1])
            assert numpy.array_equal(_rows(a.computeTracerFlux(t)), _rows(b.computeTracerFlux(t)))
        else:
            t = int(step[-1])
            assert a.computeFlux(t) == b.computeFlux(t)
            _class_rows(a, 0)
            assert numpy.array_equal(numpy.array(a._row[:a._rowlen]), numpy.array(b._row[:b._rowlen]))
            assert a.getSegmentFluxes()[0].tolist() == b.getSegmentFluxes()[0].tolist()
    for x, y in zip(_resident(a), _resident(b)):
        assert numpy.array_equal(x, y)
    assert numpy.array_equal(_class_rows(a, 1), p0)


@pytest.mark.parametrize('world', [2, 3])
def test_sharded_class_rows_add_up(world):
    """slab ranges that cut inside steps: steps a rank does not touch are exact zeros (through `out` too), the ranks' rows
    sum to the single-rank rows; with the level-index tracer, bit for bit"""
    import torch
    from nemoflux_amd.dist import slab_range
    args = _args('float64', True)
    u = _case('float64')[3]
    rng = numpy.random.default_rng(11)
    taus = {'random': _on(10. + 5. * rng.standard_normal(u.shape), True), 'level': _on(_level_tau(u.shape, u.dtype), True)}
    edges = {'random': numpy.linspace(0., 20., 17), 'level': LEVEL_EDGES}
    for name, tau in taus.items():
        full = _field(*args, **_kw(False))
        full.setTracer(tau)
        full.setClassEdges(edges[name])
        want = numpy.array([_class_rows(full, t) for t in range(NT)])
        assert numpy.abs(want).max() > 0
        acc = numpy.zeros_like(want)
        for r in range(world):
            sr = slab_range(NT, NZ, r, world)
            part = _field(*args, slab_range=sr, **_kw(False))
            part.setTracer(tau)
            part.setClassEdges(edges[name])
            for t in range(NT):
                out = torch.full((edges[name].size + 2, part._rowlen), numpy.nan, dtype=torch.float64, device='cuda')
                rows = _class_rows(part, t, out=out)
                assert numpy.array_equal(rows, out.cpu().numpy())
                assert numpy.array_equal(rows, _class_rows(part, t))
                lo, hi = max(sr[0], t * NZ), min(sr[1], (t + 1) * NZ)
                if hi <= lo:
                    assert numpy.all(rows == 0), (name, r, t)
                acc[t] += rows
        if name == 'level':
            assert numpy.array_equal(acc, want)
        else:
            assert numpy.allclose(acc, want, rtol=1e-13, atol=1e-13 * numpy.abs(want).max())


def _h5_files():
    h5 = os.path.join(GOLDEN, 'h5')
    return dict(tFile=os.path.join(h5, 'nemo_T.h5'), uFile=os.path.join(h5, 'nemo_U.h5'), vFile=os.path.join(h5, 'nemo_V.h5'))


H5_LINES = "[(-100,-80),(100,-80),(0,80)],[(-180,-70),(-160,-10),(-35,40),(20,-50),(60,50),(180,40)]"
H5_EDGES = [-0.3, -0.1, 0., 0.05, 0.2]


def test_file_backed_fields_and_tracer_equal_from_arrays():
    """file-backed uo / vo and a file-backed tracer (nemo_U.h5's uo: chunked, deflated float32 with a _FillValue) give the
    rows of fromArrays with the decoded arrays, bit for bit, in any step order"""
    from nemoflux_amd import hdf5min
    from nemoflux_amd.field import Field
    from nemoflux_amd.fluxplot import readTargets
    files = _h5_files()
    tr = readTargets(H5_LINES)[0]
    ff = _quiet(Field, files['tFile'], files['uFile'], files['vFile'], tr)
    ff.setTracer((files['uFile'], 'uo'))
    ff.setClassEdges(H5_EDGES)
    with hdf5min.File(files['tFile']) as f:
        blon, blat = f.datasets['bounds_lon'].read(), f.datasets['bounds_lat'].read()
        db = f.datasets['deptht_bounds'].read()
    with hdf5min.File(files['uFile']) as f:
        u = numpy.array(f.datasets['uo'].read())
        fill = float(f.datasets['uo'].fill_value)
    with hdf5min.File(files['vFile']) as f:
        v = numpy.array(f.datasets['vo'].read())
    fa = _field(blon, blat, db, u, v, tr, fill_value=fill)
    fa.setTracer(u.copy(), fill_value=fill)
    fa.setClassEdges(H5_EDGES)
    for t in (2, 0, 1, 1):
        got = _class_rows(ff, t)
        assert numpy.array_equal(got, _class_rows(fa, t)), t
        assert (numpy.abs(got).max(axis=1) > 0).sum() >= 4
        assert numpy.allclose(got.sum(axis=0), _volume_row(fa, t), rtol=1e-12, atol=1e-12 * numpy.abs(got).sum())


def test_fluxplot_classes_is_the_field_table(tmp_path):
    from nemoflux_amd import fluxplot
    from nemoflux_amd.field import Field
    files = _h5_files()
    out = str(tmp_path / 'classes.csv')
    _quiet(fluxplot.main, lonLatPoints=H5_LINES, output=out, sverdrup=True, tracer='uo', tracerFile=files['uFile'],
           classes=','.join(str(e) for e in H5_EDGES), **files)
    with open(out) as fh:
        text = fh.read().splitlines()
    assert text[0] == '# water flow by uo class [Sv]'
    assert text[1] == 'time,lower,upper,line0,line1'
    body = [ln.split(',') for ln in text[2:]]
    nrow = len(H5_EDGES) + 2
    ff = _quiet(Field, files['tFile'], files['uFile'], files['vFile'], fluxplot.readTargets(H5_LINES)[0], True)
    ff.setTracer((files['uFile'], 'uo'))
    ff.setClassEdges(H5_EDGES)
    assert len(body) == ff.nt * nrow
    bounds = [(-numpy.inf, H5_EDGES[0])] + list(zip(H5_EDGES[:-1], H5_EDGES[1:])) + [(H5_EDGES[-1], numpy.inf)]
    for t in range(ff.nt):
        want = ff.computeClassTransport(t)[0]
        for k in range(nrow):
            ln = body[t * nrow + k]
            lo, hi = float(ln[1]), float(ln[2])
            if k < nrow - 1:
                assert (lo, hi) == bounds[k]
            else:
                assert numpy.isnan(lo) and numpy.isnan(hi)
            assert numpy.allclose([float(x) for x in ln[3:]], want[k], rtol=1e-14, atol=1e-300)
    assert numpy.abs(want).max() > 0
