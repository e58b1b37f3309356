"""The six resolved products -- volume and tracer profile, volume / one-tracer / two-tracer class rows, tracer row -- with a
real column: 363 x 291 (odd, no multiple of 16 or 64) x 75 levels x 2 steps, periodic with wrapX, 69 transects (the seeded
seam-crossing batch, a two-vertex diagonal, a line inside one cell), against tests/resolved_reference.py.

What the toy shapes of the older tests never ran: 10 / 19 / 10 level chunks per profile with a ragged last one (the
`prof + zc * row_length` offset, the scratch reused chunk after chunk); class rows beyond the first window of 32 (`r0 > 0`),
the launches above 64 KiB of LDS in all three forms, 2 / 16 / 31 / 255 / 256 / 1025 class edges (4 to 1027 rows: one window,
32 + 1 rows, 9 and 33 windows; two powers of two whose top class holds flux; the maximum); segments of more than 256 records
(several workgroups) beside segments inside one wave.  Bar: 1e-12 x sum |terms| per value, on the reference's `mag`.
Worst |err| / mag measured on an MI355X (each test prints its own, -s): 4.5e-16 at float64 (HBM and host inputs alike),
5.5e-16 at float32; sum of four ranks' class rows against the reference 4.2e-16; the sums over levels and over classes meet
32 eps x mag against the tracer row."""
import numpy
import pytest

import bench
import test_gpu_tracer_resolved as base
from gpu_helpers import _field, _rows
from resolved_reference import ResolvedReference, array_values
from test_gpu_tracer_resolved import (CFILL, CMISSING, FILL, MISSING, TFILL, TMISSING, REF, EPS, _carried, _class_field, _tprof,
                                      _tracer_row, _trows, _window)

pytestmark = pytest.mark.gpu

NX, NY, NZ, NT = 363, 291, 75, 2
BAR = 1e-12
THREADS = 16
# the class field is 10 + 5 N(0, 1) with +-inf, 8 and 12 planted: every class of every set holds faces (checked on 1e8 random
# faces: at least 870 in the emptiest of the 1027 rows)
EDGE_COUNTS = (2, 16, 31, 255, 256, 1025)
EDGE_SETS = [numpy.array([8., 12.])] + [numpy.linspace(0., 20., n) for n in EDGE_COUNTS[1:]]
K255 = EDGE_COUNTS.index(255)


def _lines():
    polys = bench.make_transects(NX, NY, -180., 180., -90., 90., 64, seed=20260402, seam=True)
    dx, dy = 360. / NX, 180. / NY
    polys.append([(-179.3, -79.6), (178.9, 80.2)])                                              # across the whole grid
    polys.append([(-180. + 100.2 * dx, -90. + 150.3 * dy), (-180. + 100.7 * dx, -90. + 150.6 * dy)])   # inside one cell
    return [numpy.array([(x, y, 0.) for x, y in p]) for p in polys]


_DATA = {}


def _data(real):
    """bounds, host uo / vo (random, _FillValue, a second missing value, NaN), carried tracer, class field, and the class
    field without +-inf (it is carried too in the one-tracer form)"""
    if real not in _DATA:
        from nemoflux_amd.datagen import DataGen
        dg = DataGen(real=real)
        dg.setSizes(NX, NY, NZ, NT)
        dg.setBoundingBox(-180., 180., -90., 90., 0., 1.)
        dg.build()
        rng = numpy.random.default_rng(363291)
        dt = numpy.dtype(real).type
        shape = (NT, NZ, NY, NX)
        uv = []
        for _ in range(2):
            a = rng.standard_normal(shape).astype(dt)
            for m, share in ((FILL, 9), (MISSING, 11), (numpy.nan, 13)):
                a.reshape(-1)[rng.choice(a.size, a.size // share, replace=False)] = dt(m)
            uv.append(a)
        tau, sig = _carried(shape, real, 75), _class_field(shape, real, 76)
        sig_finite = numpy.where(numpy.isinf(sig), dt(11.), sig)
        _DATA[real] = dict(blon=dg.bounds_lon.cpu().numpy(), blat=dg.bounds_lat.cpu().numpy(), db=numpy.asarray(dg.deptht_bounds),
                           uo=uv[0], vo=uv[1], tau=tau, sig=sig, sig_finite=sig_finite, fields={}, on={})
    return _DATA[real]


def _sverdrup(real):
    return real == 'float32'


def _on(d, name, resident):
    """the array `name` as the Field takes it: the host array, or one device copy of it"""
    if not resident:
        return d[name]
    if name not in d['on']:
        import torch
        d['on'][name] = torch.from_numpy(d[name]).cuda()
    return d['on'][name]


def _make(real, resident, **kw):
    d = _data(real)
    return _field(d['blon'], d['blat'], d['db'], _on(d, 'uo', resident), _on(d, 'vo', resident), _lines(),
                  sverdrup=_sverdrup(real), readback=False, fill_value=FILL, missing_value=MISSING, **kw)


def _two(f, real, resident):
    """carried tracer and a class field of its own: the volume rows by that class field, and the two-tracer form"""
    d = _data(real)
    f.setTracer(_on(d, 'tau', resident), fill_value=CFILL, missing_value=CMISSING, reference=REF, wrapX=True)
    f.setClassTracer(_on(d, 'sig', resident), fill_value=TFILL, missing_value=TMISSING)


def _one(f, real, resident):
    """the (finite) class field carried by itself: the one-tracer form"""
    d = _data(real)
    f.setClassTracer(None)
    f.setTracer(_on(d, 'sig_finite', resident), fill_value=TFILL, missing_value=TMISSING, reference=REF, wrapX=True)


def _reference(real, f):
    """the reference's results {('two' | 'one', t): step dict} for the weights of f, computed once per dtype"""
    d = _data(real)
    if 'want' not in d:
        ce, w, sg = f.getWeights()
        d['weights'] = (ce, w, sg)
        kw = dict(uv_markers=(FILL, MISSING), reference=REF, wrap=True, sverdrup=_sverdrup(real))
        two = ResolvedReference(ce, w, sg, f.arcLengths, f.thickness, f._tr_off, NX, NY, tracer_markers=(CFILL, CMISSING),
                                class_markers=(TFILL, TMISSING), **kw)
        one = ResolvedReference(ce, w, sg, f.arcLengths, f.thickness, f._tr_off, NX, NY, tracer_markers=(TFILL, TMISSING),
                                class_markers=(TFILL, TMISSING), **kw)
        arrays = {'two': {'uo': d['uo'], 'vo': d['vo'], 'tracer': d['tau'], 'class': d['sig']},
                  'one': {'uo': d['uo'], 'vo': d['vo'], 'tracer': d['sig_finite'], 'class': d['sig_finite']}}
        d['want'] = {}
        for t in range(NT):
            d['want']['two', t] = two.step(array_values(arrays['two'], t), EDGE_SETS, threads=THREADS)
            d['want']['one', t] = one.step(array_values(arrays['one'], t), EDGE_SETS, threads=THREADS, volume_classes=False)
        # the shapes this file is about, on the inputs alone
        per_seg = numpy.bincount(sg, minlength=f._nseg) // 4                 # records (four entries each) per segment
        first = numpy.concatenate([[0], numpy.cumsum(per_seg)])               # K3's record order: segment after segment
        assert per_seg.max() > 256, 'some segment spans more than one workgroup'
        assert ((per_seg > 0) & (first[:-1] // 64 == (first[1:] - 1) // 64)).any(), 'some segment lies inside one wave'
        assert f._nseg > 2000 and per_seg.sum() > 500_000
    assert all(numpy.array_equal(a, b) for a, b in zip(d['weights'], f.getWeights()))
    return d['want']


WORST = {}


def _check(label, got, pair, bar=BAR, no_value_row_is_empty=False):
    """no_value_row_is_empty: the one-tracer form, whose class field is the carried tracer itself -- a face without a class
    value has no carried value either (tf = 0), so by definition the last row holds no term and must be exact zeros"""
    want, mag = pair
    assert got.shape == want.shape, label
    if mag.ndim == 2:
        carries = mag.max(axis=1) > 0
        if no_value_row_is_empty:
            assert not carries[-1] and not got[-1].any(), label
            carries = carries[:-1]
        assert carries.all(), f'{label}: every row must carry flux in some column'
    else:
        assert mag.max() > 0, label
    ratio = float((numpy.abs(got - want) / numpy.maximum(mag, 1e-300)).max())
    WORST[label] = ratio
    print(f'{label}: max |err| / mag = {ratio:.3g}')
    assert numpy.all(numpy.abs(got - want) <= bar * mag), (label, ratio)


@pytest.mark.parametrize('real,resident', [('float64', True), ('float64', False), ('float32', True)],
                         ids=['float64-hbm', 'float64-host', 'float32-hbm'])
def test_six_products_at_75_levels_against_the_reference(real, resident):
    f = _make(real, resident)
    want = _reference(real, f)
    tag = f'{real} {"hbm" if resident else "host"}'
    _two(f, real, resident)
    tracer_row = {}
    for t in range(NT):
        w = want['two', t]
        prof, tprof, trow = _rows(f.computeFluxProfile(t)), _tprof(f, t), _tracer_row(f, t)
        tracer_row[t] = trow
        _check(f'{tag} t={t} volume profile', prof, w['volume_profile'])
        _check(f'{tag} t={t} tracer profile', tprof, w['tracer_profile'])
        _check(f'{tag} t={t} tracer row', trow, w['tracer'])
        pmag = w['tracer_profile'][1]
        assert numpy.all(numpy.abs(tprof.sum(axis=0) - trow) <= 32 * EPS * pmag.sum(axis=0)), t
        for k, edges in enumerate(EDGE_SETS):
            f.setClassEdges(edges)
            vol, tra = _rows(f.computeClassTransport(t)), _trows(f, t)
            assert vol.shape == (edges.size + 2, f._rowlen)
            _check(f'{tag} t={t} {edges.size} edges volume rows', vol, w['volume_classes', k])
            _check(f'{tag} t={t} {edges.size} edges two-tracer rows', tra, w['tracer_classes', k])
            mag = w['tracer_classes', k][1]
            assert numpy.all(numpy.abs(tra.sum(axis=0) - trow) <= 32 * EPS * mag.sum(axis=0)), (t, edges.size)
    _one(f, real, resident)
    for t in range(NT):
        w = want['one', t]
        trow = _tracer_row(f, t)
        _check(f'{tag} t={t} one-tracer: tracer row', trow, w['tracer'])
        _check(f'{tag} t={t} one-tracer: tracer profile', _tprof(f, t), w['tracer_profile'])
        for k, edges in enumerate(EDGE_SETS):
            f.setClassEdges(edges)
            tra = _trows(f, t)
            _check(f'{tag} t={t} {edges.size} edges one-tracer rows', tra, w['tracer_classes', k], no_value_row_is_empty=True)
            mag = w['tracer_classes', k][1]
            assert numpy.all(numpy.abs(tra.sum(axis=0) - trow) <= 32 * EPS * mag.sum(axis=0)), (t, edges.size)
    worst = max(v for k, v in WORST.items() if k.startswith(tag))
    print(f'{tag}: worst |err| / mag of all products = {worst:.3g}')


@pytest.mark.parametrize('real', ['float64', 'float32'])
def test_windows_5_and_32_give_the_same_bits_for_255_edges(real):
    """257 rows: 52 windows of 5 (the last of 2 rows) against 9 windows of 32 (the last of 1), in the three forms"""
    f = _make(real, True)
    f.setClassEdges(EDGE_SETS[K255])
    for form in (_two, _one):
        form(f, real, True)
        for t in range(NT):
            rows32 = (_rows(f.computeClassTransport(t)), _trows(f, t))
            with _window(5):
                rows5 = (_rows(f.computeClassTransport(t)), _trows(f, t))
            for a, b in zip(rows32, rows5):
                # (the one-tracer form's no-value row is empty by definition: no class value, no carried value)
                assert a.shape == (257, f._rowlen) and (numpy.abs(a[:-1]).max(axis=1) > 0).all()
                assert numpy.array_equal(a, b), (form.__name__, t)


def test_sharded_levels_are_the_unsharded_rows():
    """four ranks, cuts at slabs 37, 75 and 112 (levels 37 of step 0 and of step 1: no multiple of 4 or 8): profile row z of the
    rank that owns level z is the unsharded row bit for bit and zero on the others; the ranks' class rows add up to the
    unsharded rows within the bar"""
    from nemoflux_amd.dist import slab_range
    real = 'float64'
    full = _make(real, True)
    want = _reference(real, full)
    _two(full, real, True)
    full.setClassEdges(EDGE_SETS[K255])
    cuts = [slab_range(NT, NZ, r, 4) for r in range(4)]
    assert [c[0] for c in cuts] == [0, 37, 75, 112]
    parts = []
    for sr in cuts:
        p = _make(real, True, slab_range=sr)
        _two(p, real, True)
        p.setClassEdges(EDGE_SETS[K255])
        parts.append(p)
    for t in range(NT):
        prof, tprof = _rows(full.computeFluxProfile(t)), _tprof(full, t)
        vol, tra = _rows(full.computeClassTransport(t)), _trows(full, t)
        vsum, tsum = numpy.zeros_like(vol), numpy.zeros_like(tra)
        owners = numpy.zeros(NZ, int)
        for p, sr in zip(parts, cuts):
            lo, hi = max(sr[0], t * NZ) - t * NZ, min(sr[1], (t + 1) * NZ) - t * NZ
            owned = numpy.zeros(NZ, bool)
            owned[max(lo, 0):max(hi, 0)] = True
            owners += owned
            for mine, whole in ((_rows(p.computeFluxProfile(t)), prof), (_tprof(p, t), tprof)):
                assert numpy.array_equal(mine[owned], whole[owned]), (t, sr)
                assert not mine[~owned].any(), (t, sr)
            vsum += _rows(p.computeClassTransport(t))
            tsum += _trows(p, t)
        assert (owners == 1).all()
        w = want['two', t]
        for label, got, whole, key in (('volume', vsum, vol, 'volume_classes'), ('two-tracer', tsum, tra, 'tracer_classes')):
            mag = w[key, K255][1]
            ratio = float((numpy.abs(got - whole) / numpy.maximum(mag, 1e-300)).max())
            print(f'sharded t={t} {label} rows: max |sum of ranks - unsharded| / mag = {ratio:.3g}')
            assert numpy.all(numpy.abs(got - whole) <= BAR * mag), (t, label, ratio)
            _check(f'sharded t={t} {label} rows, sum of ranks', got, w[key, K255])


def test_the_reference_agrees_with_the_restatement_of_the_small_grid_test():
    """for the inputs of test_against_the_numpy_restatement[float64-37x11-wrap] the sparse reference and that file's dense
    `_restated` agree to 4 eps x sum |terms|, values and sums |terms| alike"""
    real, nx, ny, wrap = 'float64', 37, 11, True
    nz, nt = 5, 2
    blon, blat, db, u, v, tau, sig = base._small_grid(real, nx, ny, nz, nt, seed=nx * 100 + ny + wrap)
    sverdrup = nx % 2 == 1
    f = _field(blon, blat, db, u, v, base._small_lines(nx, ny), sverdrup=sverdrup, readback=False, fill_value=FILL,
               missing_value=MISSING, periodX=0.)
    ref = ResolvedReference(*f.getWeights(), f.arcLengths, f.thickness, f._tr_off, nx, ny, uv_markers=(FILL, MISSING),
                            tracer_markers=(CFILL, CMISSING), class_markers=(TFILL, TMISSING), reference=3.25, wrap=wrap,
                            sverdrup=sverdrup)
    for t in range(nt):
        rows, mag, prof, pmag = base._restated(f, u[t], v[t], tau[t], sig[t], (FILL, MISSING), (CFILL, CMISSING),
                                               (TFILL, TMISSING), 3.25, wrap, sverdrup, base.SMALL_EDGES)
        got = ref.step(array_values({'uo': u, 'vo': v, 'tracer': tau, 'class': sig}, t), [base.SMALL_EDGES])
        for (a, am), (b, bm) in ((got['tracer_classes', 0], (rows, mag)), (got['tracer_profile'], (prof, pmag))):
            assert a.shape == b.shape and bm.max() > 0
            print(f't={t}: max |reference - _restated| / mag = {(numpy.abs(a - b) / numpy.maximum(bm, 1e-300)).max():.3g}')
            assert numpy.all(numpy.abs(a - b) <= 4 * EPS * bm), t
            assert numpy.all(numpy.abs(am - bm) <= 4 * EPS * bm), t
