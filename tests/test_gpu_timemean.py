"""Time means on the GPU: nf_time_mean against the numpy restatement of tests/timemean_reference.py bit for bit (both
dtypes, both rules, vector and one-value-per-lane paths, strides, an odd base pointer, series split over calls, offsets beyond
2^31 elements); Field.timeMean from HBM, host, .npz and step-by-step file inputs against a Field built from the restatement's
mean arrays (bit for bit) and against tests/resolved_reference.py on those arrays (1e-12 x sum |terms|); anchors that need no
reference (the flux of the mean state is the mean of the fluxes; the eddy part vanishes when one factor is constant in time);
Field.meanEddyTracerTransport and fluxplot --eddy; refusals; the source Field is left as it was.

Grids 72 x 36 x 7 x 3 and 73 x 37 x 7 x 3 (odd: every other step of an array is not 16-byte aligned).

Measured on an MI355X: worst |err| / sum |terms| against the resolved reference 2.7e-16 (bar 1e-12); the anchors' worst error
1.7e-4 of their bar; 48 tests in 5 s."""
import ctypes

import numpy
import pytest

from conftest import transect_xyz, write_classic_triple
from gpu_helpers import _field, _on, _quiet, _rows
from resolved_reference import ResolvedReference, array_values
import timemean_reference as tmr

pytestmark = pytest.mark.gpu

PSI_ZT = "(1+10*z)*(t+1)*(cos(2*pi*y/360) + sin(2*pi*x/360))"
LINES = ["(-100,-80),(100,-80),(0,80)", "(-100,-80),(100,-80),(0,80),(-100,-80)", "(150,-30),(179.5,-20),(179.9,10),(175,40)"]
NZ, NT = 7, 3
GRIDS = [(72, 36), (73, 37)]
FILL, MISSING = 1.e20, -999.             # uo / vo
TFILL, TMISSING = -32768., 12345.        # tracers
REF = 4.25
EDGES = [4.2, 4.4, 4.6, 4.8]
BAR = 1e-12
TH = numpy.array([0.125, 0.25, 0.5, 0.375, 0.75, 1.0, 0.625])
DB = numpy.stack([numpy.concatenate([[0.], numpy.cumsum(TH)[:-1]]), numpy.cumsum(TH)], axis=1)
NF_F64, NF_F32 = 0, 1


def _row(f):
    return numpy.array(f._row[:f._rowlen])


# ---- 1 - 3. the raw ABI ----------------------------------------------------------------------------------------------------
def _series(real, nsteps, stride, n, offset, seed):
    """a buffer that holds nsteps windows of n values, step t at offset + t * stride: random values with NaN, both markers and
    +inf / -inf (each at all steps of its value: no +inf + -inf, whose NaN has no defined sign), a value missing at every step"""
    rng = numpy.random.default_rng(seed)
    dt = numpy.dtype(real).type
    buf = numpy.full(offset + (nsteps - 1) * stride + n + 4, 7.25, real)       # what lies between the windows is never read
    win = rng.standard_normal((nsteps, n)).astype(real)
    flat = win.reshape(-1)
    for m in (numpy.nan, TFILL, TMISSING, -0.0):
        flat[rng.choice(flat.size, (flat.size + 7) // 8, replace=False)] = dt(m)
    cols = rng.choice(n, min(n, 6), replace=False)
    if n >= 3:
        win[:, cols[0]] = numpy.inf
        win[:, cols[1]] = -numpy.inf
        win[:, cols[2]] = [(dt(TFILL), numpy.nan, dt(TMISSING))[t % 3] for t in range(nsteps)]      # missing at every step
    for t in range(nsteps):
        buf[offset + t * stride:offset + t * stride + n] = win[t]
    return buf, win


def _call(dev, offset, nsteps, stride, n, code, first, last, rule, total, fill_out, acc, cnt, itemsize):
    """nf_time_mean on the windows of the device buffer `dev`; acc / cnt: (n + 4,) tensors with two guard values on each side"""
    from nemoflux_amd._lib import lib, check
    check(lib.nf_time_mean(acc.data_ptr() + 16, None if cnt is None else cnt.data_ptr() + 16, dev.data_ptr() + offset * itemsize,
                           nsteps, stride, n, code, TFILL, TMISSING, first, last, rule, total, fill_out, None))
    check(lib.nf_synchronize())


def _guards():
    import torch
    return (lambda n: torch.full((n + 4,), -7.0, dtype=torch.float64, device='cuda'),
            lambda n: torch.full((n + 8,), 77, dtype=torch.int32, device='cuda'))


def _acc_of(acc, n):
    a = acc.cpu().numpy()
    assert (a[:2] == -7.0).all() and (a[n + 2:] == -7.0).all(), 'acc was written outside its n values'
    return a[2:n + 2]


def _cnt_of(cnt, n):
    c = cnt.cpu().numpy()
    assert (c[:4] == 77).all() and (c[n + 4:] == 77).all(), 'cnt was written outside its n values'
    return c[4:n + 4].view(numpy.uint32)


@pytest.mark.parametrize('rule', [tmr.OVER_STEPS, tmr.OVER_PRESENT], ids=['steps', 'present'])
@pytest.mark.parametrize('real', ['float64', 'float32'])
def test_raw_abi_is_the_restatement_bit_for_bit(real, rule):
    """one call that finishes (the mean) and one that carries (s and c), n below, at and above a block and odd, 1 .. 13 steps
    (fewer, as many and more than a lane has in flight), contiguous and padded steps, an aligned and an odd base pointer"""
    import torch
    code, itemsize = (NF_F64, 8) if real == 'float64' else (NF_F32, 4)
    fill_out = float(numpy.dtype(real).type(TFILL))
    new_acc, new_cnt = _guards()
    seed = 0
    for n in (1, 3, 255, 256, 257, 18907):
        for nsteps in (1, 2, 5, 13):
            for stride in (n, n + 3):
                for offset in (0, 1):
                    seed += 1
                    buf, win = _series(real, nsteps, stride, n, offset, seed)
                    dev = torch.from_numpy(buf).cuda()
                    label = (n, nsteps, stride, offset)
                    total = nsteps + 2          # not nsteps: the divisor is the argument
                    acc, cnt = new_acc(n), new_cnt(n)
                    _call(dev, offset, nsteps, stride, n, code, 1, 1, rule, total, fill_out, acc, None, itemsize)
                    want = tmr.time_mean(win, (TFILL, TMISSING), rule, total, fill_out)
                    assert tmr.same_bits(_acc_of(acc, n), want), label
                    _call(dev, offset, nsteps, stride, n, code, 1, 0, rule, total, fill_out, acc, cnt, itemsize)
                    s, c = tmr.accumulate(win, (TFILL, TMISSING))
                    assert tmr.same_bits(_acc_of(acc, n), s), label
                    assert numpy.array_equal(_cnt_of(cnt, n), c.reshape(-1)), label
                    if n >= 3:
                        assert (c == 0).any() and numpy.isinf(want).sum() >= 2 and (want[c == 0] == fill_out).all()


@pytest.mark.parametrize('rule', [tmr.OVER_STEPS, tmr.OVER_PRESENT], ids=['steps', 'present'])
@pytest.mark.parametrize('real', ['float64', 'float32'])
def test_series_split_over_calls_is_one_call_bit_for_bit(real, rule):
    """13 steps as calls of 5 + 1 + 7 (first on the first call only, last on the last only); each call takes the 16-byte path
    or one value per lane as its own steps are aligned: the same bits"""
    import torch
    code, itemsize = (NF_F64, 8) if real == 'float64' else (NF_F32, 4)
    fill_out = numpy.nan
    new_acc, new_cnt = _guards()
    for n, stride in ((18907, 18907), (18907, 18908), (256, 256), (257, 260), (3, 3)):
        buf, win = _series(real, 13, stride, n, 0, 100 + n + stride)
        dev = torch.from_numpy(buf).cuda()
        one, acc, cnt = new_acc(n), new_acc(n), new_cnt(n)
        _call(dev, 0, 13, stride, n, code, 1, 1, rule, 13, fill_out, one, None, itemsize)
        t = 0
        for k in (5, 1, 7):
            _call(dev, t * stride, k, stride, n, code, 1 if t == 0 else 0, 1 if t + k == 13 else 0, rule, 13, fill_out, acc, cnt,
                  itemsize)
            t += k
        want = tmr.time_mean(win, (TFILL, TMISSING), rule, 13, fill_out)
        assert tmr.same_bits(_acc_of(one, n), want), (n, stride)
        assert tmr.same_bits(_acc_of(acc, n), want), (n, stride)
        assert numpy.isnan(want).any() and (n == 3 or numpy.isfinite(want).any())


def test_offsets_beyond_2_to_the_31_elements():
    """two steps 2^31 + 5 (one value per lane) and 2^31 + 8 (16-byte path) float32 elements apart in an uninitialised
    allocation of which only the windows are written"""
    import torch
    n = 1000
    big = torch.empty(2 ** 31 + 8 + n, dtype=torch.float32, device='cuda')
    new_acc, _ = _guards()
    for stride in (2 ** 31 + 5, 2 ** 31 + 8):
        _, win = _series('float32', 2, n, n, 0, 7)
        win[1] += numpy.float32(100.)          # a result that read step 0 twice, or step 1 at a wrapped offset, is far off
        big[:n] = torch.from_numpy(win[0]).cuda()
        big[stride:stride + n] = torch.from_numpy(win[1]).cuda()
        for rule in (tmr.OVER_STEPS, tmr.OVER_PRESENT):
            acc = new_acc(n)
            _call(big, 0, 2, stride, n, NF_F32, 1, 1, rule, 2, numpy.nan, acc, None, 4)
            assert tmr.same_bits(_acc_of(acc, n), tmr.time_mean(win, (TFILL, TMISSING), rule, 2, numpy.nan)), (stride, rule)
    del big
    torch.cuda.empty_cache()


# ---- 4. Field.timeMean -----------------------------------------------------------------------------------------------------
_CASES = {}


def _case(real, grid):
    """bounds, host u, v (nt, nz, ny, nx) with land blocks and markers of all three kinds that vary in time, a carried tracer
    (NaN and both markers, some varying in time) and a class field with +-inf"""
    key = (real, grid)
    if key not in _CASES:
        from nemoflux_amd.datagen import DataGen
        nx, ny = grid
        dg = DataGen(real=real)
        dg.setSizes(nx, ny, NZ, NT)
        dg.setBoundingBox(-180., 180., -90., 90., 0., 1.)
        dg.build()
        dg.applyStreamFunction(PSI_ZT)
        dg.computeUVFromPotential()
        u, v = dg.u.cpu().numpy().copy(), dg.v.cpu().numpy().copy()
        v[:, :, -1, :] = 0                     # the generator's pole row is 1e13-sized garbage
        dt = u.dtype.type
        rng = numpy.random.default_rng(5)
        u[:, 3:, 4:9, 10:20] = dt(FILL)        # land: missing at every step
        v[:, 3:, 4:9, 10:20] = numpy.nan
        for a in (u, v):                       # and markers that come and go with time
            flat = a.reshape(-1)
            for m in (FILL, MISSING, numpy.nan):
                flat[rng.choice(flat.size, flat.size // 25, replace=False)] = dt(m)
        tau = (4. + rng.random((NT, NZ, ny, nx))).astype(real)
        tau[:, 1::3, 3:-2:3, 2:-2:4] = numpy.nan
        tau[:, :, 10:14, 50:60] = dt(TFILL)
        tau[:, 2:, 25:28, 5:12] = dt(TMISSING)
        flat = tau.reshape(-1)
        flat[rng.choice(flat.size, flat.size // 20, replace=False)] = numpy.nan
        sig = (4. + rng.random((NT, NZ, ny, nx))).astype(real)
        sig[:, ::2, 30, 40:43] = numpy.inf
        sig[:, 1, 6, 60:62] = (numpy.inf, -numpy.inf)       # a face whose mean is NaN
        sig[:, :, 12:15, 30:50] = dt(TMISSING)
        flat = sig.reshape(-1)
        flat[rng.choice(flat.size, flat.size // 20, replace=False)] = dt(TFILL)
        _CASES[key] = (dg.bounds_lon.cpu().numpy(), dg.bounds_lat.cpu().numpy(), u, v, tau, sig)
    return _CASES[key]


def _lines():
    return [transect_xyz(s) for s in LINES]


def _source(real, grid, resident, u=None, v=None, tau=None, sig=None, **kw):
    blon, blat, u0, v0, tau0, sig0 = _case(real, grid)
    kw.setdefault('readback', False)
    f = _field(blon, blat, DB, _on(u0 if u is None else u, resident), _on(v0 if v is None else v, resident), _lines(),
               fill_value=FILL, missing_value=MISSING, **kw)
    f.setTracer(_on(tau0 if tau is None else tau, resident), fill_value=TFILL, missing_value=TMISSING, reference=REF)
    if sig is not False:
        f.setClassTracer(_on(sig0 if sig is None else sig, resident), fill_value=TFILL, missing_value=TMISSING)
        f.setClassEdges(EDGES)
    return f


def _products(f):
    """the rows of the four products of step 0 as [segments | transects]"""
    f.computeFlux(0)
    return {'volume': _row(f), 'volume_profile': _rows(f.computeFluxProfile(0)), 'tracer': _rows(f.computeTracerFlux(0)),
            ('volume_classes', 0): _rows(f.computeClassTransport(0))}


def _mean_arrays(real, grid, t0, t1, u=None, v=None, tau=None):
    _, _, u0, v0, tau0, sig0 = _case(real, grid)
    u, v, tau = (u0 if u is None else u), (v0 if v is None else v), (tau0 if tau is None else tau)
    (um, vm, fill), ((taum, tfill), (sigm, sfill)) = tmr.field_mean_arrays(
        u[t0:t1], v[t0:t1], (FILL, MISSING), [(tau[t0:t1], (TFILL, TMISSING)), (sig0[t0:t1], (TFILL, TMISSING))])
    return dict(uo=um, vo=vm, tracer=taum), {'class': sigm}, (fill, tfill, sfill)


def _resolved(f, markers, **kw):
    ce, w, sg = f.getWeights()
    return ResolvedReference(ce, w, sg, f.arcLengths, f.thickness, f._tr_off, f.nx, f.ny, uv_markers=markers[0],
                             tracer_markers=markers[1], class_markers=markers[2], reference=REF, **kw)


def _write_npz(tmp_path, real, grid):
    blon, blat, u, v, tau, sig = _case(real, grid)
    paths = {k: str(tmp_path / f'{k}.npz') for k in 'TUV'}
    fv = lambda name, a, b: {f'_FillValue_{name}': numpy.array(a), f'_missing_value_{name}': numpy.array(b)}   # noqa: E731
    numpy.savez(paths['T'], bounds_lon=blon, bounds_lat=blat, deptht_bounds=DB, tau=tau, sig=sig, **fv('tau', TFILL, TMISSING),
                **fv('sig', TFILL, TMISSING))
    numpy.savez(paths['U'], uo=u, **fv('uo', FILL, MISSING))
    numpy.savez(paths['V'], vo=v, **fv('vo', FILL, MISSING))
    return paths


@pytest.mark.parametrize('home', ['hbm', 'host', 'npz'])
@pytest.mark.parametrize('grid', GRIDS, ids=lambda g: f'{g[0]}x{g[1]}')
@pytest.mark.parametrize('real', ['float64', 'float32'])
def test_field_time_mean_against_the_restatement_and_the_resolved_reference(real, grid, home, tmp_path):
    from nemoflux_amd.field import Field
    if home == 'npz':
        paths = _write_npz(tmp_path, real, grid)
        src = _quiet(Field, paths['T'], paths['U'], paths['V'], _lines(), readback=False, unsupportedCells='refuse')
        assert src._uv_markers == (FILL, MISSING)
        src.setTracer((paths['T'], 'tau'), reference=REF)
        src.setClassTracer((paths['T'], 'sig'))
        src.setClassEdges(EDGES)
    else:
        src = _source(real, grid, home == 'hbm')
    blon, blat = _case(real, grid)[:2]
    for steps in (None, (1, 3)):
        t0, t1 = (0, NT) if steps is None else steps
        got = _quiet(src.timeMean, steps)
        assert (got.nt, got.nz, got.ny, got.nx) == (1, NZ, grid[1], grid[0]) and got._uv_code == NF_F64
        arrays, cls, (fill, tfill, sfill) = _mean_arrays(real, grid, t0, t1)
        assert fill == float(numpy.dtype(real).type(FILL)) and tfill == TFILL
        assert numpy.isinf(cls['class']).any() and (arrays['uo'] == fill).any() and (arrays['tracer'] == tfill).any()
        want = _field(blon, blat, DB, _on(arrays['uo'], True), _on(arrays['vo'], True), _lines(), readback=False, fill_value=fill)
        want.setTracer(_on(arrays['tracer'], True), fill_value=tfill, reference=REF)
        want.setClassTracer(_on(cls['class'], True), fill_value=sfill)
        want.setClassEdges(EDGES)
        rows, wrows = _products(got), _products(want)
        ref = _resolved(got, ((fill,), (tfill,), (sfill,))).step(array_values(dict(arrays, **cls), 0), edge_sets=[EDGES])
        for k in rows:
            assert numpy.abs(rows[k]).max() > 0, k
            assert numpy.array_equal(rows[k], wrows[k]), (steps, k)
            value, mag = ref[k]
            err = numpy.abs(rows[k] - value)
            print(f'{real} {grid} {home} {steps} {k}: max |err| / mag = {float((err / numpy.maximum(mag, 1e-300)).max()):.3g}')
            assert rows[k].shape == value.shape and numpy.all(err <= BAR * mag), (steps, k)


def test_step_by_step_file_input_gives_the_rows_of_the_arrays(tmp_path):
    """float32 record variables of a NetCDF-3 file are read one step at a time through one pinned buffer (uo, vo and a
    tracer): the rows of the mean state of the same arrays in memory, bit for bit"""
    from nemoflux_amd.field import Field
    real, grid = 'float32', GRIDS[1]
    blon, blat, u, v, _, _ = _case(real, grid)
    # the files carry one marker: _FillValue on uo, NaN in vo
    g = dict(u=numpy.where(numpy.isnan(u) | (u == numpy.float32(MISSING)), numpy.float32(FILL), u),
             v=numpy.where((v == numpy.float32(FILL)) | (v == numpy.float32(MISSING)), numpy.float32(numpy.nan), v),
             bounds_lon=blon, bounds_lat=blat, deptht_bounds=DB)
    paths, uf, vf = write_classic_triple(tmp_path, g)
    blon, blat = blon.astype(numpy.float32), blat.astype(numpy.float32)       # as the T file holds them
    ff = _quiet(Field, paths['T'], paths['U'], paths['V'], _lines(), readback=False, unsupportedCells='refuse')
    assert ff._lazy is not None
    ff.setTracer((paths['U'], 'uo'), reference=0.5)
    mem = _field(blon, blat, DB.astype(numpy.float32), uf, vf, _lines(), readback=False, fill_value=FILL)
    mem.setTracer(uf, fill_value=FILL, reference=0.5)
    for steps in (None, (1, 2)):
        a, b = _quiet(ff.timeMean, steps), _quiet(mem.timeMean, steps)
        for f in (a, b):
            f.computeFlux(0)
        assert numpy.abs(_row(b)).max() > 0 and numpy.array_equal(_row(a), _row(b))
        assert numpy.array_equal(_rows(a.computeTracerFlux(0)), _rows(b.computeTracerFlux(0)))


# ---- 5. anchors that need no reference -------------------------------------------------------------------------------------
def _step_mags(f, arrays, key):
    """sum |terms| of `key` for every step of the source arrays, and the values"""
    r = _resolved(f, ((FILL, MISSING), (TFILL, TMISSING), ()))
    both = dict(arrays, **{'class': arrays['tracer']})
    out = [r.step(array_values(both, t))[key] for t in range(NT)]
    return numpy.array([x[0] for x in out]), numpy.array([x[1] for x in out])


def _mean_mag(f, real, grid, key, **kw):
    arrays, cls, (fill, tfill, sfill) = _mean_arrays(real, grid, 0, NT, **kw)
    return _resolved(f, ((fill,), (tfill,), (sfill,))).step(array_values(dict(arrays, **cls), 0))[key][1]


@pytest.mark.parametrize('resident', [True, False], ids=['hbm', 'host'])
@pytest.mark.parametrize('grid', GRIDS, ids=lambda g: f'{g[0]}x{g[1]}')
@pytest.mark.parametrize('real', ['float64', 'float32'])
def test_flux_of_the_mean_state_is_the_mean_of_the_fluxes(real, grid, resident):
    """missing velocities count as 0 at every step and in the mean, so the volume row is linear in uo / vo although their
    markers vary in time.  Bar: 1e-12 x (mean over the steps of sum |terms| + sum |terms| of the mean state); the rounding of
    the means perturbs each term by at most (nt + 1) eps ~ 1e-15."""
    _, _, u, v, tau, _ = _case(real, grid)
    assert ((u[0] == u.dtype.type(FILL)) != (u[1] == u.dtype.type(FILL))).any() and (numpy.isnan(v[0]) != numpy.isnan(v[2])).any()
    f = _source(real, grid, resident)
    series = _rows(f.computeAll())
    m = _quiet(f.timeMean)
    m.computeFlux(0)
    _, mags = _step_mags(f, dict(uo=u, vo=v, tracer=tau), 'volume')
    bar = BAR * (mags.mean(axis=0) + _mean_mag(m, real, grid, 'volume'))
    err = numpy.abs(_row(m) - series.sum(axis=0) / NT)
    print(f'{real} {grid}: max |err| / bar = {float((err / numpy.maximum(bar, 1e-300)).max()):.3g} x 1e-12')
    assert numpy.abs(series).max() > 0 and bar[-3:].min() > 0 and numpy.all(err <= bar)


@pytest.mark.parametrize('constant', ['tracer', 'velocity'])
@pytest.mark.parametrize('grid', GRIDS, ids=lambda g: f'{g[0]}x{g[1]}')
@pytest.mark.parametrize('real', ['float64', 'float32'])
def test_eddy_part_vanishes_when_one_factor_is_constant_in_time(real, grid, constant):
    """a tracer constant in time (the velocity markers vary), or velocities constant in time with a tracer whose values vary
    but whose markers do not: total = mean, within the bar of the volume anchor taken for the tracer terms"""
    _, _, u, v, tau, _ = _case(real, grid)
    if constant == 'tracer':
        tau = numpy.ascontiguousarray(numpy.broadcast_to(tau[1], tau.shape))
    else:
        u, v = (numpy.ascontiguousarray(numpy.broadcast_to(x[1], x.shape)) for x in (u, v))
        keep = tau[0] != tau[0]
        tau = (4. + numpy.random.default_rng(9).random(tau.shape)).astype(real)
        tau[:, keep] = numpy.nan
        tau[:, :, 10:14, 50:60] = tau.dtype.type(TFILL)
    assert numpy.isfinite(tau[~numpy.isnan(tau)]).all()
    f = _source(real, grid, True, u=u, v=v, tau=tau, sig=False)
    d = _quiet(f.meanEddyTracerTransport)
    _, mags = _step_mags(f, dict(uo=u, vo=v, tracer=tau), 'tracer')
    bar = BAR * (mags.mean(axis=0) + _mean_mag(d['meanField'], real, grid, 'tracer', u=u, v=v, tau=tau))[-3:]
    print(f'{real} {grid} {constant}: max |eddy| / bar = {float((numpy.abs(d["eddy"]) / bar).max()):.3g} x 1e-12')
    assert numpy.abs(d['total']).min() > 0 and bar.min() > 0
    assert numpy.all(numpy.abs(d['eddy']) <= bar), (d['eddy'], bar)
    if constant == 'tracer':       # and with both factors varying it does not vanish
        e = _quiet(_source(real, grid, True, sig=False).meanEddyTracerTransport)
        assert numpy.all(numpy.abs(e['eddy']) > 1e3 * bar)


# ---- 6 - 7. the split and the command line ---------------------------------------------------------------------------------
@pytest.mark.parametrize('steps', [None, (1, 3)], ids=['all', '1to3'])
@pytest.mark.parametrize('resident', [True, False], ids=['hbm', 'host'])
def test_mean_eddy_split_is_assembled_from_the_series_and_the_mean_field(resident, steps):
    real, grid = 'float32', GRIDS[1]
    f = _source(real, grid, resident)
    d = _quiet(f.meanEddyTracerTransport, steps)
    t0, t1 = (0, NT) if steps is None else steps
    series = f.computeTracerAll()[0]
    total = series[t0:t1].sum(axis=0) / (t1 - t0)
    mean = _quiet(f.timeMean, steps).computeTracerFlux(0)[0]
    assert sorted(d) == ['eddy', 'mean', 'meanField', 'total']
    assert numpy.array_equal(d['total'], total) and numpy.array_equal(d['mean'], mean) and numpy.array_equal(d['eddy'], total - mean)
    assert d['total'].shape == (3,) and numpy.abs(d['eddy']).min() > 0
    assert numpy.array_equal(d['meanField'].computeTracerFlux(0)[0], mean) and d['meanField'].nt == 1
    # the mean Field takes the other calls: its decomposition adds up to its transport
    parts = d['meanField'].decomposeTracerTransport(0)
    assert numpy.array_equal(parts['total'], mean)


def test_fluxplot_eddy_writes_the_three_parts(tmp_path):
    from nemoflux_amd import fluxplot
    from nemoflux_amd.field import Field
    real, grid = 'float32', GRIDS[0]
    paths = _write_npz(tmp_path, real, grid)
    lines = "[" + "],[".join(LINES) + "]"
    tr = fluxplot.readTargets(lines)[0]
    f = _quiet(Field, paths['T'], paths['U'], paths['V'], tr, True, readback=False, compact=True)
    f.setTracer((paths['T'], 'tau'), reference=REF)
    d = _quiet(f.meanEddyTracerTransport)
    want = numpy.array([d[k] for k in ('total', 'mean', 'eddy')]) * 2.5
    out = str(tmp_path / 'eddy.csv')
    got = _quiet(fluxplot.main, tFile=paths['T'], uFile=paths['U'], vFile=paths['V'], lonLatPoints=lines, sverdrup=True,
                 tracer='tau', tracerRef=REF, tracerScale=2.5, eddy=True, output=out)
    assert numpy.array_equal(got, want) and numpy.abs(want).min() > 0
    with open(out) as fh:
        text = fh.read().splitlines()
    assert text[0].startswith('# mean transport of tau over 3 time steps') and 'tau x Sv x 2.5' in text[0]
    assert text[1] == 'part,line0,line1,line2' and [ln.split(',')[0] for ln in text[2:]] == ['total', 'mean', 'eddy']
    table = numpy.array([[float(x) for x in ln.split(',')[1:]] for ln in text[2:]])
    assert numpy.allclose(table, want, rtol=1e-14, atol=0)


# ---- 8 - 9. refusals, carried state, the source --------------------------------------------------------------------------
def test_refusals():
    real, grid = 'float64', GRIDS[0]
    _, _, u, _, _, _ = _case(real, grid)
    f = _source(real, grid, True)
    e3 = numpy.ascontiguousarray(numpy.broadcast_to(TH[None, :, None, None], u.shape))
    f.setCellThickness(_on(e3, True), _on(e3.copy(), True))
    for call in (f.timeMean, f.meanEddyTracerTransport):
        with pytest.raises(RuntimeError, match='the mean state of a time-varying cell thickness is not defined here'):
            call()
    f.setCellThickness(None, None)
    _quiet(f.timeMean)
    g = _source(real, grid, True, slab_range=(3, 12))
    for call in (g.timeMean, g.meanEddyTracerTransport):
        with pytest.raises(RuntimeError, match='slab_range'):
            call()
    blon, blat = _case(real, grid)[:2]
    h = _field(blon, blat, DB, _on(u, True), _on(u, True), _lines(), readback=False)
    with pytest.raises(RuntimeError, match='setTracer first'):
        h.meanEddyTracerTransport()
    for bad in ((0, 0), (2, 1), (0, NT + 1)):
        with pytest.raises(RuntimeError, match='half-open'):
            h.timeMean(bad)
    m = _quiet(h.timeMean, (0, 1))         # no tracer: a mean state without one, with the source's (absent) fill
    assert getattr(m, '_tracer', None) is None and m._uv_markers[0] != m._uv_markers[0]


@pytest.mark.parametrize('resident', [True, False], ids=['hbm', 'host'])
def test_static_cell_thickness_is_carried_over_as_float64(resident):
    real, grid = 'float32', GRIDS[0]
    nx, ny = grid
    rng = numpy.random.default_rng(13)
    e3u, e3v = (rng.uniform(0.2, 3., (NZ, ny, nx)).astype(real) for _ in range(2))
    e3u[2:, 5:9, 30:40] = numpy.float32(-1.e30)
    f = _source(real, grid, resident, sig=False)
    f.setCellThickness(_on(e3u, resident), _on(e3v, resident), fill_value=-1.e30)
    m = _quiet(f.timeMean)
    arrays, _, (fill, tfill, _) = _mean_arrays(real, grid, 0, NT)
    blon, blat = _case(real, grid)[:2]
    want = _field(blon, blat, DB, _on(arrays['uo'], True), _on(arrays['vo'], True), _lines(), readback=False, fill_value=fill)
    want.setTracer(_on(arrays['tracer'], True), fill_value=tfill, reference=REF)
    plain = want.computeFlux(0)
    want.setCellThickness(e3u.astype(numpy.float64), e3v.astype(numpy.float64), fill_value=float(numpy.float32(-1.e30)))
    assert m.computeFlux(0) == want.computeFlux(0) != plain
    assert numpy.array_equal(_row(m), _row(want))
    assert numpy.array_equal(_rows(m.computeTracerFlux(0)), _rows(want.computeTracerFlux(0)))


@pytest.mark.parametrize('resident', [True, False], ids=['hbm', 'host'])
def test_source_field_is_left_as_it_was(resident):
    from nemoflux_amd import _lib
    from nemoflux_amd._lib import lib, check
    real, grid = 'float64', GRIDS[1]
    f = _source(real, grid, resident, readback=True)

    def state():
        n = f.ny * f.nx
        iV, eU, eV, mx = numpy.zeros((n, 4)), numpy.zeros(n), numpy.zeros(n), ctypes.c_double()
        check(lib.nf_field_read_step(ctypes.byref(f._h), _lib.dptr(iV), _lib.dptr(eU), _lib.dptr(eV), ctypes.byref(mx)))
        return [iV, eU, eV, numpy.array(mx.value), _row(f), numpy.array(f.maxAbsFlux), numpy.array(f.timeIndex)]

    f.computeFlux(2, readback=True)
    rows = {t: _rows(f.computeTracerFlux(t)) for t in range(NT)}
    f.computeFlux(1, readback=True)
    before = state()
    assert before[5] > 0 and numpy.abs(before[4]).max() > 0
    _quiet(f.timeMean)
    _quiet(f.timeMean, (0, 2))
    for x, y in zip(state(), before):
        assert numpy.array_equal(x, y)
    for t in range(NT):
        assert numpy.array_equal(_rows(f.computeTracerFlux(t)), rows[t])
    f.computeFlux(1, readback=True)         # the running max has not moved either
    for x, y in zip(state(), before):
        assert numpy.array_equal(x, y)
