"""Thickness-weighted time means on the GPU: nf_time_mean_weighted against the numpy restatement of
tests/weighted_mean_reference.py bit for bit (both dtypes, vector and one-value-per-lane paths, strides that differ between the
two series, an odd base pointer on either series, series split over calls, offsets beyond 2^31 elements);
Field.timeMean(thicknessWeighted=True) with the velocities and the thicknesses in HBM, on the host, in .npz files, read step by
step from NetCDF-3 files and in mixed homes, against a Field built from the restatement's arrays (bit for bit); anchors that
need no reference (the flux of the weighted mean state is the mean of the fluxes; with a tracer constant in time the eddy part
vanishes with the weighting and does not without it; power-of-two thicknesses constant in time give the plain mean; a static
thickness gives timeMean()); Field.meanEddyTracerTransport(thicknessWeighted=True) and fluxplot --thickness-weighted; the source
Field is left as it was.

Grids 72 x 36 x 7 x 3 and 73 x 37 x 7 x 3 (odd: every other step of an array is not 16-byte aligned).  No +-inf in the
velocities and thicknesses of this file: 0 x inf is NaN here as in every flux kernel.

Measured on an MI355X: the anchors' worst error 2.4e-4 of their bar (volume and profile rows) and 4.3e-5 (the eddy part of a
constant tracer); the eddy part that the plain means leave is 8.6e8 x the bar or more; 52 tests in 3.5 s."""
import ctypes

import numpy
import pytest

from conftest import transect_xyz, write_classic_triple
from cellthick_reference import CellThickReference, array_values
from gpu_helpers import _field, _on, _quiet, _rows
import timemean_reference as tmr
import weighted_mean_reference as wmr

pytestmark = pytest.mark.gpu

PSI_ZT = "(1+10*z)*(t+1)*(cos(2*pi*y/360) + sin(2*pi*x/360))"
LINES = ["(-100,-80),(100,-80),(0,80)", "(-100,-80),(100,-80),(0,80),(-100,-80)", "(150,-30),(179.5,-20),(179.9,10),(175,40)"]
NZ, NT = 7, 3
GRIDS = [(72, 36), (73, 37)]
FILL, MISSING = 1.e20, -999.             # uo / vo
TFILL, TMISSING = -32768., 12345.        # tracer
THFILL, THMISSING = -1.e30, 9999.        # e3u / e3v
REF = 4.25
BAR = 1e-12
TH = numpy.array([0.125, 0.25, 0.5, 0.375, 0.75, 1.0, 0.625])
DB = numpy.stack([numpy.concatenate([[0.], numpy.cumsum(TH)[:-1]]), numpy.cumsum(TH)], axis=1)
TH2 = numpy.array([0.125, 0.25, 0.5, 0.25, 1.0, 2.0, 0.5])       # powers of two: anchor (c)
DB2 = numpy.stack([numpy.concatenate([[0.], numpy.cumsum(TH2)[:-1]]), numpy.cumsum(TH2)], axis=1)
NF_F64, NF_F32 = 0, 1
US = 4                                   # kTimeMeanWeightedSteps of nf_timemean.hip: the steps a lane has in flight


def _row(f):
    return numpy.array(f._row[:f._rowlen])


# ---- 1 - 3. the raw ABI ----------------------------------------------------------------------------------------------------
def _series(real, nsteps, strides, n, offsets, seed):
    """two buffers that hold nsteps windows of n values each, step t at offset + t * stride: velocities (random, NaN, both
    markers, -0.0, a value missing at every step) and thicknesses (0.2 .. 3, NaN, both markers, exact zeros, a value that is
    zero at every step); no +-inf"""
    rng = numpy.random.default_rng(seed)
    dt = numpy.dtype(real).type
    win = rng.standard_normal((nsteps, n)).astype(real)
    hwin = rng.uniform(0.2, 3., (nsteps, n)).astype(real)
    for w, marks in ((win, (numpy.nan, FILL, MISSING, -0.0)), (hwin, (numpy.nan, THFILL, THMISSING, 0.0))):
        flat = w.reshape(-1)
        for m in marks:
            flat[rng.choice(flat.size, (flat.size + 7) // 8, replace=False)] = dt(m)
    if n >= 3:
        cols = rng.choice(n, 2, replace=False)
        win[:, cols[0]] = [(dt(FILL), numpy.nan, dt(MISSING))[t % 3] for t in range(nsteps)]      # missing at every step
        hwin[:, cols[0]] = dt(1.5)
        win[:, cols[1]] = dt(0.75)
        hwin[:, cols[1]] = [(dt(0.0), numpy.nan, dt(THFILL))[t % 3] for t in range(nsteps)]       # never any water
    bufs = []
    for w, stride, offset in zip((win, hwin), strides, offsets):
        buf = numpy.full(offset + (nsteps - 1) * stride + n + 4, 7.25, real)       # what lies between the windows is never read
        for t in range(nsteps):
            buf[offset + t * stride:offset + t * stride + n] = w[t]
        bufs.append(buf)
    return bufs, win, hwin


def _call(devs, offsets, nsteps, strides, n, code, first, last, total, fill_out, accf, acch, cnt, itemsize):
    """nf_time_mean_weighted on the windows of the device buffers `devs`; accf / acch / cnt: tensors with two (four) guard
    values on each side"""
    from nemoflux_amd._lib import lib, check
    check(lib.nf_time_mean_weighted(accf.data_ptr() + 16, acch.data_ptr() + 16, None if cnt is None else cnt.data_ptr() + 16,
                                    devs[0].data_ptr() + offsets[0] * itemsize, strides[0],
                                    devs[1].data_ptr() + offsets[1] * itemsize, strides[1], nsteps, n, code, FILL, MISSING,
                                    THFILL, THMISSING, first, last, total, fill_out, None))
    check(lib.nf_synchronize())


def _guards():
    import torch
    return (lambda n: torch.full((n + 4,), -7.0, dtype=torch.float64, device='cuda'),
            lambda n: torch.full((n + 8,), 77, dtype=torch.int32, device='cuda'))


def _acc_of(acc, n):
    a = acc.cpu().numpy()
    assert (a[:2] == -7.0).all() and (a[n + 2:] == -7.0).all(), 'accf / acch was written outside its n values'
    return a[2:n + 2]


def _cnt_of(cnt, n):
    c = cnt.cpu().numpy()
    assert (c[:4] == 77).all() and (c[n + 4:] == 77).all(), 'cnt was written outside its n values'
    return c[4:n + 4].view(numpy.uint32)


@pytest.mark.parametrize('real', ['float64', 'float32'])
def test_raw_abi_is_the_restatement_bit_for_bit(real):
    """one call that finishes (the weighted mean and the mean thickness) and one that carries (sF, sH and c); n below, at and
    above a block and odd; 1 .. 2 US + 1 steps (fewer, as many and more than a lane has in flight); contiguous steps, padded
    steps whose strides differ between the series (16-byte aligned, and not), an odd base pointer on one series only"""
    import torch
    code, itemsize = (NF_F64, 8) if real == 'float64' else (NF_F32, 4)
    fill_out = float(numpy.dtype(real).type(FILL))
    new_acc, new_cnt = _guards()
    seed = 0
    for n in (1, 3, 255, 256, 257, 18907):
        a = (n + 7) // 4 * 4        # padded steps that stay 16-byte aligned in both dtypes: the 16-byte path, also for an odd n
        shapes = [((n, n), (0, 0)), ((a, a + 4), (0, 0)), ((n + 3, n + 5), (0, 0)), ((a, a + 4), (1, 0)), ((a, a + 4), (0, 1))]
        for nsteps in range(1, 2 * US + 2):
            for strides, offsets in shapes:
                seed += 1
                bufs, win, hwin = _series(real, nsteps, strides, n, offsets, seed)
                devs = [torch.from_numpy(b).cuda() for b in bufs]
                label = (n, nsteps, strides, offsets)
                total = nsteps + 2          # not nsteps: the divisor is the argument
                accf, acch, cnt = new_acc(n), new_acc(n), new_cnt(n)
                _call(devs, offsets, nsteps, strides, n, code, 1, 1, total, fill_out, accf, acch, None, itemsize)
                want, want_h = wmr.weighted_time_mean(win, hwin, (FILL, MISSING), (THFILL, THMISSING), total, fill_out)
                assert wmr.same_bits(_acc_of(accf, n), want), label
                assert wmr.same_bits(_acc_of(acch, n), want_h), label
                _call(devs, offsets, nsteps, strides, n, code, 1, 0, total, fill_out, accf, acch, cnt, itemsize)
                sF, sH, c = wmr.accumulate(win, hwin, (FILL, MISSING), (THFILL, THMISSING))
                assert wmr.same_bits(_acc_of(accf, n), sF) and wmr.same_bits(_acc_of(acch, n), sH), label
                assert numpy.array_equal(_cnt_of(cnt, n), c.reshape(-1)), label
                assert numpy.isfinite(want_h).all() and numpy.isfinite(want).all()
                if n >= 3:
                    assert (c == 0).any() and (want[c == 0] == fill_out).all()
                    assert ((sH == 0) & (c > 0)).any() and (want[(sH == 0) & (c > 0)] == 0).all()


@pytest.mark.parametrize('real', ['float64', 'float32'])
def test_series_split_over_calls_is_one_call_bit_for_bit(real):
    """7 steps as every cut into two calls and as 2 + 1 + 4 (first on the first call only, last on the last only); each call
    takes the 16-byte path or one value per lane as its own steps are aligned: the same bits"""
    import torch
    code, itemsize = (NF_F64, 8) if real == 'float64' else (NF_F32, 4)
    fill_out = numpy.nan
    new_acc, new_cnt = _guards()
    for n, strides in ((18907, (18907, 18907)), (18907, (18908, 18912)), (257, (260, 264)), (3, (3, 3))):
        bufs, win, hwin = _series(real, 7, strides, n, (0, 0), 200 + n + strides[1])
        devs = [torch.from_numpy(b).cuda() for b in bufs]
        one_f, one_h = new_acc(n), new_acc(n)
        _call(devs, (0, 0), 7, strides, n, code, 1, 1, 7, fill_out, one_f, one_h, None, itemsize)
        want, want_h = wmr.weighted_time_mean(win, hwin, (FILL, MISSING), (THFILL, THMISSING), 7, fill_out)
        assert wmr.same_bits(_acc_of(one_f, n), want) and wmr.same_bits(_acc_of(one_h, n), want_h), (n, strides)
        for cuts in [(k, 7 - k) for k in range(1, 7)] + [(2, 1, 4)]:
            accf, acch, cnt = new_acc(n), new_acc(n), new_cnt(n)
            t = 0
            for k in cuts:
                _call(devs, (t * strides[0], t * strides[1]), k, strides, n, code, 1 if t == 0 else 0, 1 if t + k == 7 else 0, 7,
                      fill_out, accf, acch, cnt, itemsize)
                t += k
            assert wmr.same_bits(_acc_of(accf, n), want) and wmr.same_bits(_acc_of(acch, n), want_h), (n, strides, cuts)
        assert numpy.isnan(want).any() and numpy.isfinite(want).any()


def test_offsets_beyond_2_to_the_31_elements():
    """two steps 2^31 + 5 (one value per lane) and 2^31 + 8 (16-byte path) float32 elements apart; one uninitialised
    allocation serves both series, the thickness 2048 elements behind the velocity; only the windows are written"""
    import torch
    n, shift = 1000, 2048
    big = torch.empty(2 ** 31 + 8 + shift + n, dtype=torch.float32, device='cuda')
    new_acc, _ = _guards()
    for stride in (2 ** 31 + 5, 2 ** 31 + 8):
        _, win, hwin = _series('float32', 2, (n, n), n, (0, 0), 7)
        win[1] += numpy.float32(100.)          # a result that read step 0 twice, or step 1 at a wrapped offset, is far off
        hwin[1][wmr.present(hwin[1], (THFILL, THMISSING))] *= numpy.float32(16.)
        for t in range(2):
            big[t * stride:t * stride + n] = torch.from_numpy(win[t]).cuda()
            big[shift + t * stride:shift + t * stride + n] = torch.from_numpy(hwin[t]).cuda()
        accf, acch = new_acc(n), new_acc(n)
        _call((big, big), (0, shift), 2, (stride, stride), n, NF_F32, 1, 1, 2, numpy.nan, accf, acch, None, 4)
        want, want_h = wmr.weighted_time_mean(win, hwin, (FILL, MISSING), (THFILL, THMISSING), 2, numpy.nan)
        assert wmr.same_bits(_acc_of(accf, n), want) and wmr.same_bits(_acc_of(acch, n), want_h), stride
    del big
    torch.cuda.empty_cache()


# ---- 4. Field.timeMean(thicknessWeighted=True) -----------------------------------------------------------------------------
_CASES = {}


def _case(real, grid):
    """bounds; host u, v (nt, nz, ny, nx) with a land block and markers of all three kinds that come and go with time, and
    the same before the markers went in; a carried tracer (NaN and both markers, some varying in time); e3u, e3v: independent,
    time-varying, in [0.2, 3], with their own markers, NaN and exact zeros that come and go, and a block without water at any
    step under present velocities"""
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
        clean = (u.copy(), v.copy())
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
        e3 = [_thickness_markers(rng.uniform(0.2, 3., (NT, NZ, ny, nx)).astype(real), rng) for _ in range(2)]
        _CASES[key] = (dg.bounds_lon.cpu().numpy(), dg.bounds_lat.cpu().numpy(), u, v, tau, e3[0], e3[1], clean)
    return _CASES[key]


def _thickness_markers(e3, rng):
    dt = e3.dtype.type
    flat = e3.reshape(-1)
    for m in (THFILL, THMISSING, numpy.nan, 0.0):
        flat[rng.choice(flat.size, flat.size // 25, replace=False)] = dt(m)
    e3[0, 5:, 20:24, 30:45] = dt(0.0)                # below the bottom: never any water
    e3[1, 5:, 20:24, 30:45] = numpy.nan
    e3[2, 5:, 20:24, 30:45] = dt(THFILL)
    return e3


def _lines():
    return [transect_xyz(s) for s in LINES]


def _source(real, grid, uv_resident, th_resident=None, u=None, v=None, tau=None, e3u=None, e3v=None, db=DB, **kw):
    """a Field of the case with a time-varying cell thickness; uv_resident / th_resident: in HBM, or on the host"""
    blon, blat, u0, v0, tau0, e3u0, e3v0, _ = _case(real, grid)
    th_resident = uv_resident if th_resident is None else th_resident
    kw.setdefault('readback', False)
    f = _field(blon, blat, db, _on(u0 if u is None else u, uv_resident), _on(v0 if v is None else v, uv_resident), _lines(),
               fill_value=FILL, missing_value=MISSING, **kw)
    f.setTracer(_on(tau0 if tau is None else tau, uv_resident), fill_value=TFILL, missing_value=TMISSING, reference=REF)
    f.setCellThickness(_on(e3u0 if e3u is None else e3u, th_resident), _on(e3v0 if e3v is None else e3v, th_resident),
                       fill_value=THFILL, missing_value=THMISSING)
    return f


def _products(f):
    """the rows of every product that takes a cell thickness, of step 0, as [segments | transects]"""
    f.computeFlux(0)
    area, tarea = f.computeAreaProfile(0)
    return {'volume': _row(f), 'volume_profile': _rows(f.computeFluxProfile(0)), 'tracer': _rows(f.computeTracerFlux(0)),
            'area': _rows(area), 'tracer_area': _rows(tarea), 'gross': _rows(f.computeGrossProfile(0)),
            'gross_carried': _rows(f.computeGrossProfile(0, carry=True))}


def _mean_arrays(real, grid, t0, t1, u=None, v=None, tau=None, e3u=None, e3v=None, uv_markers=(FILL, MISSING),
                 tracer_markers=(TFILL, TMISSING), thick_markers=(THFILL, THMISSING)):
    """the restatement's arrays of the weighted mean state: {'uo', 'vo', 'tracer', 'e3u', 'e3v'} (1, nz, ny, nx) float64 and
    the fills (velocities, tracer)"""
    _, _, u0, v0, tau0, e3u0, e3v0, _ = _case(real, grid)
    pick = lambda a, b: (b if a is None else a)[t0:t1]   # noqa: E731
    (um, vm, fill), (hu, hv) = wmr.field_weighted_mean_arrays(pick(u, u0), pick(v, v0), uv_markers, pick(e3u, e3u0),
                                                              pick(e3v, e3v0), thick_markers)
    _, ((taum, tfill),) = tmr.field_mean_arrays(pick(u, u0), pick(v, v0), uv_markers, [(pick(tau, tau0), tracer_markers)])
    return dict(uo=um, vo=vm, tracer=taum, e3u=hu, e3v=hv), (fill, tfill)


def _want_field(blon, blat, arrays, fills, db=DB):
    """fromArrays of the restatement's arrays plus a static float64 setCellThickness"""
    fill, tfill = fills
    f = _field(blon, blat, db, _on(arrays['uo'], True), _on(arrays['vo'], True), _lines(), readback=False, fill_value=fill)
    f.setTracer(_on(arrays['tracer'], True), fill_value=None if tfill != tfill else tfill, reference=REF)
    f.setCellThickness(_on(arrays['e3u'], True), _on(arrays['e3v'], True))
    return f


def _write_npz(tmp_path, real, grid):
    blon, blat, u, v, tau, e3u, e3v, _ = _case(real, grid)
    paths = {k: str(tmp_path / f'{k}.npz') for k in 'TUV'}
    fv = lambda name, a, b: {f'_FillValue_{name}': numpy.array(a), f'_missing_value_{name}': numpy.array(b)}   # noqa: E731
    numpy.savez(paths['T'], bounds_lon=blon, bounds_lat=blat, deptht_bounds=DB, tau=tau, **fv('tau', TFILL, TMISSING))
    numpy.savez(paths['U'], uo=u, e3u=e3u, **fv('uo', FILL, MISSING), **fv('e3u', THFILL, THMISSING))
    numpy.savez(paths['V'], vo=v, e3v=e3v, **fv('vo', FILL, MISSING), **fv('e3v', THFILL, THMISSING))
    return paths


@pytest.mark.parametrize('home', ['hbm', 'host', 'npz', 'uv_hbm_e3_host', 'uv_host_e3_hbm'])
@pytest.mark.parametrize('grid', GRIDS, ids=lambda g: f'{g[0]}x{g[1]}')
@pytest.mark.parametrize('real', ['float64', 'float32'])
def test_weighted_time_mean_against_a_field_of_the_restatement(real, grid, home, tmp_path):
    from nemoflux_amd.field import Field
    if home == 'npz':
        paths = _write_npz(tmp_path, real, grid)
        src = _quiet(Field, paths['T'], paths['U'], paths['V'], _lines(), readback=False, unsupportedCells='refuse')
        src.setTracer((paths['T'], 'tau'), reference=REF)
        src.setCellThickness((paths['U'], 'e3u'), (paths['V'], 'e3v'))
        assert (src._e3['fill'], src._e3['missing'], src._e3['nt']) == (THFILL, THMISSING, NT)
    else:
        src = _source(real, grid, home in ('hbm', 'uv_hbm_e3_host'), home in ('hbm', 'uv_host_e3_hbm'))
        if grid == GRIDS[1]:
            src._MEAN_STAGE_BYTES = 1          # host arrays go up one step at a time, sF, sH and c carried between the calls
    blon, blat = _case(real, grid)[:2]
    for steps in (None, (1, 3)):
        t0, t1 = (0, NT) if steps is None else steps
        got = _quiet(src.timeMean, steps, thicknessWeighted=True)
        assert (got.nt, got.nz, got.ny, got.nx) == (1, NZ, grid[1], grid[0]) and got._uv_code == NF_F64
        assert got._e3['nt'] == 1 and got._e3['fill'] != got._e3['fill'] and got._e3['missing'] != got._e3['missing']
        arrays, fills = _mean_arrays(real, grid, t0, t1)
        assert fills == (float(numpy.dtype(real).type(FILL)), TFILL)
        assert (arrays['uo'] == fills[0]).any() and (arrays['e3u'] == 0).any() and (arrays['e3u'] > 0).any()
        assert ((arrays['e3u'] == 0) & (arrays['uo'] == 0)).any()        # a present velocity that never had any water
        want = _want_field(blon, blat, arrays, fills)
        rows, wrows = _products(got), _products(want)
        for k in rows:
            assert numpy.abs(rows[k]).max() > 0, k
            assert numpy.array_equal(rows[k], wrows[k]), (steps, k)


def _write_classic(path, name, a, fill):
    """a (nt, nz, ny, nx) float32 record variable over an unlimited time axis, big-endian"""
    from scipy.io import netcdf_file
    nt, nz, ny, nx = a.shape
    f = netcdf_file(path, 'w', version=2)
    for n, s in (('time_counter', None), ('depth', nz), ('y', ny), ('x', nx)):
        f.createDimension(n, s)
    var = f.createVariable(name, 'f4', ('time_counter', 'depth', 'y', 'x'))
    var._FillValue = numpy.float32(fill)
    var[:] = a
    f.close()


@pytest.mark.parametrize('lazy', ['both', 'thickness'])
def test_step_by_step_file_input_gives_the_rows_of_the_arrays(tmp_path, lazy):
    """float32 record variables of NetCDF-3 files are read one step at a time through pinned buffers -- uo, vo and the
    thicknesses, or the thicknesses alone beside velocities in HBM: the rows of the weighted mean state of the same arrays in
    memory, bit for bit"""
    from nemoflux_amd.field import Field
    real, grid = 'float32', GRIDS[1]
    blon, blat, u, v, _, e3u, e3v, _ = _case(real, grid)
    f32 = numpy.float32
    # the files carry one marker per variable
    g = dict(u=numpy.where(numpy.isnan(u) | (u == f32(MISSING)), f32(FILL), u),
             v=numpy.where((v == f32(FILL)) | (v == f32(MISSING)), f32(numpy.nan), v),
             bounds_lon=blon, bounds_lat=blat, deptht_bounds=DB)
    paths, uf, vf = write_classic_triple(tmp_path, g)
    e3u, e3v = (numpy.where(x == f32(THMISSING), f32(THFILL), x) for x in (e3u, e3v))
    pu, pv = str(tmp_path / 'e3u.nc'), str(tmp_path / 'e3v.nc')
    _write_classic(pu, 'e3u', e3u, THFILL)
    _write_classic(pv, 'e3v', e3v, THFILL)
    blon, blat = blon.astype(f32), blat.astype(f32)       # as the T file holds them
    if lazy == 'both':
        ff = _quiet(Field, paths['T'], paths['U'], paths['V'], _lines(), readback=False, unsupportedCells='refuse')
        assert ff._lazy is not None
    else:
        ff = _field(blon, blat, DB.astype(f32), _on(uf, True), _on(vf, True), _lines(), readback=False, fill_value=FILL)
    ff.setTracer((paths['U'], 'uo'), reference=0.5)
    ff.setCellThickness((pu, 'e3u'), (pv, 'e3v'))
    assert ff._cell_thickness_lazy()
    mem = _field(blon, blat, DB.astype(f32), uf, vf, _lines(), readback=False, fill_value=FILL)
    mem.setTracer(uf, fill_value=FILL, reference=0.5)
    mem.setCellThickness(e3u, e3v, fill_value=THFILL)
    for steps in (None, (1, 2)):
        a, b = _quiet(ff.timeMean, steps, thicknessWeighted=True), _quiet(mem.timeMean, steps, True)
        ra, rb = _products(a), _products(b)
        for k in ra:
            assert numpy.abs(rb[k]).max() > 0 and numpy.array_equal(ra[k], rb[k]), (steps, k)
    for t in (2, 0):                            # the file-backed source still computes its own steps
        ff.computeFlux(t), mem.computeFlux(t)
        assert numpy.array_equal(_row(ff), _row(mem))


# ---- 5. anchors that need no reference -------------------------------------------------------------------------------------
def _reference(f, uv_markers, tracer_markers, thick_markers):
    ce, w, sg = f.getWeights()
    return CellThickReference(ce, w, sg, f.arcLengths, f.thickness, f._tr_off, f.nx, f.ny, uv_markers=uv_markers,
                              tracer_markers=tracer_markers, thick_markers=thick_markers, reference=REF, wrap=True)


def _bars(f, source_arrays, mean_arrays, fills, keys):
    """BAR x (mean over the steps of sum |terms| of the source + sum |terms| of the mean state), on the host from getWeights()"""
    src = _reference(f, (FILL, MISSING), (TFILL, TMISSING), (THFILL, THMISSING))
    steps = [src.step(array_values(source_arrays, t)) for t in range(NT)]
    mean = _reference(f, (fills[0],), (fills[1],), ()).step(array_values(mean_arrays, 0))
    return {k: BAR * (numpy.array([s[k][1] for s in steps]).mean(axis=0) + mean[k][1]) for k in keys}


@pytest.mark.parametrize('resident', [True, False], ids=['hbm', 'host'])
@pytest.mark.parametrize('grid', GRIDS, ids=lambda g: f'{g[0]}x{g[1]}')
@pytest.mark.parametrize('real', ['float64', 'float32'])
def test_flux_of_the_weighted_mean_state_is_the_mean_of_the_fluxes(real, grid, resident):
    """(mean thickness) x (weighted mean velocity) = (sH / nt) (sF / sH) is the mean of thickness x velocity up to 1.2 ulp per
    term, although the markers of both vary in time: the volume row and the rows of the volume profile of the mean state are
    the means over the steps of the source's rows.  Bar: 1e-12 x (mean over the steps of sum |terms| + sum |terms| of the
    mean state)."""
    _, _, u, v, tau, e3u, e3v, _ = _case(real, grid)
    f = _source(real, grid, resident)
    series = _rows(f.computeAll())
    profiles = numpy.array([_rows(f.computeFluxProfile(t)) for t in range(NT)])
    m = _quiet(f.timeMean, thicknessWeighted=True)
    m.computeFlux(0)
    arrays, fills = _mean_arrays(real, grid, 0, NT)
    bars = _bars(f, dict(uo=u, vo=v, tracer=tau, e3u=e3u, e3v=e3v), arrays, fills, ('volume', 'volume_profile'))
    for k, got, want in (('volume', _row(m), series.sum(axis=0) / NT),
                         ('volume_profile', _rows(m.computeFluxProfile(0)), profiles.sum(axis=0) / NT)):
        err, bar = numpy.abs(got - want), bars[k]
        print(f'{real} {grid} {k}: max |err| / bar = {float((err / numpy.maximum(bar, 1e-300)).max()):.3g} x 1e-12')
        assert got.shape == want.shape == bar.shape and numpy.abs(want).max() > 0
        assert bar[..., -3:].min() > 0 and numpy.all(err <= bar), k


def _plain_mean_field(f, real, grid, u, v, tau, e3u, e3v):
    """the split a user builds by hand from the plain means: nf_time_mean of uo, vo, e3u, e3v (the thickness under
    NF_MEAN_OVER_STEPS, 0 where it is never there), then fromArrays and setCellThickness"""
    import torch
    from nemoflux_amd import _lib
    from nemoflux_amd._lib import lib, check
    code = NF_F64 if real == 'float64' else NF_F32
    n = u[0].size
    fill = float(numpy.dtype(real).type(FILL))

    def mean(a, markers, fill_out):
        dev = _on(a, True)
        acc = torch.empty((1,) + a.shape[1:], dtype=torch.float64, device='cuda')
        check(lib.nf_time_mean(acc.data_ptr(), None, dev.data_ptr(), NT, n, n, code, markers[0], markers[1], 1, 1,
                               _lib.NF_MEAN_OVER_STEPS, NT, fill_out, None))
        check(lib.nf_synchronize())
        return acc

    blon, blat = _case(real, grid)[:2]
    p = _field(blon, blat, DB, mean(u, (FILL, MISSING), fill), mean(v, (FILL, MISSING), fill), _lines(), readback=False,
               fill_value=fill)
    p.setTracer(_on(tmr.time_mean(tau, (TFILL, TMISSING), tmr.OVER_PRESENT, NT, TFILL)[None], True), fill_value=TFILL, reference=REF)
    p.setCellThickness(mean(e3u, (THFILL, THMISSING), 0.0), mean(e3v, (THFILL, THMISSING), 0.0))
    return p


@pytest.mark.parametrize('grid', GRIDS, ids=lambda g: f'{g[0]}x{g[1]}')
@pytest.mark.parametrize('real', ['float64', 'float32'])
def test_eddy_part_vanishes_for_a_constant_tracer_only_with_the_weighting(real, grid):
    """a tracer constant in time, velocities and thicknesses that vary, the thickness correlated with the velocity
    (e3 = 1 + 0.5 tanh(u / median |u|) before the markers go in): total = mean within the bar of the volume anchor taken for
    the tracer terms.  The same split built by hand from the plain means of uo, vo, e3u, e3v leaves <e3' u'> in the eddy part:
    more than 1e3 x the bar."""
    _, _, u, v, tau, _, _, (uc, vc) = _case(real, grid)
    tau = numpy.ascontiguousarray(numpy.broadcast_to(tau[1], tau.shape))
    rng = numpy.random.default_rng(17)
    e3u, e3v = (_thickness_markers((1. + 0.5 * numpy.tanh(x.astype(numpy.float64) / numpy.median(numpy.abs(x[x != 0]))))
                                   .astype(real), rng) for x in (uc, vc))
    ok = wmr.present(e3u, (THFILL, THMISSING))
    assert e3u[ok].min() >= 0 and e3u[ok].max() <= 1.5 and (e3u[0][ok[0] & ok[2]] != e3u[2][ok[0] & ok[2]]).any()
    f = _source(real, grid, True, tau=tau, e3u=e3u, e3v=e3v)
    d = _quiet(f.meanEddyTracerTransport, thicknessWeighted=True)
    arrays, fills = _mean_arrays(real, grid, 0, NT, tau=tau, e3u=e3u, e3v=e3v)
    bar = _bars(f, dict(uo=u, vo=v, tracer=tau, e3u=e3u, e3v=e3v), arrays, fills, ('tracer',))['tracer'][-3:]
    print(f'{real} {grid}: max |eddy| / bar = {float((numpy.abs(d["eddy"]) / bar).max()):.3g} x 1e-12')
    assert numpy.abs(d['total']).min() > 0 and bar.min() > 0
    assert numpy.all(numpy.abs(d['eddy']) <= bar), (d['eddy'], bar)
    plain = _plain_mean_field(f, real, grid, u, v, tau, e3u, e3v)
    eddy = d['total'] - numpy.array(plain.computeTracerFlux(0)[0])
    print(f'{real} {grid}: plain means, min |eddy| / bar = {float((numpy.abs(eddy) / bar).min()):.3g} x 1e-12')
    assert numpy.all(numpy.abs(eddy) > 1e3 * bar), (eddy, bar)


@pytest.mark.parametrize('grid', GRIDS, ids=lambda g: f'{g[0]}x{g[1]}')
@pytest.mark.parametrize('real', ['float64', 'float32'])
def test_power_of_two_thickness_constant_in_time_gives_the_plain_mean(real, grid):
    """a time-varying thickness array whose steps are all the per-level powers of two TH2 (deptht_bounds from their running
    sum): sF / sH has the bits of the plain mean and sH / nt those of the thickness
    (tests/test_weighted_mean_cpu.py::test_power_of_two_thicknesses_give_the_plain_mean_and_the_thickness), so the rows are
    those of timeMean() of the source with that thickness set static -- and those of the source without any cell thickness"""
    nx, ny = grid
    e3 = numpy.ascontiguousarray(numpy.broadcast_to(TH2[None, :, None, None], (NT, NZ, ny, nx))).astype(real)
    f = _source(real, grid, True, e3u=e3, e3v=e3.copy(), db=DB2)
    assert numpy.array_equal(f.thickness, TH2)
    got = _products(_quiet(f.timeMean, thicknessWeighted=True))
    f.setCellThickness(_on(e3[0], True), _on(e3[0].copy(), True))
    static = _products(_quiet(f.timeMean))
    for k in got:
        assert numpy.abs(got[k]).max() > 0 and numpy.array_equal(got[k], static[k]), k
    f.setCellThickness(None, None)
    m = _quiet(f.timeMean)
    m.computeFlux(0)
    assert numpy.array_equal(_row(m), got['volume'])
    assert numpy.array_equal(_rows(m.computeFluxProfile(0)), got['volume_profile'])
    assert numpy.array_equal(_rows(m.computeTracerFlux(0)), got['tracer'])


@pytest.mark.parametrize('resident', [True, False], ids=['hbm', 'host'])
def test_static_thickness_gives_the_plain_time_mean_bit_for_bit(resident):
    real, grid = 'float32', GRIDS[1]
    e3u, e3v = (x[1] for x in _case(real, grid)[5:7])
    f = _source(real, grid, resident, e3u=e3u, e3v=e3v)
    assert f._e3['nt'] == 1
    for steps in (None, (0, 2)):
        a, b = _products(_quiet(f.timeMean, steps, thicknessWeighted=True)), _products(_quiet(f.timeMean, steps))
        for k in a:
            assert numpy.abs(a[k]).max() > 0 and numpy.array_equal(a[k], b[k]), (steps, k)


# ---- 6. the split and the command line -------------------------------------------------------------------------------------
@pytest.mark.parametrize('steps', [None, (1, 3)], ids=['all', '1to3'])
@pytest.mark.parametrize('resident', [True, False], ids=['hbm', 'host'])
def test_mean_eddy_split_is_assembled_from_the_series_and_the_mean_field(resident, steps):
    real, grid = 'float32', GRIDS[1]
    f = _source(real, grid, resident)
    d = _quiet(f.meanEddyTracerTransport, steps, thicknessWeighted=True)
    t0, t1 = (0, NT) if steps is None else steps
    series = f.computeTracerAll()[0]
    total = series[t0:t1].sum(axis=0) / (t1 - t0)
    mean = _quiet(f.timeMean, steps, thicknessWeighted=True).computeTracerFlux(0)[0]
    assert sorted(d) == ['eddy', 'mean', 'meanField', 'total']
    assert numpy.array_equal(d['total'], total) and numpy.array_equal(d['mean'], mean) and numpy.array_equal(d['eddy'], total - mean)
    assert d['total'].shape == (3,) and numpy.abs(d['eddy']).min() > 0
    assert numpy.array_equal(d['meanField'].computeTracerFlux(0)[0], mean) and d['meanField'].nt == 1
    assert d['meanField']._e3['nt'] == 1
    # the mean Field takes the other calls that take a cell thickness: its decomposition adds up to its transport
    parts = d['meanField'].decomposeTracerTransport(0)
    assert numpy.array_equal(parts['total'], mean)


def test_fluxplot_thickness_weighted_writes_the_three_parts(tmp_path):
    from nemoflux_amd import fluxplot
    from nemoflux_amd.field import Field
    real, grid = 'float32', GRIDS[0]
    paths = _write_npz(tmp_path, real, grid)
    lines = "[" + "],[".join(LINES) + "]"
    tr = fluxplot.readTargets(lines)[0]
    f = _quiet(Field, paths['T'], paths['U'], paths['V'], tr, True, readback=False, compact=True)
    f.setTracer((paths['T'], 'tau'), reference=REF)
    f.setCellThickness((paths['U'], 'e3u'), (paths['V'], 'e3v'))
    d = _quiet(f.meanEddyTracerTransport, thicknessWeighted=True)
    want = numpy.array([d[k] for k in ('total', 'mean', 'eddy')]) * 2.5
    out = str(tmp_path / 'eddy.csv')
    kw = dict(tFile=paths['T'], uFile=paths['U'], vFile=paths['V'], lonLatPoints=lines, sverdrup=True, tracer='tau',
              tracerRef=REF, tracerScale=2.5, eddy=True, cellThickness=True, output=out)
    got = _quiet(fluxplot.main, thicknessWeighted=True, **kw)
    assert numpy.array_equal(got, want) and numpy.abs(want).min() > 0
    with open(out) as fh:
        text = fh.read().splitlines()
    assert text[0].startswith('# mean transport of tau over 3 time steps') and 'tau x Sv x 2.5' in text[0]
    assert text[1] == 'part,line0,line1,line2' and [ln.split(',')[0] for ln in text[2:]] == ['total', 'mean', 'eddy']
    table = numpy.array([[float(x) for x in ln.split(',')[1:]] for ln in text[2:]])
    assert numpy.allclose(table, want, rtol=1e-14, atol=0)
    with pytest.raises(RuntimeError, match='the mean state of a time-varying cell thickness is not defined here'):
        _quiet(fluxplot.main, **kw)            # without the flag these files are refused as before


# ---- 7. the source ---------------------------------------------------------------------------------------------------------
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
    series = _rows(f.computeAll())
    f.computeFlux(1, readback=True)
    before = state()
    assert before[5] > 0 and numpy.abs(before[4]).max() > 0
    m = _quiet(f.timeMean, thicknessWeighted=True)
    _quiet(f.timeMean, (0, 2), thicknessWeighted=True)
    for x, y in zip(state(), before):
        assert numpy.array_equal(x, y)
    for t in range(NT):
        assert numpy.array_equal(_rows(f.computeTracerFlux(t)), rows[t])
    assert numpy.array_equal(_rows(f.computeAll()), series)
    f.computeFlux(1, readback=True)         # the running max has not moved either
    for x, y in zip(state(), before):
        assert numpy.array_equal(x, y)
    # its thickness is still the time-varying one, and the calls without the keyword still raise
    assert f._e3['nt'] == NT and m._e3['nt'] == 1
    for call in (f.timeMean, f.meanEddyTracerTransport, lambda: f.timeMean(thicknessWeighted=False)):
        with pytest.raises(RuntimeError, match='the mean state of a time-varying cell thickness is not defined here'):
            call()
    # what the mean Field refuses is what a Field with a static thickness refuses
    with pytest.raises(RuntimeError):
        m.computeTracerProfile(0)
