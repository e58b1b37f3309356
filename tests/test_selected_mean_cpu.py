"""Time means over selected, weighted steps (nf_time_mean_steps, nf_time_mean_weighted_steps, Field.timeMean(select=,
weights=), Field.meanEddySplit, fluxplot --time-weights / --time-select), the part that needs no GPU: the numpy restatement of
tests/selected_mean_reference.py pinned bit for bit to scalar Python loops; the three exact consequences of the definition
(unit weights give nf_time_mean / nf_time_mean_weighted, so do weights that all equal one power of two, any cut of the table
into calls gives one call); TimeObj step lengths and months; the fluxplot check; the symbols declared, exported and bound;
the argument errors the library decides before it needs a device; the Python refusals.

Everything computed is checked in tests/test_gpu_selected_mean.py."""
import ctypes
import os
import re
import subprocess

import numpy
import pytest

from conftest import ROOT
import selected_mean_reference as smr
import timemean_reference as tmr
import weighted_mean_reference as wmr

NF_ERR_ARG = 1
NF_F64, NF_F32 = 0, 1
FILL, MISSING = 1.e20, -999.
THFILL, THMISSING = -1.e30, 9999.


def _values(real, nsteps, n, seed, inf=True):
    """(nsteps, n) values and thicknesses: NaN and both markers in both, -0.0, +-inf in the values (a tracer), a value missing
    at every step, a thickness that is never there under a present value"""
    rng = numpy.random.default_rng(seed)
    dt = numpy.dtype(real).type
    a = rng.standard_normal((nsteps, n)).astype(real)
    h = rng.uniform(0.2, 3., (nsteps, n)).astype(real)
    marks = (numpy.nan, FILL, MISSING, -0.0) + ((numpy.inf, -numpy.inf) if inf else ())
    for arr, ms in ((a, marks), (h, (numpy.nan, THFILL, THMISSING, 0.0))):
        flat = arr.reshape(-1)
        for m in ms:
            flat[rng.choice(flat.size, max(1, flat.size // 14), replace=False)] = dt(m)
    a[:, 0] = [(dt(FILL), numpy.nan, dt(MISSING))[t % 3] for t in range(nsteps)]        # missing at every step
    h[:, 0] = dt(1.5)
    a[:, 1] = dt(0.75)
    h[:, 1] = [(dt(0.0), numpy.nan, dt(THFILL))[t % 3] for t in range(nsteps)]          # never any water
    a[:, 2] = dt(-0.0)
    h[:, 2] = dt(2.0)
    return a, h


def _weights(kind, nsteps, seed=0):
    if kind == 'months':
        return numpy.resize(smr.MONTHS, nsteps)
    if kind == 'random':
        return numpy.random.default_rng(100 + seed).uniform(0.5, 4., nsteps)
    return None


@pytest.mark.parametrize('kind', ['months', 'random', 'unit'])
@pytest.mark.parametrize('nsteps', [1, 2, 7])
@pytest.mark.parametrize('real', ['float64', 'float32'])
def test_restatement_is_the_scalar_loop_bit_for_bit(real, nsteps, kind):
    """markers, NaN and +-inf in the tracer; both rules; the weighted form without +-inf (0 x inf)"""
    n = 200
    a, h = _values(real, nsteps, n, seed=31 + nsteps)
    w = _weights(kind, nsteps, nsteps)
    total = smr.total_weight(w, nsteps) + 0.5           # not the sum: the divisor is the argument
    for markers in ((FILL, MISSING), (FILL, numpy.nan), (numpy.nan, numpy.nan)):
        fill_out = float(numpy.dtype(real).type(FILL)) if markers[0] == markers[0] else numpy.nan
        for rule in (smr.OVER_STEPS, smr.OVER_PRESENT):
            want, want_s, want_w, want_c = smr.scalar_selected_mean(a, w, markers, rule, total, fill_out)
            s, wp, c = smr.accumulate(a, w, markers)
            assert numpy.array_equal(c, want_c) and c.dtype == numpy.uint32
            assert smr.same_bits(s, want_s) and smr.same_bits(wp, want_w)
            assert smr.same_bits(smr.finish(s, wp, c, rule, total, fill_out), want)
            assert smr.same_bits(smr.selected_mean(a, w, markers, rule, total, fill_out), want)
        if markers == (FILL, MISSING):
            assert c[0] == 0 and want[0] == fill_out and c[2] == nsteps and want[2] == 0
            assert numpy.isinf(a).any() and numpy.isnan(a).any() and 0 < (c == nsteps).sum() < n
    a, h = _values(real, nsteps, n, seed=57 + nsteps, inf=False)
    for markers, hmarkers in (((FILL, MISSING), (THFILL, THMISSING)), ((numpy.nan, numpy.nan), (numpy.nan, THMISSING))):
        fill_out = float(numpy.dtype(real).type(FILL)) if markers[0] == markers[0] else numpy.nan
        want, want_h, want_sF, want_sH, want_c = smr.scalar_selected_weighted_mean(a, h, w, markers, hmarkers, total, fill_out)
        sF, sH, c = smr.accumulate_weighted(a, h, w, markers, hmarkers)
        assert numpy.array_equal(c, want_c) and smr.same_bits(sF, want_sF) and smr.same_bits(sH, want_sH)
        got, got_h = smr.finish_weighted(sF, sH, c, total, fill_out)
        assert smr.same_bits(got, want) and smr.same_bits(got_h, want_h)
        one = smr.selected_weighted_mean(a, h, w, markers, hmarkers, total, fill_out)
        assert smr.same_bits(one[0], want) and smr.same_bits(one[1], want_h)
        if markers == (FILL, MISSING):
            assert c[0] == 0 and got[0] == fill_out and c[1] == nsteps and got[1] == 0 and got_h[1] == 0


@pytest.mark.parametrize('real', ['float64', 'float32'])
def test_unit_and_power_of_two_weights_give_the_existing_means(real):
    """1 * x is exact, wp == c and total_weight == total_steps: the bits of nf_time_mean / nf_time_mean_weighted; weights that
    all equal 2^k scale every sum exactly and cancel in the quotients"""
    nsteps, n = 9, 400
    a, h = _values(real, nsteps, n, seed=5)
    b, hb = _values(real, nsteps, n, seed=6, inf=False)
    markers, hmarkers = (FILL, MISSING), (THFILL, THMISSING)
    for wt in (None, 1.0, 4.0, 0.25):
        w = None if wt is None else numpy.full(nsteps, wt)
        total = smr.total_weight(w, nsteps)
        assert total == nsteps * (wt or 1.0)
        for rule in (smr.OVER_STEPS, smr.OVER_PRESENT):
            got = smr.selected_mean(a, w, markers, rule, total, FILL)
            assert smr.same_bits(got, tmr.time_mean(a, markers, rule, nsteps, FILL)), (wt, rule)
        got, got_h = smr.selected_weighted_mean(b, hb, w, markers, hmarkers, total, FILL)
        want, want_h = wmr.weighted_time_mean(b, hb, markers, hmarkers, nsteps, FILL)
        assert smr.same_bits(got, want) and smr.same_bits(got_h, want_h), wt
    s, wp, c = smr.accumulate(a, None, markers)
    assert numpy.array_equal(wp, c.astype(numpy.float64))


@pytest.mark.parametrize('real', ['float64', 'float32'])
def test_any_cut_of_the_table_gives_the_bits_of_one_call(real):
    nsteps, n = 7, 300
    a, h = _values(real, nsteps, n, seed=9, inf=False)
    w = _weights('random', nsteps)
    markers, hmarkers = (FILL, MISSING), (THFILL, THMISSING)
    one = smr.accumulate(a, w, markers)
    onew = smr.accumulate_weighted(a, h, w, markers, hmarkers)
    cuts = [(k, nsteps - k) for k in range(1, nsteps)] + [(i, j - i, nsteps - j) for i in range(1, nsteps) for j in range(i + 1, nsteps)]
    for cut in cuts:
        part, partw, t = (None, None, None), (None, None, None), 0
        for k in cut:
            part = smr.accumulate(a[t:t + k], w[t:t + k], markers, *part)
            partw = smr.accumulate_weighted(a[t:t + k], h[t:t + k], w[t:t + k], markers, hmarkers, *partw)
            t += k
        for x, y in zip(part + partw, one + onew):
            assert smr.same_bits(x.astype(numpy.float64), y.astype(numpy.float64)), cut


# ---- TimeObj ---------------------------------------------------------------------------------------------------------------
def _time_variables(calendar, with_bounds, name='time_counter'):
    """twelve monthly steps from 1 January 2001, in days, centred in their months"""
    lengths = [30.] * 12 if calendar == '360_day' else list(smr.MONTHS)
    edges = numpy.concatenate([[0.], numpy.cumsum(lengths)])
    v = {name: 0.5 * (edges[:-1] + edges[1:]),
         '_attrs_' + name: dict(standard_name='time', units='days since 2001-01-01 00:00:00', calendar=calendar),
         'uo': numpy.zeros((12, 1, 2, 2)), '_attrs_uo': dict(units='m/s')}
    if with_bounds:
        v['_attrs_' + name]['bounds'] = name + '_bounds'
        v[name + '_bounds'] = numpy.stack([edges[:-1], edges[1:]], axis=1)
    return v, numpy.array(lengths)


@pytest.mark.parametrize('calendar', ['gregorian', 'noleap', '360_day'])
def test_time_object_step_lengths_and_months(calendar):
    from nemoflux_amd.timeobj import TimeObj
    v, lengths = _time_variables(calendar, True)
    t = TimeObj.fromVariables(v)
    got = t.getStepLengths()
    assert got.dtype == numpy.float64 and numpy.array_equal(got, lengths)
    assert t.getMonths() == list(range(1, 13)) and t.getSize() == 12 and t.timeVarName == 'time_counter'
    v, _ = _time_variables(calendar, False)
    t = TimeObj.fromVariables(v)
    assert t.getStepLengths() is None and t.getMonths() == list(range(1, 13))
    # a bounds attribute that names nothing, or something of another shape, is no bounds
    v, _ = _time_variables(calendar, True)
    v['time_counter_bounds'] = v['time_counter_bounds'][:5]
    assert TimeObj.fromVariables(v).getStepLengths() is None
    del v['time_counter_bounds']
    assert TimeObj.fromVariables(v).getStepLengths() is None
    # the constructor as it was; no time variable: neither
    t = TimeObj([0., 31.], 'days since 2001-01-01', 'noleap', 'time')
    assert t.getStepLengths() is None and t.getMonths() == [1, 2] and t.getTimeAsString(1) == '2001-2-1'
    assert TimeObj().getStepLengths() is None and TimeObj().getMonths() is None
    assert TimeObj.fromVariables({'uo': numpy.zeros(3)}).getMonths() is None
    assert TimeObj([0., 1.], 'fortnights since then').getMonths() == [None, None]


# ---- fluxplot --------------------------------------------------------------------------------------------------------------
def test_fluxplot_time_options_are_checked():
    from nemoflux_amd.fluxplot import checkTimeMeanArgs, main, parseTimeSelect, parseTimeWeights
    checkTimeMeanArgs()
    checkTimeMeanArgs('', '', eddy=True)
    checkTimeMeanArgs('bounds', 'months:12,1,2', eddy=True)
    checkTimeMeanArgs('31,28,31', '0,1,2', eddy=True)
    for kw, opt in ((dict(timeWeights='bounds'), '--time-weights'), (dict(timeSelect='0,2'), '--time-select'),
                    (dict(timeWeights='1,2', timeSelect='0,2'), '--time-weights')):
        with pytest.raises(RuntimeError, match=f'{opt} needs --eddy'):
            checkTimeMeanArgs(**kw)
    for bad in ('0,-1', 'x', '1,inf', '1,nan', '0', ''):
        if bad:
            with pytest.raises(RuntimeError, match='--time-weights'):
                checkTimeMeanArgs(bad, '', eddy=True)
    for bad in ('2,1', '1,1', '-1,2', 'months:0', 'months:13', 'months:x', '1.5'):
        with pytest.raises(RuntimeError, match='--time-select'):
            checkTimeMeanArgs('', bad, eddy=True)
    assert parseTimeWeights('bounds') == 'bounds' and parseTimeWeights('31,28.25') == [31., 28.25]
    assert parseTimeSelect('0,2,3,6') == [0, 2, 3, 6] and parseTimeSelect('months:12,1,2') == ('months', [12, 1, 2])
    # refused before any file is opened, whatever else is asked for: none of these files exists
    files = dict(tFile='/nonexistent/T.nc', uFile='/nonexistent/U.nc', vFile='/nonexistent/V.nc', lonLatPoints='(0,0),(1,1)')
    for kw in (dict(), dict(tracer='thetao'), dict(levels=True), dict(tracer='thetao', decompose=True), dict(gross=True),
               dict(depthBins='0,100,200'), dict(crossings='x.npz')):
        with pytest.raises(RuntimeError, match='--time-weights needs --eddy'):
            main(timeWeights='bounds', **kw, **files)
        with pytest.raises(RuntimeError, match='--time-select needs --eddy'):
            main(timeSelect='months:1', **kw, **files)
    with pytest.raises(RuntimeError, match='--eddy needs --tracer'):          # the other checks still apply
        main(timeWeights='bounds', eddy=True, **files)
    with pytest.raises(RuntimeError, match='no such file'):      # an accepted combination goes on to open the files
        main(timeWeights='bounds', timeSelect='0,2', eddy=True, tracer='thetao', **files)


def test_fluxplot_months_select_the_steps_of_those_months():
    from nemoflux_amd.fluxplot import parseTimeSelect, selectSteps
    from nemoflux_amd.timeobj import TimeObj

    class Stub(object):
        pass
    fld = Stub()
    v, _ = _time_variables('360_day', True)
    two_years = numpy.concatenate([v['time_counter'], v['time_counter'] + 360.])
    fld.timeObj = TimeObj(two_years, 'days since 2001-01-01', '360_day', 'time_counter')
    assert selectSteps(fld, parseTimeSelect('months:12,1,2')) == [0, 1, 11, 12, 13, 23]
    assert selectSteps(fld, parseTimeSelect('3,4')) == [3, 4] and selectSteps(fld, None) is None
    fld.timeObj = TimeObj()
    with pytest.raises(RuntimeError, match='--time-select months:... needs a time variable'):
        selectSteps(fld, parseTimeSelect('months:1'))


# ---- ABI -------------------------------------------------------------------------------------------------------------------
ARGS = {'nf_time_mean_steps': ('double *acc_dev, double *wsum_dev, unsigned *cnt_dev, const void *src_dev, '
                               'const long long *step_offsets, const double *weights, long nsteps, size_t n, int dtype, '
                               'double fill, double missing, int first, int last, int rule, double total_weight, '
                               'double fill_out, void *hip_stream'),
        'nf_time_mean_weighted_steps': ('double *accf_dev, double *acch_dev, unsigned *cnt_dev, const void *src_dev, '
                                        'const long long *src_offsets, const void *thk_dev, const long long *thk_offsets, '
                                        'const double *weights, long nsteps, size_t n, int dtype, double fill, double missing, '
                                        'double thk_fill, double thk_missing, int first, int last, double total_weight, '
                                        'double fill_out, void *hip_stream')}
# device addresses are bound as integers (c_void_p), the two host tables as typed pointers
C_TYPES = [('const long long *', ctypes.POINTER(ctypes.c_longlong)), ('const double *', ctypes.POINTER(ctypes.c_double)),
           ('double *', ctypes.c_void_p), ('unsigned *', ctypes.c_void_p), ('const void *', ctypes.c_void_p),
           ('void *', ctypes.c_void_p), ('long ', ctypes.c_long), ('size_t ', ctypes.c_size_t), ('int ', ctypes.c_int),
           ('double ', ctypes.c_double)]


@pytest.mark.parametrize('name', sorted(ARGS))
def test_symbols_are_exported_declared_and_bound_with_one_argument_list(name):
    from nemoflux_amd import _lib
    with open(os.path.join(ROOT, 'include', 'nemoflux_amd.h')) as fh:
        header = re.sub(r'/\*.*?\*/', '', fh.read(), flags=re.S)
    out = subprocess.run(['nm', '-D', '--defined-only', _lib._SO], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stderr
    assert name in {ln.split()[-1] for ln in out.stdout.splitlines() if ln.split()}
    m = re.search(r'\bint\s+' + name + r'\s*\(([^)]*)\)\s*;', header)
    assert m, f'{name} is not declared in include/nemoflux_amd.h'
    declared = ' '.join(m.group(1).split())
    assert declared == ARGS[name], declared
    want = [next(v for k, v in C_TYPES if a.strip().startswith(k)) for a in declared.split(',')]
    fn = getattr(_lib.lib, name)
    assert fn.restype is ctypes.c_int and list(fn.argtypes) == want, fn.argtypes
    with open(os.path.join(ROOT, 'nemoflux_amd', 'csrc', 'nf_timemean.hip')) as fh:
        m = re.search(r'extern "C" int ' + name + r'\s*\(([^)]*)\)', fh.read())
    assert m and ' '.join(m.group(1).split()) == ARGS[name]


def _table(values, ctype):
    return (ctype * len(values))(*values)


def test_argument_errors_are_decided_without_a_device():
    """every error listed in the header, each naming the function; the device pointers are never dereferenced"""
    from nemoflux_amd import _lib
    lib = _lib.lib
    A, W, C, S, T = 4096, 8192, 12288, 16384, 20480            # stand-ins for device addresses
    nan, inf = numpy.nan, numpy.inf

    def plain(acc=A, wsum=W, cnt=C, src=S, off=(0, 100, 200), w=(1., 2., 3.), nsteps=3, n=100, dtype=NF_F64, first=1, last=1,
              rule=0, total=6.):
        return lib.nf_time_mean_steps(acc, wsum, cnt, src, None if off is None else _table(off, ctypes.c_longlong),
                                      None if w is None else _table(w, ctypes.c_double), nsteps, n, dtype, nan, nan, first, last,
                                      rule, total, nan, None)

    def weighted(accf=A, acch=W, cnt=C, src=S, thk=T, off=(0, 100, 200), toff=(0, 100, 200), w=(1., 2., 3.), nsteps=3, n=100,
                 dtype=NF_F64, first=1, last=1, total=6.):
        return lib.nf_time_mean_weighted_steps(accf, acch, cnt, src, None if off is None else _table(off, ctypes.c_longlong), thk,
                                               None if toff is None else _table(toff, ctypes.c_longlong),
                                               None if w is None else _table(w, ctypes.c_double), nsteps, n, dtype, nan, nan, nan,
                                               nan, first, last, total, nan, None)

    bad_weights = [(dict(w=(1., x, 3.)), b'weight') for x in (0., -1., nan, inf, -inf)]
    common = [(dict(src=None), b'null'), (dict(off=None), b'null'), (dict(nsteps=0), b'nsteps'), (dict(nsteps=-2), b'nsteps'),
              (dict(n=0), b'n must not be 0'), (dict(dtype=2), b'dtype'), (dict(off=(0, -100, 200)), b'offset'),
              (dict(total=0.), b'total_weight'), (dict(total=-6.), b'total_weight'), (dict(total=nan), b'total_weight'),
              (dict(total=inf), b'total_weight'), (dict(cnt=None, first=0), b'cnt_dev'), (dict(cnt=None, last=0), b'cnt_dev')]
    for kw, word in common + bad_weights + [(dict(acc=None), b'null'), (dict(rule=2), b'rule'),
                                            (dict(wsum=None, rule=1, first=0), b'wsum_dev'),
                                            (dict(wsum=None, rule=1, last=0), b'wsum_dev')]:
        assert plain(**kw) == NF_ERR_ARG, kw
        err = lib.nf_last_error()
        assert word in err and err.startswith(b'nf_time_mean_steps:'), (kw, err)
    for kw, word in common + bad_weights + [(dict(accf=None), b'null'), (dict(acch=None), b'null'), (dict(thk=None), b'null'),
                                            (dict(toff=None), b'null'), (dict(toff=(0, 100, -1)), b'offset')]:
        assert weighted(**kw) == NF_ERR_ARG, kw
        err = lib.nf_last_error()
        assert word in err and err.startswith(b'nf_time_mean_weighted_steps:'), (kw, err)
    if _lib.device_count() == 0:
        # what is NOT an error goes on to need a device: no weights, repeated and descending offsets, total_weight unused by a
        # call that does not finish (or by the tracer rule), no wsum_dev under the velocity rule, nothing carried
        for kw in (dict(w=None), dict(off=(200, 0, 0)), dict(total=0., last=0), dict(total=0., rule=1), dict(wsum=None, first=0),
                   dict(wsum=None, cnt=None, rule=1), dict(dtype=NF_F32)):
            assert plain(**kw) == 4, kw
            assert b'no usable AMD GPU' in lib.nf_last_error()
        for kw in (dict(w=None), dict(off=(200, 0, 0), toff=(7, 7, 7)), dict(total=0., last=0), dict(cnt=None)):
            assert weighted(**kw) == 4, kw
            assert b'no usable AMD GPU' in lib.nf_last_error()


# ---- Python refusals -------------------------------------------------------------------------------------------------------
def test_python_refusals_that_need_no_device():
    from nemoflux_amd.field import Field, _TimeObj
    from nemoflux_amd.timeobj import TimeObj
    f = Field.__new__(Field)
    f.nt, f.nz, f.ny, f.nx = 12, 4, 5, 6
    f.slab_range = None
    f._e3 = None
    f.timeObj = _TimeObj(None)
    for kw, word in ((dict(steps=(0, 3), select=[0, 1]), 'steps or select, not both'), (dict(select=[2, 1]), 'strictly ascending'),
                     (dict(select=[1, 1]), 'strictly ascending'), (dict(select=[0, 12]), 'strictly ascending'),
                     (dict(select=[-1, 2]), 'strictly ascending'), (dict(select=[]), 'strictly ascending'),
                     (dict(select=[0.5, 2]), 'whole step indices'),
                     (dict(select=[0, 2], weights=[1.]), '1 weights for 2 steps'), (dict(weights=[1.] * 11), '11 weights for 12'),
                     (dict(select=[0, 2], weights=[1., 0.]), 'finite and > 0'), (dict(select=[0, 2], weights=[1., -2.]), 'finite'),
                     (dict(select=[0, 2], weights=[numpy.nan, 1.]), 'finite'), (dict(select=[0, 2], weights=[numpy.inf, 1.]), 'finite'),
                     (dict(weights='lengths'), "numbers or 'bounds'"), (dict(weights='bounds'), 'none found'),
                     (dict(steps=(3, 3), weights=[1.]), 'half-open')):
        with pytest.raises(RuntimeError, match=word):
            f.timeMean(**kw)
        with pytest.raises(RuntimeError, match=word):
            f.meanEddySplit('computeFluxProfile', **kw)
    v, lengths = _time_variables('noleap', False)
    f.timeObj = TimeObj.fromVariables(v)
    with pytest.raises(RuntimeError, match=r"weights='bounds' needs the bounds of the time variable \(time_counter\)"):
        f.timeMean(weights='bounds')
    f.timeObj = TimeObj.fromVariables(_time_variables('noleap', True)[0])
    idx, w, total = f._step_table('timeMean', None, [0, 1, 11], 'bounds')
    assert idx == [0, 1, 11] and numpy.array_equal(w, [31., 28., 31.]) and total == 90.
    assert f._step_table('timeMean', (2, 6), None, None) == ([2, 3, 4, 5], None, 4.0)
    idx, w, total = f._step_table('timeMean', None, range(3), [0.1, 0.2, 0.3])
    assert total == (0.1 + 0.2) + 0.3
    with pytest.raises(RuntimeError, match='method must be one of computeTracerFlux'):
        f.meanEddySplit('computeFlux')
    with pytest.raises(RuntimeError, match='setTracer first'):
        f.meanEddyTracerTransport(select=[0, 1])
