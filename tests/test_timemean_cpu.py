"""Time means (nf_time_mean, Field.timeMean, Field.meanEddyTracerTransport, fluxplot --eddy), the part that needs no GPU: the
numpy restatement of tests/timemean_reference.py pinned bit for bit to a scalar Python loop; the new symbol exported, declared
and bound with one argument list; every argument error the library decides before it needs a device; the fluxplot refusals.

Everything computed is checked in tests/test_gpu_timemean.py."""
import ctypes
import os
import re
import subprocess
import sys

import numpy
import pytest

from conftest import ROOT
import timemean_reference as tmr

NF_ERR_ARG = 1
NF_F64, NF_F32 = 0, 1
FILL, MISSING = 1.e20, -999.


def _values(real, nsteps, n, seed):
    """(nsteps, n) values with NaN, both markers, +-inf, -0.0 and a value missing at every step"""
    rng = numpy.random.default_rng(seed)
    dt = numpy.dtype(real).type
    a = rng.standard_normal((nsteps, n)).astype(real)
    flat = a.reshape(-1)
    for m in (numpy.nan, FILL, MISSING, numpy.inf, -numpy.inf, -0.0):
        flat[rng.choice(flat.size, max(1, flat.size // 12), replace=False)] = dt(m)
    a[:, 0] = (dt(FILL), numpy.nan, dt(MISSING), dt(FILL), numpy.nan, dt(MISSING), numpy.nan)[:nsteps]   # missing at every step
    a[:, 1] = dt(-0.0)                                           # a sum of negative zeros from +0.0
    a[:, 2] = numpy.inf
    a[1:, 2] = -numpy.inf                                        # +inf + -inf
    a[:, 3] = numpy.nan
    a[nsteps // 2, 3] = dt(3.5)                                  # present once
    return a


@pytest.mark.parametrize('rule', [tmr.OVER_STEPS, tmr.OVER_PRESENT], ids=['steps', 'present'])
@pytest.mark.parametrize('nsteps', [1, 2, 7])
@pytest.mark.parametrize('real', ['float64', 'float32'])
def test_restatement_is_the_scalar_loop_bit_for_bit(real, nsteps, rule):
    n = 300
    a = _values(real, nsteps, n, seed=11 + nsteps)
    for markers in ((FILL, MISSING), (FILL, numpy.nan), (numpy.nan, numpy.nan)):
        fill_out = float(numpy.dtype(real).type(FILL)) if markers[0] == markers[0] else numpy.nan
        want, want_c = tmr.scalar_time_mean(a, markers, rule, nsteps, fill_out)
        s, c = tmr.accumulate(a, markers)
        got = tmr.finish(s, c, rule, nsteps, fill_out)
        assert numpy.array_equal(c, want_c) and c.dtype == numpy.uint32
        assert tmr.same_bits(got, want)
        assert tmr.same_bits(tmr.time_mean(a, markers, rule, nsteps, fill_out), want)
        # carried in groups: the same bits
        s1, c1 = tmr.accumulate(a[:nsteps // 2], markers)
        s2, c2 = tmr.accumulate(a[nsteps // 2:], markers, s1, c1)
        assert numpy.array_equal(c2, c) and tmr.same_bits(s2, s)
        if markers == (FILL, MISSING):
            assert c[0] == 0 and (got[0] == fill_out or fill_out != fill_out)
            assert c[1] == nsteps and got[1] == 0 and not numpy.signbit(got[1])          # +0.0 + -0.0 = +0.0
            assert c[3] == 1 and got[3] == (3.5 / nsteps if rule == tmr.OVER_STEPS else 3.5)
            if nsteps > 1:
                assert numpy.isnan(got[2]) and c[2] == nsteps                            # +inf + -inf: present, NaN
            assert 0 < (c == nsteps).sum() < n
    assert not tmr.same_bits(numpy.array([0.0]), numpy.array([-0.0])) and tmr.same_bits(numpy.array([numpy.nan]), -numpy.array([numpy.nan]))


# ---- ABI -------------------------------------------------------------------------------------------------------------------
ARGS = ('double *acc_dev, unsigned *cnt_dev, const void *src_dev, long nsteps, long long stride_elems, size_t n, int dtype, '
        'double fill, double missing, int first, int last, int rule, long total_steps, double fill_out, void *hip_stream')
# device addresses are bound as integers (c_void_p), like every other HBM pointer of the binding
C_TYPES = [('double *', ctypes.c_void_p), ('unsigned *', ctypes.c_void_p), ('const void *', ctypes.c_void_p),
           ('void *', ctypes.c_void_p), ('long long ', ctypes.c_longlong), ('long ', ctypes.c_long), ('size_t ', ctypes.c_size_t),
           ('int ', ctypes.c_int), ('double ', ctypes.c_double)]


def test_symbol_is_exported_declared_and_bound_with_one_argument_list():
    from nemoflux_amd import _lib
    with open(os.path.join(ROOT, 'include', 'nemoflux_amd.h')) as fh:
        header = re.sub(r'/\*.*?\*/', '', fh.read(), flags=re.S)
    out = subprocess.run(['nm', '-D', '--defined-only', _lib._SO], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stderr
    assert 'nf_time_mean' in {ln.split()[-1] for ln in out.stdout.splitlines() if ln.split()}
    m = re.search(r'\bint\s+nf_time_mean\s*\(([^)]*)\)\s*;', header)
    assert m, 'nf_time_mean is not declared in include/nemoflux_amd.h'
    declared = ' '.join(m.group(1).split())
    assert declared == ARGS, declared
    want = [next(v for k, v in C_TYPES if a.strip().startswith(k)) for a in declared.split(',')]
    fn = _lib.lib.nf_time_mean
    assert fn.restype is ctypes.c_int and list(fn.argtypes) == want, fn.argtypes
    assert '#define NF_MEAN_OVER_STEPS 0' in header and '#define NF_MEAN_OVER_PRESENT 1' in header
    assert (_lib.NF_MEAN_OVER_STEPS, _lib.NF_MEAN_OVER_PRESENT) == (0, 1) == (tmr.OVER_STEPS, tmr.OVER_PRESENT)
    # the implementation takes the same list
    with open(os.path.join(ROOT, 'nemoflux_amd', 'csrc', 'nf_timemean.hip')) as fh:
        m = re.search(r'extern "C" int nf_time_mean\s*\(([^)]*)\)', fh.read())
    assert m and ' '.join(m.group(1).split()) == ARGS
    with open(os.path.join(ROOT, 'nemoflux_amd', 'csrc', 'Makefile')) as fh:
        assert re.search(r'^SRCS = .*\bnf_timemean\.hip\b', fh.read(), flags=re.M)


def test_argument_errors_are_decided_without_a_device():
    """every error listed in the header; the pointers are never dereferenced (they are not device memory)"""
    from nemoflux_amd import _lib
    lib = _lib.lib
    P, C, S = 4096, 8192, 16384            # stand-ins for device addresses
    nan = numpy.nan

    def call(acc=P, cnt=C, src=S, nsteps=3, stride=100, n=100, dtype=NF_F64, first=1, last=1, rule=0, total=3):
        return lib.nf_time_mean(acc, cnt, src, nsteps, stride, n, dtype, nan, nan, first, last, rule, total, nan, None)

    for kw, word in ((dict(acc=None), b'null'), (dict(src=None), b'null'), (dict(nsteps=0), b'nsteps'), (dict(nsteps=-2), b'nsteps'),
                     (dict(n=0), b'n must not be 0'), (dict(stride=99), b'stride_elems'), (dict(stride=-100), b'stride_elems'),
                     (dict(dtype=2), b'dtype'), (dict(dtype=-1), b'dtype'), (dict(rule=2), b'rule'), (dict(rule=-1), b'rule'),
                     (dict(total=0), b'total_steps'), (dict(total=-3), b'total_steps'),
                     (dict(cnt=None, first=0), b'cnt_dev'), (dict(cnt=None, last=0), b'cnt_dev'),
                     (dict(cnt=None, first=0, last=0), b'cnt_dev')):
        assert call(**kw) == NF_ERR_ARG, kw
        assert word in lib.nf_last_error(), (kw, lib.nf_last_error())
    if _lib.device_count() == 0:
        # what is NOT an error goes on to need a device: a stride below n with one step, total_steps unused by a call that
        # does not finish or by the tracer rule, no cnt_dev when nothing is carried
        for kw in (dict(nsteps=1, stride=0), dict(total=0, last=0), dict(total=0, rule=1), dict(cnt=None), dict(dtype=NF_F32)):
            assert call(**kw) == 4, kw
            assert b'no usable AMD GPU' in lib.nf_last_error()


# ---- fluxplot --------------------------------------------------------------------------------------------------------------
def test_fluxplot_eddy_option_is_checked():
    from nemoflux_amd.fluxplot import checkEddyArgs, main
    checkEddyArgs()
    checkEddyArgs(False, classes='1,2', levels=True, zrange='0,1', show=True, decompose=True)
    checkEddyArgs(True, 'thetao')
    with pytest.raises(RuntimeError, match='--eddy needs --tracer'):
        checkEddyArgs(True)
    for kw, opt in ((dict(classes='1,2'), '--classes'), (dict(levels=True), '--levels'), (dict(zrange='0,10'), '--zrange'),
                    (dict(show=True), '--show'), (dict(decompose=True), '--decompose')):
        with pytest.raises(RuntimeError, match=f'--eddy and {opt} cannot be combined'):
            checkEddyArgs(True, 'thetao', **kw)
    # refused before any file is opened: none of these files exists
    files = dict(tFile='/nonexistent/T.nc', uFile='/nonexistent/U.nc', vFile='/nonexistent/V.nc', lonLatPoints='(0,0),(1,1)')
    with pytest.raises(RuntimeError, match='--eddy needs --tracer'):
        main(eddy=True, **files)
    for kw in (dict(classes='1,2'), dict(levels=True), dict(zrange='0,10'), dict(show=True), dict(decompose=True)):
        with pytest.raises(RuntimeError, match='--eddy and .* cannot be combined'):
            main(eddy=True, tracer='thetao', **kw, **files)
    with pytest.raises(RuntimeError, match='no such file'):      # an accepted combination goes on to open the files
        main(eddy=True, tracer='thetao', tracerRef=1.5, tracerScale=4.1e-3, sverdrup=True, **files)


def test_fluxplot_command_line_lists_the_eddy_option():
    out = subprocess.run([sys.executable, '-m', 'nemoflux_amd.fluxplot', '--help'], cwd=ROOT, capture_output=True, text=True,
                         timeout=120)
    assert out.returncode == 0, out.stderr
    assert '--eddy' in out.stdout


def test_python_refusals_that_need_no_device():
    """timeMean refuses a sharded Field and a time-varying thickness, meanEddyTracerTransport a Field without a tracer, and a
    bad step range, before anything is computed"""
    from nemoflux_amd.field import Field
    f = Field.__new__(Field)
    f.nt, f.nz, f.ny, f.nx = 3, 4, 5, 6
    f.slab_range = (0, 6)
    with pytest.raises(RuntimeError, match='sharded Field'):
        f.timeMean()
    f.slab_range = None
    f._e3 = dict(nt=3)
    with pytest.raises(RuntimeError, match='the mean state of a time-varying cell thickness is not defined here'):
        f.timeMean()
    f._e3 = None
    for bad in ((0, 0), (2, 1), (-1, 2), (0, 4)):
        with pytest.raises(RuntimeError, match='half-open'):
            f.timeMean(bad)
    with pytest.raises(RuntimeError, match='setTracer first'):
        f.meanEddyTracerTransport()
