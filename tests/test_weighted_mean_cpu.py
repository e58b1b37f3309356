"""Thickness-weighted time means (nf_time_mean_weighted, Field.timeMean(thicknessWeighted=True),
Field.meanEddyTracerTransport(thicknessWeighted=True), fluxplot --thickness-weighted), the part that needs no GPU: the numpy
restatement of tests/weighted_mean_reference.py pinned bit for bit to a scalar Python loop; the new symbol exported, declared
and bound with one argument list; every argument error the library decides before it needs a device; the fluxplot and Python
refusals.

Everything computed is checked in tests/test_gpu_weighted_mean.py."""
import ctypes
import os
import re
import subprocess
import sys

import numpy
import pytest

from conftest import ROOT
import weighted_mean_reference as wmr

NF_ERR_ARG = 1
NF_F64, NF_F32 = 0, 1
FILL, MISSING = 1.e20, -999.
THFILL, THMISSING = -1.e30, 9999.


def _values(real, nsteps, n, seed):
    """(nsteps, n) velocities and thicknesses with NaN and both markers in both series, -0.0, a velocity missing at every
    step, a thickness zero (or missing) at every step under a present velocity, a thickness present once"""
    rng = numpy.random.default_rng(seed)
    dt = numpy.dtype(real).type
    a = rng.standard_normal((nsteps, n)).astype(real)
    h = rng.uniform(0.2, 3., (nsteps, n)).astype(real)
    for arr, marks in ((a, (numpy.nan, FILL, MISSING, -0.0)), (h, (numpy.nan, THFILL, THMISSING, 0.0))):
        flat = arr.reshape(-1)
        for m in marks:
            flat[rng.choice(flat.size, max(1, flat.size // 12), replace=False)] = dt(m)
    a[:, 0] = (dt(FILL), numpy.nan, dt(MISSING), dt(FILL), numpy.nan, dt(MISSING), numpy.nan)[:nsteps]   # missing at every step
    h[:, 0] = dt(1.5)
    a[:, 1] = dt(0.75)                                           # present at every step ...
    h[:, 1] = dt(0.0)                                            # ... under a thickness that is zero at every step
    a[:, 2] = dt(-1.25)
    h[:, 2] = (dt(THFILL), numpy.nan, dt(THMISSING), dt(0.0), numpy.nan, dt(THFILL), dt(THMISSING))[:nsteps]   # or never there
    a[:, 3] = dt(2.5)
    h[:, 3] = numpy.nan
    h[nsteps // 2, 3] = dt(0.5)                                  # water once
    a[:, 4] = dt(-0.0)
    h[:, 4] = dt(2.0)
    return a, h


@pytest.mark.parametrize('nsteps', [1, 2, 7])
@pytest.mark.parametrize('real', ['float64', 'float32'])
def test_restatement_is_the_scalar_loop_bit_for_bit(real, nsteps):
    n = 300
    a, h = _values(real, nsteps, n, seed=23 + nsteps)
    total = nsteps + 1              # not nsteps: the divisor is the argument
    for markers, hmarkers in (((FILL, MISSING), (THFILL, THMISSING)), ((FILL, numpy.nan), (numpy.nan, THMISSING)),
                              ((numpy.nan, numpy.nan), (numpy.nan, numpy.nan))):
        fill_out = float(numpy.dtype(real).type(FILL)) if markers[0] == markers[0] else numpy.nan
        want, want_h, want_sF, want_sH, want_c = wmr.scalar_weighted_time_mean(a, h, markers, hmarkers, total, fill_out)
        sF, sH, c = wmr.accumulate(a, h, markers, hmarkers)
        got, got_h = wmr.finish(sF, sH, c, total, fill_out)
        assert numpy.array_equal(c, want_c) and c.dtype == numpy.uint32
        assert wmr.same_bits(sF, want_sF) and wmr.same_bits(sH, want_sH)
        assert wmr.same_bits(got, want) and wmr.same_bits(got_h, want_h)
        one = wmr.weighted_time_mean(a, h, markers, hmarkers, total, fill_out)
        assert wmr.same_bits(one[0], want) and wmr.same_bits(one[1], want_h)
        # carried in groups: the same bits
        k = nsteps // 2
        part = wmr.accumulate(a[:k], h[:k], markers, hmarkers)
        sF2, sH2, c2 = wmr.accumulate(a[k:], h[k:], markers, hmarkers, *part)
        assert numpy.array_equal(c2, c) and wmr.same_bits(sF2, sF) and wmr.same_bits(sH2, sH)
        if markers == (FILL, MISSING):
            assert c[0] == 0 and got[0] == fill_out and got_h[0] == 1.5 * nsteps / total      # missing stays missing
            assert c[1] == nsteps and got[1] == 0 and not numpy.signbit(got[1]) and got_h[1] == 0   # never any water: 0, 0
            assert c[2] == nsteps and got[2] == 0 and not numpy.signbit(got[2]) and got_h[2] == 0
            assert got[3] == 2.5 and got_h[3] == 0.5 / total                                 # water once: that velocity
            assert got[4] == 0 and got_h[4] == 2.0 * nsteps / total
            assert 0 < (c == nsteps).sum() < n and numpy.isfinite(got).all() and numpy.isfinite(got_h).all()


def test_power_of_two_thicknesses_give_the_plain_mean_and_the_thickness():
    """anchor (c) of the GPU tests: with a thickness 2^k constant in time, sF / sH has the bits of the plain mean over the
    steps and sH / nt those of the thickness, whenever nt h is exact -- so also for nt = 3"""
    import timemean_reference as tmr
    rng = numpy.random.default_rng(3)
    for real in ('float64', 'float32'):
        for nt in (1, 2, 3, 4):
            a = rng.standard_normal((nt, 500)).astype(real)
            a.reshape(-1)[rng.choice(a.size, a.size // 10, replace=False)] = numpy.nan
            for h in (0.125, 0.25, 0.5, 1.0, 2.0):
                thk = numpy.full(a.shape, h, real)
                got, hbar = wmr.weighted_time_mean(a, thk, (), (), nt, numpy.nan)
                assert wmr.same_bits(got, tmr.time_mean(a, (), tmr.OVER_STEPS, nt, numpy.nan)), (real, nt, h)
                assert (hbar == h).all()


# ---- ABI -------------------------------------------------------------------------------------------------------------------
ARGS = ('double *accf_dev, double *acch_dev, unsigned *cnt_dev, const void *src_dev, long long src_stride_elems, '
        'const void *thk_dev, long long thk_stride_elems, long nsteps, size_t n, int dtype, double fill, double missing, '
        'double thk_fill, double thk_missing, int first, int last, long total_steps, double fill_out, void *hip_stream')
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
    assert 'nf_time_mean_weighted' in {ln.split()[-1] for ln in out.stdout.splitlines() if ln.split()}
    m = re.search(r'\bint\s+nf_time_mean_weighted\s*\(([^)]*)\)\s*;', header)
    assert m, 'nf_time_mean_weighted is not declared in include/nemoflux_amd.h'
    declared = ' '.join(m.group(1).split())
    assert declared == ARGS, declared
    want = [next(v for k, v in C_TYPES if a.strip().startswith(k)) for a in declared.split(',')]
    fn = _lib.lib.nf_time_mean_weighted
    assert fn.restype is ctypes.c_int and list(fn.argtypes) == want, fn.argtypes
    with open(os.path.join(ROOT, 'nemoflux_amd', 'csrc', 'nf_timemean.hip')) as fh:
        m = re.search(r'extern "C" int nf_time_mean_weighted\s*\(([^)]*)\)', fh.read())
    assert m and ' '.join(m.group(1).split()) == ARGS


def test_argument_errors_are_decided_without_a_device():
    """every error listed in the header, each naming the function; the pointers are never dereferenced (they are not device
    memory)"""
    from nemoflux_amd import _lib
    lib = _lib.lib
    F, H, C, S, T = 4096, 8192, 12288, 16384, 20480            # stand-ins for device addresses
    nan = numpy.nan

    def call(accf=F, acch=H, cnt=C, src=S, thk=T, nsteps=3, sstride=100, tstride=100, n=100, dtype=NF_F64, first=1, last=1,
             total=3):
        return lib.nf_time_mean_weighted(accf, acch, cnt, src, sstride, thk, tstride, nsteps, n, dtype, nan, nan, nan, nan, first,
                                         last, total, nan, None)

    for kw, word in ((dict(accf=None), b'null'), (dict(acch=None), b'null'), (dict(src=None), b'null'), (dict(thk=None), b'null'),
                     (dict(nsteps=0), b'nsteps'), (dict(nsteps=-2), b'nsteps'), (dict(n=0), b'n must not be 0'),
                     (dict(sstride=99), b'src_stride_elems'), (dict(sstride=-100), b'src_stride_elems'),
                     (dict(tstride=99), b'thk_stride_elems'), (dict(tstride=-100), b'thk_stride_elems'),
                     (dict(dtype=2), b'dtype'), (dict(dtype=-1), b'dtype'),
                     (dict(total=0), b'total_steps'), (dict(total=-3), b'total_steps'),
                     (dict(cnt=None, first=0), b'cnt_dev'), (dict(cnt=None, last=0), b'cnt_dev'),
                     (dict(cnt=None, first=0, last=0), b'cnt_dev')):
        assert call(**kw) == NF_ERR_ARG, kw
        err = lib.nf_last_error()
        assert word in err and err.startswith(b'nf_time_mean_weighted:'), (kw, err)
    if _lib.device_count() == 0:
        # what is NOT an error goes on to need a device: strides below n with one step, total_steps unused by a call that does
        # not finish, no cnt_dev when nothing is carried, strides that differ
        for kw in (dict(nsteps=1, sstride=0, tstride=0), dict(total=0, last=0), dict(cnt=None), dict(dtype=NF_F32),
                   dict(sstride=100, tstride=164)):
            assert call(**kw) == 4, kw
            assert b'no usable AMD GPU' in lib.nf_last_error()


# ---- fluxplot --------------------------------------------------------------------------------------------------------------
def test_fluxplot_thickness_weighted_option_is_checked():
    from nemoflux_amd.fluxplot import checkThicknessWeightedArgs, main
    checkThicknessWeightedArgs()
    checkThicknessWeightedArgs(False, eddy=True, cellThickness=True)
    checkThicknessWeightedArgs(True, eddy=True, cellThickness=True)
    for kw in (dict(), dict(eddy=True), dict(cellThickness=True)):
        with pytest.raises(RuntimeError, match='--thickness-weighted needs --eddy and --cell-thickness'):
            checkThicknessWeightedArgs(True, **kw)
    # refused before any file is opened: none of these files exists
    files = dict(tFile='/nonexistent/T.nc', uFile='/nonexistent/U.nc', vFile='/nonexistent/V.nc', lonLatPoints='(0,0),(1,1)')
    for kw in (dict(), dict(eddy=True, tracer='thetao'), dict(cellThickness=True), dict(cellThickness=True, tracer='thetao'),
               dict(cellThickness=True, gross=True)):
        with pytest.raises(RuntimeError, match='--thickness-weighted needs --eddy and --cell-thickness'):
            main(thicknessWeighted=True, **kw, **files)
    with pytest.raises(RuntimeError, match='--eddy needs --tracer'):          # the other checks still apply
        main(thicknessWeighted=True, eddy=True, cellThickness=True, **files)
    with pytest.raises(RuntimeError, match='no such file'):      # an accepted combination goes on to open the files
        main(thicknessWeighted=True, eddy=True, cellThickness=True, tracer='thetao', **files)


def test_fluxplot_command_line_lists_the_option():
    out = subprocess.run([sys.executable, '-m', 'nemoflux_amd.fluxplot', '--help'], cwd=ROOT, capture_output=True, text=True,
                         timeout=120)
    assert out.returncode == 0, out.stderr
    assert '--thickness-weighted' in out.stdout


def test_python_refusals_that_need_no_device():
    """thicknessWeighted=True refuses a sharded Field as before and a Field without a cell thickness; without the keyword a
    time-varying thickness raises as before, with the same message; a bad step range is refused under both"""
    from nemoflux_amd.field import Field
    f = Field.__new__(Field)
    f.nt, f.nz, f.ny, f.nx = 3, 4, 5, 6
    f.slab_range = (0, 6)
    f._e3 = dict(nt=3)
    with pytest.raises(RuntimeError, match='sharded Field'):
        f.timeMean(thicknessWeighted=True)
    f.slab_range = None
    f._e3 = None
    for call in (lambda: f.timeMean(thicknessWeighted=True), lambda: f.timeMean(None, True)):
        with pytest.raises(RuntimeError, match='setCellThickness'):
            call()
    f._e3 = dict(nt=3)
    for call in (f.timeMean, lambda: f.timeMean(thicknessWeighted=False)):
        with pytest.raises(RuntimeError, match='the mean state of a time-varying cell thickness is not defined here '
                                               r'\(it would need thickness-weighted means\)'):
            call()
    for bad in ((0, 0), (2, 1), (-1, 2), (0, 4)):
        with pytest.raises(RuntimeError, match='half-open'):
            f.timeMean(bad, thicknessWeighted=True)
    with pytest.raises(RuntimeError, match='setTracer first'):
        f.meanEddyTracerTransport(thicknessWeighted=True)
