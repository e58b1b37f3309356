"""Potential density from theta and S (nf_sigma_eos80, nemoflux_amd.eos, fluxplot --sigma), the part that needs no GPU: the
numpy restatement of tests/eos_reference.py against the published UNESCO 1983 check values and pinned bit for bit to a scalar
Python loop; its presence rule; the new symbol exported, declared and bound with one argument list; every argument error the
library decides before it needs a device; the Python and fluxplot refusals.

Everything computed on the device is checked in tests/test_gpu_eos.py."""
import ctypes
import math
import os
import re
import subprocess
import sys

import numpy
import pytest

from conftest import ROOT
import eos_reference as eos

NF_ERR_ARG = 1
NF_F64, NF_F32 = 0, 1


# ---- the formulas ------------------------------------------------------------------------------------------------------------
def test_restatement_gives_the_published_check_values():
    """UNESCO technical papers in marine science 44 (1983): each to half a unit of its last printed digit"""
    def rho(S, T, p):
        return eos.rho(S, T, p, math.sqrt(S))

    got = [(rho(35., 5., 0.), 1027.67547, 5e-6), (rho(0., 5., 0.), 999.96675, 5e-6), (rho(35., 25., 0.), 1023.34306, 5e-6),
           (rho(0., 25., 0.), 997.04796, 5e-6), (rho(35., 5., 10000.), 1069.48914, 5e-6), (rho(35., 25., 10000.), 1062.53817, 5e-6),
           (rho(0., 5., 10000.), 1044.12802, 5e-6), (rho(0., 25., 10000.), 1037.90204, 5e-6),
           (eos.bulk(35., 25., 1000., math.sqrt(35.)), 27108.95, 5e-3), (eos.atg(40., 40., 10000.), 3.255976e-4, 5e-11),
           (eos.ptmp(40., 40., 10000., 0.), 36.89073, 5e-6)]
    for k, (value, want, half) in enumerate(got):
        print(k, repr(value), want)
        assert abs(value - want) <= half, (k, value, want)
    # at the surface the pressure form is the one-atmosphere equation, and sigma is rho - 1000
    assert rho(35., 5., 0.) == eos.rho0(35., 5., math.sqrt(35.))
    assert eos.sigma_f64(numpy.array([5.]), numpy.array([35.]), 0.)[0] == eos.rho0(35., 5., math.sqrt(35.)) - 1000.0
    # sigma4 of deep water: theta moved down 4000 dbar warms, the density is that of the in-situ pair
    T4 = eos.ptmp(34.7, 1.0, 0.0, 4000.)
    assert 1.3 < T4 < 1.4
    assert eos.sigma_f64(numpy.array([1.0]), numpy.array([34.7]), 4000.)[0] == rho(34.7, T4, 4000.) - 1000.0


def _random(real, n, seed):
    rng = numpy.random.default_rng(seed)
    theta = rng.uniform(-2., 32., n).astype(real)
    salt = rng.uniform(0., 42., n).astype(real)
    theta[:3], salt[3:6] = 0., 0.                      # exact zeros (sqrt(0), the polynomials at T = 0)
    return theta, salt


@pytest.mark.parametrize('pref', [0., 2000., 4000.])
@pytest.mark.parametrize('real', ['float64', 'float32'])
def test_restatement_is_the_scalar_loop_bit_for_bit(real, pref):
    theta, salt = _random(real, 400, seed=int(pref) + 3)
    got = eos.sigma(theta, salt, pref)
    want = eos.scalar_sigma(theta, salt, pref)
    assert got.dtype == numpy.dtype(real) and numpy.isfinite(got).all() and got.min() > -5. and got.max() < 60.
    assert eos.same_bits(got, want)
    if pref:
        assert (got > eos.sigma(theta, salt, 0.)).all()          # compressed water is denser
    if real == 'float32':        # the arithmetic is float64: the float32 result is the rounded float64 result of the widened inputs
        wide = eos.sigma(theta.astype(numpy.float64), salt.astype(numpy.float64), pref)
        assert numpy.array_equal(got, wide.astype(numpy.float32))


@pytest.mark.parametrize('pref', [0., 2000.])
@pytest.mark.parametrize('real', ['float64', 'float32'])
def test_presence_rule(real, pref):
    TF, TM, SF, SM = 1.e20, -999., -32768., 1.e300        # 1e300 is not a float32: it is compared as the dtype holds it (inf)
    dt = numpy.dtype(real).type
    theta, salt = _random(real, 64, seed=9)
    with numpy.errstate(over='ignore'):
        theta[10], theta[11], theta[12] = dt(TF), dt(TM), numpy.nan            # theta only
        salt[20], salt[21], salt[22] = dt(SF), dt(SM), numpy.nan               # S only
        theta[30], salt[30] = dt(TF), dt(SM)                                   # both
        theta[40], salt[41] = dt(SF), dt(TM)                                   # the other array's marker is a value
        salt[50] = dt(-0.5)                                                    # S < 0
        salt[51] = numpy.inf                                                   # float32: what SM is held as
    for fill_out in (numpy.nan, -7.5, 1.e20):
        kw = dict(theta_markers=(TF, TM), salt_markers=(SF, SM), fill_out=fill_out)
        got = eos.sigma(theta, salt, pref, **kw)
        assert eos.same_bits(got, eos.scalar_sigma(theta, salt, pref, **kw))
        missing = [10, 11, 12, 20, 21, 22, 30] + ([51] if real == 'float32' else [])
        fo = dt(fill_out)
        for i in missing:
            assert got[i] == fo or (fo != fo and got[i] != got[i]), i
        plain = eos.sigma(theta, salt, pref)
        keep = numpy.ones(64, bool)
        keep[missing] = False
        assert eos.same_bits(got[keep], plain[keep])
        assert numpy.isnan(got[50]) and numpy.isnan(plain[50])                 # sqrt(-0.5)
    # one marker, or none
    one = eos.sigma(theta, salt, pref, theta_markers=(TF, numpy.nan), salt_markers=(numpy.nan, numpy.nan), fill_out=-1.)
    assert one[10] == -1. and one[12] == -1. and one[22] == -1. and one[11] != -1. and one[20] != -1.


# ---- ABI ---------------------------------------------------------------------------------------------------------------------
ARGS = ('void *out_dev, const void *theta_dev, const void *salt_dev, size_t n, int dtype, double pref_dbar, double theta_fill, '
        'double theta_missing, double salt_fill, double salt_missing, double fill_out, void *hip_stream')
C_TYPES = [('void *', ctypes.c_void_p), ('const void *', ctypes.c_void_p), ('size_t ', ctypes.c_size_t), ('int ', ctypes.c_int),
           ('double ', ctypes.c_double)]


def test_symbol_is_exported_declared_and_bound_with_one_argument_list():
    from nemoflux_amd import _lib
    with open(os.path.join(ROOT, 'include', 'nemoflux_amd.h')) as fh:
        header = re.sub(r'/\*.*?\*/', '', fh.read(), flags=re.S)
    out = subprocess.run(['nm', '-D', '--defined-only', _lib._SO], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stderr
    assert 'nf_sigma_eos80' in {ln.split()[-1] for ln in out.stdout.splitlines() if ln.split()}
    m = re.search(r'\bint\s+nf_sigma_eos80\s*\(([^)]*)\)\s*;', header)
    assert m, 'nf_sigma_eos80 is not declared in include/nemoflux_amd.h'
    declared = ' '.join(m.group(1).split())
    assert declared == ARGS, declared
    want = [next(v for k, v in C_TYPES if a.strip().startswith(k)) for a in declared.split(',')]
    fn = _lib.lib.nf_sigma_eos80
    assert fn.restype is ctypes.c_int and list(fn.argtypes) == want, fn.argtypes
    with open(os.path.join(ROOT, 'nemoflux_amd', 'csrc', 'nf_eos.hip')) as fh:
        m = re.search(r'extern "C" int nf_sigma_eos80\s*\(([^)]*)\)', fh.read())
    assert m and ' '.join(m.group(1).split()) == ARGS
    with open(os.path.join(ROOT, 'nemoflux_amd', 'csrc', 'Makefile')) as fh:
        assert re.search(r'^SRCS = .*\bnf_eos\.hip\b', fh.read(), flags=re.M)


def test_argument_errors_are_decided_without_a_device():
    """every error listed in the header; the pointers are never dereferenced (they are not device memory)"""
    from nemoflux_amd import _lib
    lib = _lib.lib
    O, T, S = 1 << 20, 2 << 20, 3 << 20            # stand-ins for device addresses, 1 MiB apart
    nan = numpy.nan

    def call(out=O, theta=T, salt=S, n=1000, dtype=NF_F64, pref=0.0):
        return lib.nf_sigma_eos80(out, theta, salt, n, dtype, pref, nan, nan, nan, nan, nan, None)

    for kw, word in ((dict(out=None), b'null'), (dict(theta=None), b'null'), (dict(salt=None), b'null'),
                     (dict(dtype=2), b'dtype'), (dict(dtype=-1), b'dtype'), (dict(pref=-1.0), b'pref_dbar'),
                     (dict(pref=nan), b'pref_dbar'), (dict(pref=numpy.inf), b'pref_dbar'), (dict(pref=-0.5, n=0), b'pref_dbar'),
                     (dict(dtype=7, n=0), b'dtype'),
                     (dict(out=T + 8), b'overlaps'), (dict(out=T - 8), b'overlaps'), (dict(out=S + 7992), b'overlaps'),
                     (dict(out=S - 3996, dtype=NF_F32), b'overlaps'), (dict(out=T + 3996, dtype=NF_F32), b'overlaps')):
        assert call(**kw) == NF_ERR_ARG, kw
        err = lib.nf_last_error()
        assert word in err and err.startswith(b'nf_sigma_eos80:'), (kw, err)
    # n == 0 is a no-op whatever the pointers are, with or without a device
    assert call(n=0) == 0 and call(n=0, out=None, theta=None, salt=None) == 0 and call(n=0, pref=2000., dtype=NF_F32) == 0
    if _lib.device_count() == 0:
        # what is NOT an error goes on to need a device: in place over either input, ranges that only touch, any pref >= 0
        for kw in (dict(out=T), dict(out=S), dict(out=T + 8000), dict(out=T - 8000), dict(out=T + 4000, dtype=NF_F32),
                   dict(pref=2000.), dict(pref=1.e-300), dict(theta=S)):
            assert call(**kw) == 4, kw
            assert b'no usable AMD GPU' in lib.nf_last_error()


# ---- Python ------------------------------------------------------------------------------------------------------------------
def test_sigma_describes_a_derived_tracer_and_refuses_what_it_cannot_be():
    from nemoflux_amd.eos import Sigma, sigma_eos80
    th, so = numpy.zeros((2, 3, 4, 5), numpy.float32), numpy.ones((2, 3, 4, 5), numpy.float32)
    s = Sigma(th, so, pref=2000, fill_value=1.e20, so_missing_value=-1.)
    assert s.pref == 2000.0 and s.shape == (2, 3, 4, 5) and s.dtype == numpy.float32
    assert s.markers == ((1.e20, None), (None, -1.))
    assert Sigma(th, so).pref == 0.0
    for bad in (-1., numpy.nan, numpy.inf):
        with pytest.raises(RuntimeError, match='pref'):
            Sigma(th, so, pref=bad)
    with pytest.raises(RuntimeError, match='different shapes'):
        Sigma(th, so[:, :2])
    with pytest.raises(RuntimeError, match='thetao is float32 and so float64'):
        Sigma(th, so.astype(numpy.float64))
    with pytest.raises(RuntimeError, match='CUDA tensors or DeviceArrays'):
        sigma_eos80(th, so)


def test_a_field_with_a_sigma_refuses_the_time_means():
    from nemoflux_amd.field import Field
    f = Field.__new__(Field)
    f.nt, f.nz, f.ny, f.nx = 3, 4, 5, 6
    f.slab_range = None
    f._e3 = None
    for slot in ('_tracer', '_class_tracer'):
        f._tracer = f._class_tracer = None
        setattr(f, slot, dict(sigma=object()))
        for call in (f.timeMean, f.meanEddyTracerTransport):
            with pytest.raises(RuntimeError, match='a Sigma .* the mean of sigma and sigma of the means'):
                call()


def test_fluxplot_sigma_option_is_checked():
    from nemoflux_amd.fluxplot import main, parseSigma
    assert parseSigma('thetao,so') == ('thetao', 'so', 0.0)
    assert parseSigma(' thetao , so , 2000 ') == ('thetao', 'so', 2000.0)
    for bad in ('thetao', 'thetao,so,1,2', 'thetao,,0', 'thetao,so,deep', 'thetao,so,-5', 'thetao,so,nan'):
        with pytest.raises(RuntimeError, match='--sigma'):
            parseSigma(bad)
    files = dict(tFile='/nonexistent/T.nc', uFile='/nonexistent/U.nc', vFile='/nonexistent/V.nc', lonLatPoints='(0,0),(1,1)')
    with pytest.raises(RuntimeError, match='--sigma and --tracer cannot be combined'):
        main(sigma='thetao,so', tracer='sigma0', classes='26,27', **files)
    with pytest.raises(RuntimeError, match='--sigma needs --classes, --gross-classes or --classes2'):
        main(sigma='thetao,so', **files)
    with pytest.raises(RuntimeError, match='--sigma'):
        main(sigma='thetao', classes='26,27', **files)
    with pytest.raises(RuntimeError, match='no such file'):      # an accepted combination goes on to open the files
        main(sigma='thetao,so,2000', classes='36,37', sverdrup=True, **files)


def test_fluxplot_command_line_lists_the_sigma_option():
    out = subprocess.run([sys.executable, '-m', 'nemoflux_amd.fluxplot', '--help'], cwd=ROOT, capture_output=True, text=True,
                         timeout=120)
    assert out.returncode == 0, out.stderr
    assert '--sigma' in out.stdout
