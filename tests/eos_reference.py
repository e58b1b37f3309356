"""The numpy restatement of nf_sigma_eos80 (include/nemoflux_amd.h, nemoflux_amd/csrc/nf_eos.hip): the UNESCO EOS-80 equation
of state, vectorised over the values, every polynomial in the kernel's Horner form and operation order in float64, with the
engine's presence rule and the one rounding to the array's dtype at the end.  Every operation is one IEEE float64 operation, so
the kernel's bits are these bits.  scalar_sigma is the same thing as a Python loop over floats (tests/test_eos_cpu.py pins the
two to each other)."""
import math

import numpy


def rho0(S, T, r):
    """one-atmosphere density, r = sqrt(S)"""
    rw = 999.842594 + (6.793952e-2 + (-9.095290e-3 + (1.001685e-4 + (-1.120083e-6 + 6.536332e-9 * T) * T) * T) * T) * T
    b = 8.24493e-1 + (-4.0899e-3 + (7.6438e-5 + (-8.2467e-7 + 5.3875e-9 * T) * T) * T) * T
    c = -5.72466e-3 + (1.0227e-4 - 1.6546e-6 * T) * T
    return rw + (b + c * r + 4.8314e-4 * S) * S


def bulk(S, T, P, r):
    """secant bulk modulus, P in bar"""
    kw = 19652.21 + (148.4206 + (-2.327105 + (1.360477e-2 - 5.155288e-5 * T) * T) * T) * T
    k0 = kw + (54.6746 + (-0.603459 + (1.09987e-2 - 6.1670e-5 * T) * T) * T) * S + (7.944e-2 + (1.6483e-2 - 5.3009e-4 * T) * T) * S * r
    aw = 3.239908 + (1.43713e-3 + (1.16092e-4 - 5.77905e-7 * T) * T) * T
    a = aw + (2.2838e-3 + (-1.0981e-5 - 1.6078e-6 * T) * T) * S + 1.91075e-4 * S * r
    bw = 8.50935e-5 + (-6.12293e-6 + 5.2787e-8 * T) * T
    bb = bw + (-9.9348e-7 + (2.0816e-8 + 9.1697e-10 * T) * T) * S
    return k0 + (a + bb * P) * P


def atg(S, T, p):
    """adiabatic lapse rate in degC / dbar, p in dbar"""
    ds = S - 35.0
    return (3.5803e-5 + (8.5258e-6 + (-6.836e-8 + 6.6228e-10 * T) * T) * T + (1.8932e-6 - 4.2393e-8 * T) * ds
            + ((1.8741e-8 + (-6.7795e-10 + (8.733e-12 - 5.4481e-14 * T) * T) * T) + (-1.1351e-10 + 2.7759e-12 * T) * ds) * p
            + (-4.6206e-13 + (1.8676e-14 - 2.1687e-16 * T) * T) * p * p)


def ptmp(S, T, p, pr):
    """T moved adiabatically from p to pr"""
    h = pr - p
    xk = h * atg(S, T, p)
    T = T + 0.5 * xk
    q = xk
    p = p + 0.5 * h
    xk = h * atg(S, T, p)
    T = T + 0.29289322 * (xk - q)
    q = 0.58578644 * xk + 0.121320344 * q
    xk = h * atg(S, T, p)
    T = T + 1.707106781 * (xk - q)
    q = 3.414213562 * xk - 4.121320344 * q
    p = p + 0.5 * h
    xk = h * atg(S, T, p)
    return T + (xk - 2.0 * q) / 6.0


def rho(S, T, p_dbar, r):
    """in-situ density at p_dbar"""
    P = p_dbar / 10.0
    return rho0(S, T, r) / (1.0 - P / bulk(S, T, P, r))


def sigma_f64(theta, S, pref):
    """sigma_pref of float64 arrays (or floats, with r = math.sqrt) before the presence rule and the final rounding"""
    pref = float(pref)
    with numpy.errstate(invalid='ignore', over='ignore'):
        r = numpy.sqrt(S)
        if pref == 0.0:
            return rho0(S, theta, r) - 1000.0
        return rho(S, ptmp(S, theta, 0.0, pref), pref, r) - 1000.0


def present(a, markers):
    """the engine's rule: not NaN and equal to neither marker, each cast to the array's dtype and compared in that dtype"""
    a = numpy.asarray(a)
    here = ~numpy.isnan(a)
    with numpy.errstate(over='ignore'):
        for m in markers:
            if m == m:
                here &= a != a.dtype.type(m)
    return here


def sigma(theta, salt, pref=0.0, theta_markers=(), salt_markers=(), fill_out=numpy.nan):
    """nf_sigma_eos80 on arrays of one shape and dtype (float64 or float32): an array of that dtype"""
    theta, salt = numpy.asarray(theta), numpy.asarray(salt)
    assert theta.dtype == salt.dtype and theta.shape == salt.shape and theta.dtype in (numpy.float64, numpy.float32)
    here = present(theta, theta_markers) & present(salt, salt_markers)
    s = sigma_f64(theta.astype(numpy.float64), salt.astype(numpy.float64), pref)
    with numpy.errstate(over='ignore', invalid='ignore'):
        return numpy.where(here, s.astype(theta.dtype), theta.dtype.type(fill_out))


def scalar_sigma(theta, salt, pref=0.0, theta_markers=(), salt_markers=(), fill_out=numpy.nan):
    """the same, one value at a time with math.sqrt and Python float arithmetic"""
    theta, salt = numpy.asarray(theta), numpy.asarray(salt)
    dt = theta.dtype.type
    pref = float(pref)
    with numpy.errstate(over='ignore'):
        tm = [dt(m) for m in theta_markers if m == m]
        sm = [dt(m) for m in salt_markers if m == m]
        out = numpy.empty(theta.shape, theta.dtype)
        fo = dt(fill_out)
    for i in numpy.ndindex(theta.shape):
        t, s = theta[i], salt[i]
        if t != t or s != s or any(t == m for m in tm) or any(s == m for m in sm):
            out[i] = fo
            continue
        T, S = float(t), float(s)
        if S < 0.0:
            out[i] = numpy.nan
            continue
        r = math.sqrt(S)
        if pref == 0.0:
            v = rho0(S, T, r) - 1000.0
        else:
            Tp = ptmp(S, T, 0.0, pref)
            P = pref / 10.0
            v = rho0(S, Tp, r) / (1.0 - P / bulk(S, Tp, P, r)) - 1000.0
        with numpy.errstate(over='ignore'):
            out[i] = dt(v)
    return out


def same_bits(a, b):
    """equal value by value, NaNs by position, zeros by sign"""
    a, b = numpy.asarray(a), numpy.asarray(b)
    if a.shape != b.shape or a.dtype != b.dtype:
        return False
    na, nb = numpy.isnan(a), numpy.isnan(b)
    return bool(numpy.array_equal(na, nb) and numpy.array_equal(a[~na], b[~nb])
                and numpy.array_equal(numpy.signbit(a[~na]), numpy.signbit(b[~nb])))
