"""Tracer transports, the parts that need no GPU: the header declares the six entry points and the library exports them; the
calls check their handle, dtype, shape and call order before touching a device; fluxplot's tracer options."""
import ctypes
import os
import re

import numpy
import pytest

NF_ERR_ARG, NF_ERR_STATE = 1, 2
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CALLS = ('nf_field_set_tracer', 'nf_field_set_tracer_missing_value', 'nf_field_set_tracer_reference',
         'nf_field_set_tracer_wrap', 'nf_field_compute_tracer_flux', 'nf_field_compute_tracer_all_async')


def test_header_declares_and_library_exports_the_tracer_calls():
    from nemoflux_amd import _lib
    with open(os.path.join(ROOT, 'include', 'nemoflux_amd.h')) as fh:
        header = fh.read()
    for name in CALLS:
        assert re.search(r'\bint\s+' + name + r'\s*\(\s*nf_field\s*\*\*\s*self', header), name
        assert hasattr(_lib.lib, name), name


def _handle_with_uv(nt=3, dtype=0):
    """a field handle with host uo / vo set (set_uv needs no device)"""
    from nemoflux_amd import _lib
    lib = _lib.lib
    h = ctypes.c_void_p()
    assert lib.nf_field_new(ctypes.byref(h)) == 0
    uv = numpy.zeros(16)
    assert lib.nf_field_set_uv(ctypes.byref(h), uv.ctypes.data, uv.ctypes.data, nt, dtype, 0, numpy.nan) == 0
    return h, uv


def test_null_handles_and_arguments_are_refused():
    from nemoflux_amd import _lib
    lib = _lib.lib
    tau = numpy.zeros(16)
    row = numpy.zeros(16)
    assert lib.nf_field_set_tracer(None, tau.ctypes.data, 3, 0, 0, numpy.nan) == NF_ERR_ARG
    assert b'null' in lib.nf_last_error()
    assert lib.nf_field_set_tracer_missing_value(None, 0.) == NF_ERR_ARG
    assert lib.nf_field_set_tracer_reference(None, 0.) == NF_ERR_ARG
    assert lib.nf_field_set_tracer_wrap(None, 1) == NF_ERR_ARG
    assert lib.nf_field_compute_tracer_flux(None, 0, _lib.dptr(row)) == NF_ERR_ARG
    assert lib.nf_field_compute_tracer_all_async(None, ctypes.c_void_p(row.ctypes.data)) == NF_ERR_ARG
    h, uv = _handle_with_uv()
    try:
        assert lib.nf_field_set_tracer(ctypes.byref(h), None, 3, 0, 0, numpy.nan) == NF_ERR_ARG
        assert lib.nf_field_compute_tracer_all_async(ctypes.byref(h), None) == NF_ERR_ARG
        assert lib.nf_field_set_tracer(ctypes.byref(h), tau.ctypes.data, 3, 7, 0, numpy.nan) == NF_ERR_ARG
        assert b'dtype' in lib.nf_last_error()
        assert lib.nf_field_set_tracer_wrap(ctypes.byref(h), 2) == NF_ERR_ARG
        assert lib.nf_field_set_tracer_reference(ctypes.byref(h), numpy.inf) == NF_ERR_ARG
        assert lib.nf_field_set_tracer_reference(ctypes.byref(h), numpy.nan) == NF_ERR_ARG
        assert lib.nf_field_set_tracer_reference(ctypes.byref(h), 20.) == 0
        assert lib.nf_field_set_tracer_wrap(ctypes.byref(h), 0) == 0
        assert lib.nf_field_set_tracer_missing_value(ctypes.byref(h), numpy.nan) == 0
    finally:
        assert lib.nf_field_del(ctypes.byref(h)) == 0


def test_dtype_and_shape_must_match_uo_vo():
    from nemoflux_amd import _lib
    lib = _lib.lib
    tau = numpy.zeros(16)
    h, uv = _handle_with_uv(nt=3, dtype=0)
    try:
        assert lib.nf_field_set_tracer(ctypes.byref(h), tau.ctypes.data, 3, 1, 0, numpy.nan) == NF_ERR_ARG
        assert b"tracer's dtype differs" in lib.nf_last_error()
        assert lib.nf_field_set_tracer(ctypes.byref(h), tau.ctypes.data, 2, 0, 0, numpy.nan) == NF_ERR_ARG
        assert b'nt = 2' in lib.nf_last_error() and b'have 3' in lib.nf_last_error()
        assert lib.nf_field_set_tracer(ctypes.byref(h), tau.ctypes.data, 3, 0, 1, -32768.) == 0
    finally:
        assert lib.nf_field_del(ctypes.byref(h)) == 0


def test_call_order_is_checked_without_a_gpu():
    from nemoflux_amd import _lib
    lib = _lib.lib
    tau = numpy.zeros(16)
    row = numpy.zeros(16)
    h = ctypes.c_void_p()
    assert lib.nf_field_new(ctypes.byref(h)) == 0
    try:
        # no uo / vo yet: nothing to match the tracer against
        assert lib.nf_field_set_tracer(ctypes.byref(h), tau.ctypes.data, 3, 0, 0, numpy.nan) == NF_ERR_STATE
        assert b'set_uv first' in lib.nf_last_error()
        # compute before set_tracer
        assert lib.nf_field_compute_tracer_flux(ctypes.byref(h), 0, _lib.dptr(row)) == NF_ERR_STATE
        assert b'set_tracer first' in lib.nf_last_error()
        assert lib.nf_field_compute_tracer_all_async(ctypes.byref(h), ctypes.c_void_p(row.ctypes.data)) == NF_ERR_STATE
        assert b'set_tracer first' in lib.nf_last_error()
    finally:
        assert lib.nf_field_del(ctypes.byref(h)) == 0
    h, uv = _handle_with_uv()
    try:
        assert lib.nf_field_compute_tracer_flux(ctypes.byref(h), 0, _lib.dptr(row)) == NF_ERR_STATE
        assert b'set_tracer first' in lib.nf_last_error()
    finally:
        assert lib.nf_field_del(ctypes.byref(h)) == 0


def test_fluxplot_tracer_options_are_checked():
    from nemoflux_amd.fluxplot import checkTracerArgs, main
    checkTracerArgs()
    checkTracerArgs('thetao')
    checkTracerArgs('thetao', 'T2.nc', 20., 4.1e-3)
    with pytest.raises(RuntimeError, match='--tracer and --zrange'):
        checkTracerArgs('thetao', zrange='0,1000')
    with pytest.raises(RuntimeError, match='--tracer-file needs --tracer'):
        checkTracerArgs('', 'T2.nc')
    with pytest.raises(RuntimeError, match='need --tracer'):
        checkTracerArgs('', tracerRef=20.)
    with pytest.raises(RuntimeError, match='need --tracer'):
        checkTracerArgs('', tracerScale=2.)
    with pytest.raises(RuntimeError, match='finite'):
        checkTracerArgs('thetao', tracerScale=float('nan'))
    # refused before any file is opened
    with pytest.raises(RuntimeError, match='--zrange'):
        main(tFile='no_such_T.nc', uFile='no_such_U.nc', vFile='no_such_V.nc', lonLatPoints='[(0,0),(1,1)]',
             tracer='thetao', zrange='0,10')


def test_fluxplot_command_line_has_the_tracer_options():
    import subprocess
    import sys
    out = subprocess.run([sys.executable, '-m', 'nemoflux_amd.fluxplot', '--help'], cwd=ROOT, capture_output=True, text=True,
                         timeout=120)
    assert out.returncode == 0, out.stderr
    for opt in ('--tracer NAME', '--tracer-file FILE', '--tracer-ref X', '--tracer-scale S'):
        assert opt in out.stdout, opt
