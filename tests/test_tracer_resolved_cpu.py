"""Depth- and class-resolved tracer transports, the parts that need no GPU: the header declares the six entry points and the
library exports them (and nothing the header does not declare); the calls check their handle, arguments and call order
before touching a device; fluxplot's --levels and --carry options."""
import ctypes
import os
import re
import subprocess
import sys

import numpy
import pytest

NF_ERR_ARG, NF_ERR_STATE = 1, 2
NF_F64, NF_F32 = 0, 1
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CALLS = ('nf_field_compute_tracer_profile', 'nf_field_compute_tracer_profile_async', 'nf_field_set_class_tracer',
         'nf_field_set_class_tracer_missing_value', 'nf_field_compute_class_tracer_transport',
         'nf_field_compute_class_tracer_transport_async')
COMPUTE = ('nf_field_compute_tracer_profile', 'nf_field_compute_tracer_profile_async',
           'nf_field_compute_class_tracer_transport', 'nf_field_compute_class_tracer_transport_async')


def _header():
    with open(os.path.join(ROOT, 'include', 'nemoflux_amd.h')) as fh:
        return fh.read()


def test_header_declares_and_library_exports_the_six_calls():
    from nemoflux_amd import _lib
    header = _header()
    for name in CALLS:
        assert re.search(r'\bint\s+' + name + r'\s*\(\s*nf_field\s*\*\*\s*self', header), name
        assert hasattr(_lib.lib, name), name
        assert getattr(_lib.lib, name).argtypes, name      # bound with a signature in _lib.py
    assert _lib.lib.nf_version() == 100


def test_exported_field_calls_are_the_declared_ones():
    """nm -D: every exported nf_field_* symbol is declared in the header and every declared one is exported"""
    from nemoflux_amd import _lib
    out = subprocess.run(['nm', '-D', '--defined-only', _lib._SO], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stderr
    exported = {ln.split()[-1] for ln in out.stdout.splitlines() if ln.split() and ln.split()[-1].startswith('nf_field_')}
    declared = set(re.findall(r'\bint\s+(nf_field_\w+)\s*\(', _header()))
    assert set(CALLS) <= declared
    assert exported == declared, (sorted(exported - declared), sorted(declared - exported))


def _new():
    from nemoflux_amd import _lib
    h = ctypes.c_void_p()
    assert _lib.lib.nf_field_new(ctypes.byref(h)) == 0
    return h


def _compute(name, h, out):
    from nemoflux_amd import _lib
    fn = getattr(_lib.lib, name)
    if out is None:
        return fn(h, 0, None)
    return fn(h, 0, ctypes.c_void_p(out.ctypes.data) if name.endswith('_async') else _lib.dptr(out))


def test_null_handles_and_arguments_are_refused():
    from nemoflux_amd import _lib
    lib = _lib.lib
    rows = numpy.zeros(64)
    for name in COMPUTE:
        assert _compute(name, None, rows) == NF_ERR_ARG, name
        assert b'null' in lib.nf_last_error()
    assert lib.nf_field_set_class_tracer(None, rows.ctypes.data, 1, NF_F64, 0, numpy.nan) == NF_ERR_ARG
    assert b'null' in lib.nf_last_error()
    assert lib.nf_field_set_class_tracer_missing_value(None, 1.0) == NF_ERR_ARG
    assert b'null' in lib.nf_last_error()
    h = _new()
    try:
        for name in COMPUTE:
            assert _compute(name, ctypes.byref(h), None) == NF_ERR_ARG, name
            assert b'null' in lib.nf_last_error() and name.encode() in lib.nf_last_error()
    finally:
        assert lib.nf_field_del(ctypes.byref(h)) == 0


def test_compute_before_set_tracer_or_set_class_edges_is_a_state_error():
    from nemoflux_amd import _lib
    lib = _lib.lib
    rows = numpy.zeros(64)
    uv = numpy.zeros(16)
    edges = numpy.array([0., 1., 2.])

    def all_four(h):
        got = {}
        for name in COMPUTE:
            rc = _compute(name, ctypes.byref(h), rows)
            got[name] = (rc, lib.nf_last_error())
        return got

    h = _new()
    try:
        for name, (rc, msg) in all_four(h).items():           # nothing set
            assert rc == NF_ERR_STATE and b'set_tracer first' in msg, name
        assert lib.nf_field_set_class_edges(ctypes.byref(h), _lib.dptr(edges), 3) == 0
        for name, (rc, msg) in all_four(h).items():           # edges, no tracer
            assert rc == NF_ERR_STATE and b'set_tracer first' in msg, name
        # a class tracer does not stand in for the carried one, and needs uo / vo first
        assert lib.nf_field_set_class_tracer(ctypes.byref(h), uv.ctypes.data, 3, NF_F64, 0, numpy.nan) == NF_ERR_STATE
        assert b'set_uv first' in lib.nf_last_error()
    finally:
        assert lib.nf_field_del(ctypes.byref(h)) == 0
    h = _new()
    try:
        assert lib.nf_field_set_uv(ctypes.byref(h), uv.ctypes.data, uv.ctypes.data, 3, NF_F64, 0, numpy.nan) == 0
        assert lib.nf_field_set_class_tracer(ctypes.byref(h), uv.ctypes.data, 3, NF_F64, 0, numpy.nan) == 0
        for name, (rc, msg) in all_four(h).items():           # class tracer only
            assert rc == NF_ERR_STATE and b'set_tracer first' in msg, name
        assert lib.nf_field_set_tracer(ctypes.byref(h), uv.ctypes.data, 3, NF_F64, 0, numpy.nan) == 0
        for name, (rc, msg) in all_four(h).items():           # tracer, no edges, no grid
            assert rc == NF_ERR_STATE, name
            assert (b'set_class_edges first' if 'class' in name else b'set_bounds') in msg, (name, msg)
        assert lib.nf_field_set_class_edges(ctypes.byref(h), _lib.dptr(edges), 3) == 0
        for name, (rc, msg) in all_four(h).items():           # everything but the grid
            assert rc == NF_ERR_STATE and b'set_bounds' in msg, name
    finally:
        assert lib.nf_field_del(ctypes.byref(h)) == 0


def test_class_tracer_dtype_and_nt_must_be_those_of_uv():
    from nemoflux_amd import _lib
    lib = _lib.lib
    uv = numpy.zeros(16)
    h = _new()
    try:
        assert lib.nf_field_set_uv(ctypes.byref(h), uv.ctypes.data, uv.ctypes.data, 3, NF_F64, 0, numpy.nan) == 0
        assert lib.nf_field_set_class_tracer(ctypes.byref(h), uv.ctypes.data, 3, NF_F32, 0, numpy.nan) == NF_ERR_ARG
        msg = lib.nf_last_error()
        assert b'float32' in msg and b'float64' in msg and b'dtype' in msg
        assert lib.nf_field_set_class_tracer(ctypes.byref(h), uv.ctypes.data, 2, NF_F64, 0, numpy.nan) == NF_ERR_ARG
        msg = lib.nf_last_error()
        assert b'nt = 2' in msg and b'uo/vo have 3' in msg
        assert lib.nf_field_set_class_tracer(ctypes.byref(h), uv.ctypes.data, 3, 7, 0, numpy.nan) == NF_ERR_ARG
        assert b'dtype must be' in lib.nf_last_error()
        assert lib.nf_field_set_class_tracer(ctypes.byref(h), uv.ctypes.data, 3, NF_F64, 0, numpy.nan) == 0
        assert lib.nf_field_set_class_tracer_missing_value(ctypes.byref(h), -999.) == 0
        # NULL clears the slot, whatever the other arguments say, also before uo / vo are known
        assert lib.nf_field_set_class_tracer(ctypes.byref(h), None, 0, 7, 0, numpy.nan) == 0
    finally:
        assert lib.nf_field_del(ctypes.byref(h)) == 0
    h = _new()
    try:
        assert lib.nf_field_set_class_tracer(ctypes.byref(h), None, 0, NF_F64, 0, numpy.nan) == 0
    finally:
        assert lib.nf_field_del(ctypes.byref(h)) == 0


def test_fluxplot_levels_and_carry_options_are_checked():
    from nemoflux_amd.fluxplot import checkLevelsArgs, checkCarryArgs, checkClassArgs, checkTracerArgs, main
    checkLevelsArgs()
    checkLevelsArgs(True)
    checkCarryArgs()
    checkCarryArgs('thetao', 'T.nc', 1.5, 4.1e-3, '26,27', 'sigma0')
    with pytest.raises(RuntimeError, match='--zrange'):
        checkLevelsArgs(True, zrange='0,100')
    with pytest.raises(RuntimeError, match='--classes'):
        checkLevelsArgs(True, classes='26,27')
    with pytest.raises(RuntimeError, match='--show'):
        checkLevelsArgs(True, show=True)
    with pytest.raises(RuntimeError, match='--carry-file needs --carry'):
        checkCarryArgs(carryFile='T.nc')
    with pytest.raises(RuntimeError, match='need --carry'):
        checkCarryArgs(carryRef=1.0)
    with pytest.raises(RuntimeError, match='need --carry'):
        checkCarryArgs(carryScale=2.0)
    with pytest.raises(RuntimeError, match='--carry needs --classes'):
        checkCarryArgs('thetao')
    with pytest.raises(RuntimeError, match='--carry needs --classes'):
        checkCarryArgs('thetao', classes='26,27')                  # no class field
    with pytest.raises(RuntimeError, match='--levels'):
        checkCarryArgs('thetao', classes='26,27', tracer='sigma0', levels=True)
    for bad in (dict(carryRef=numpy.nan), dict(carryScale=numpy.inf)):
        with pytest.raises(RuntimeError, match='finite'):
            checkCarryArgs('thetao', classes='26,27', tracer='sigma0', **bad)
    # the refusals of the older options stay
    with pytest.raises(RuntimeError, match='--zrange'):
        checkTracerArgs('thetao', zrange='0,1000')
    with pytest.raises(RuntimeError, match='--zrange'):
        checkClassArgs('26,27', 'sigma0', zrange='0,1000')
    with pytest.raises(RuntimeError, match='--tracer-ref'):
        checkClassArgs('26,27', 'sigma0', tracerRef=1.0)
    with pytest.raises(RuntimeError, match='--tracer-scale'):
        checkClassArgs('26,27', 'sigma0', tracerScale=2.0)
    # refused before any file is opened
    files = dict(tFile='no_such_T.nc', uFile='no_such_U.nc', vFile='no_such_V.nc', lonLatPoints='[(0,0),(1,1)]')
    for kw in (dict(levels=True, zrange='0,10'), dict(levels=True, show=True), dict(levels=True, tracer='thetao', zrange='0,10'),
               dict(levels=True, tracer='sigma0', classes='26,27'), dict(carry='thetao'), dict(carry='thetao', tracer='sigma0'),
               dict(carryFile='T.nc'), dict(carryScale=2.0), dict(carry='thetao', tracer='sigma0', classes='26,27', zrange='0,10'),
               dict(carry='thetao', tracer='sigma0', classes='26,27', tracerRef=2.0),
               dict(carry='thetao', tracer='sigma0', classes='26,27', carryRef=numpy.nan)):
        with pytest.raises(RuntimeError, match='--'):
            main(**files, **kw)


def test_fluxplot_command_line_lists_the_new_options():
    out = subprocess.run([sys.executable, '-m', 'nemoflux_amd.fluxplot', '--help'], cwd=ROOT, capture_output=True, text=True,
                         timeout=120)
    assert out.returncode == 0, out.stderr
    for opt in ('--levels', '--carry NAME', '--carry-file FILE', '--carry-ref X', '--carry-scale S', '--classes E0,E1,...,EN',
                '--zrange ZTOP,ZBOT', '--tracer NAME'):
        assert opt in out.stdout, opt
    bad = subprocess.run([sys.executable, '-m', 'nemoflux_amd.fluxplot', '-t', 'no_T.nc', '-u', 'no_U.nc', '-v', 'no_V.nc',
                          '-l', '[(0,0),(1,1)]', '--carry', 'thetao'], cwd=ROOT, capture_output=True, text=True, timeout=120)
    assert bad.returncode != 0 and '--carry needs --classes' in bad.stderr
    bad = subprocess.run([sys.executable, '-m', 'nemoflux_amd.fluxplot', '-t', 'no_T.nc', '-u', 'no_U.nc', '-v', 'no_V.nc',
                          '-l', '[(0,0),(1,1)]', '--levels', '--zrange', '0,10'], cwd=ROOT, capture_output=True, text=True,
                         timeout=120)
    assert bad.returncode != 0 and '--levels and --zrange' in bad.stderr
