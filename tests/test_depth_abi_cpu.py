"""The C ABI of the transports in true-depth bins without a GPU: nf_field_set_depth_edges, nf_field_compute_depth_transport and
nf_field_compute_depth_transport_async are declared, exported and bound, and return NF_ERR_ARG for null arguments, bad edges, a
`top` that is not finite and a bad `carry`, NF_ERR_STATE before set_depth_edges and with `carry` before set_tracer -- all
decided before a device is needed.  The depth edges are a set of their own: the class calls do not see them."""
import ctypes
import os
import re
import subprocess

import numpy

from conftest import ROOT

NF_ERR_ARG, NF_ERR_STATE = 1, 2
NF_F64 = 0
CALLS = ('nf_field_compute_depth_transport', 'nf_field_compute_depth_transport_async')
SET = 'nf_field_set_depth_edges'


def _header():
    with open(os.path.join(ROOT, 'include', 'nemoflux_amd.h')) as fh:
        return re.sub(r'/\*.*?\*/', '', fh.read(), flags=re.S)


def test_header_declares_and_library_exports_the_three_calls():
    from nemoflux_amd import _lib
    header = _header()
    out = subprocess.run(['nm', '-D', '--defined-only', _lib._SO], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stderr
    exported = {ln.split()[-1] for ln in out.stdout.splitlines() if ln.split()}
    args = {CALLS[0]: 'nf_field **self, long tIndex, int carry, double *rows_host',
            CALLS[1]: 'nf_field **self, long tIndex, int carry, double *rows_dev',
            SET: 'nf_field **self, const double *edges, int nedges, double top'}
    for name, want in args.items():
        m = re.search(r'\bint\s+' + name + r'\s*\(([^)]*)\)\s*;', header)
        assert m, f'{name} is not declared in include/nemoflux_amd.h'
        assert ' '.join(m.group(1).split()) == want, name
        assert name in exported, name
        fn = getattr(_lib.lib, name)
        assert fn.restype is ctypes.c_int and len(fn.argtypes) == 4, name
    for name in CALLS:
        fn = getattr(_lib.lib, name)
        assert fn.argtypes[1] is ctypes.c_long and fn.argtypes[2] is ctypes.c_int, name
    fn = getattr(_lib.lib, SET)
    assert fn.argtypes[2] is ctypes.c_int and fn.argtypes[3] is ctypes.c_double
    assert _lib.lib.nf_version() == 100


def _compute(name, h, carry, out):
    from nemoflux_amd import _lib
    fn = getattr(_lib.lib, name)
    if out is None:
        return fn(h, 0, carry, None)
    return fn(h, 0, carry, ctypes.c_void_p(out.ctypes.data) if name.endswith('_async') else _lib.dptr(out))


def test_set_depth_edges_checks_its_arguments():
    from nemoflux_amd import _lib
    lib = _lib.lib
    good = numpy.array([0., 100., 500.])
    assert lib.nf_field_set_depth_edges(None, _lib.dptr(good), 3, 0.0) == NF_ERR_ARG
    assert b'nf_field_set_depth_edges: null argument' in lib.nf_last_error()
    h = ctypes.c_void_p()
    assert lib.nf_field_new(ctypes.byref(h)) == 0
    try:
        assert lib.nf_field_set_depth_edges(ctypes.byref(h), None, 3, 0.0) == NF_ERR_ARG
        assert b'nf_field_set_depth_edges: null argument' in lib.nf_last_error()
        for n in (1, 0, -3, 1026):
            e = numpy.arange(max(n, 2), dtype=numpy.float64)
            assert lib.nf_field_set_depth_edges(ctypes.byref(h), _lib.dptr(e), n, 0.0) == NF_ERR_ARG, n
            assert b'nf_field_set_depth_edges: need 2 <= nedges <= 1025' in lib.nf_last_error()
        for bad, words in ((numpy.array([0., numpy.nan, 2.]), b'every edge must be a finite number'),
                           (numpy.array([0., numpy.inf]), b'every edge must be a finite number'),
                           (numpy.array([0., 2., 2.]), b'the edges must be strictly increasing'),
                           (numpy.array([3., 2., 1.]), b'the edges must be strictly increasing')):
            assert lib.nf_field_set_depth_edges(ctypes.byref(h), _lib.dptr(bad), bad.size, 0.0) == NF_ERR_ARG
            assert b'nf_field_set_depth_edges: ' + words in lib.nf_last_error()
        for top in (numpy.nan, numpy.inf, -numpy.inf):
            assert lib.nf_field_set_depth_edges(ctypes.byref(h), _lib.dptr(good), 3, top) == NF_ERR_ARG
            assert b'nf_field_set_depth_edges: top must be a finite number' in lib.nf_last_error()
        # none of the refused calls set anything
        rows = numpy.zeros(64)
        assert _compute(CALLS[0], ctypes.byref(h), 0, rows) == NF_ERR_STATE
        assert b'set_depth_edges first' in lib.nf_last_error()
        for e, top in ((good, 0.0), (numpy.arange(1025) / 32., -1.5), (numpy.array([-5., 5.]), 1e6)):
            assert lib.nf_field_set_depth_edges(ctypes.byref(h), _lib.dptr(e), e.size, top) == 0
    finally:
        assert lib.nf_field_del(ctypes.byref(h)) == 0


def test_argument_and_state_errors_of_the_two_computes():
    """null, carry, then set_depth_edges first, then (carry) set_tracer first, then the grid -- all before a device is needed"""
    from nemoflux_amd import _lib
    lib = _lib.lib
    rows = numpy.zeros(256)
    uv = numpy.zeros(16)
    edges = numpy.array([1., 2., 3.])
    for name in CALLS:
        assert _compute(name, None, 0, rows) == NF_ERR_ARG, name
        assert b'null' in lib.nf_last_error() and name.encode() in lib.nf_last_error()
    h = ctypes.c_void_p()
    assert lib.nf_field_new(ctypes.byref(h)) == 0
    try:
        for name in CALLS:
            assert _compute(name, ctypes.byref(h), 0, None) == NF_ERR_ARG, name
            assert b'null' in lib.nf_last_error() and name.encode() in lib.nf_last_error()
            for carry in (2, -1):
                assert _compute(name, ctypes.byref(h), carry, rows) == NF_ERR_ARG, name
                assert b'carry must be 0 or 1' in lib.nf_last_error() and name.encode() in lib.nf_last_error()
            for carry in (0, 1):
                assert _compute(name, ctypes.byref(h), carry, rows) == NF_ERR_STATE, name
                assert (name + ': set_depth_edges first').encode() in lib.nf_last_error()
        # the class edges are another set: the depth calls do not see them, the class calls do not see the depth edges
        assert lib.nf_field_set_class_edges(ctypes.byref(h), _lib.dptr(edges), 3) == 0
        for name in CALLS:
            assert _compute(name, ctypes.byref(h), 0, rows) == NF_ERR_STATE, name
            assert (name + ': set_depth_edges first').encode() in lib.nf_last_error()
        assert lib.nf_field_set_depth_edges(ctypes.byref(h), _lib.dptr(edges), 3, 0.0) == 0
        for name in CALLS:
            assert _compute(name, ctypes.byref(h), 1, rows) == NF_ERR_STATE, name
            assert (name + ': set_tracer first').encode() in lib.nf_last_error()
            assert _compute(name, ctypes.byref(h), 0, rows) == NF_ERR_STATE, name            # the volume form needs no tracer
            assert b'set_bounds' in lib.nf_last_error() and name.encode() in lib.nf_last_error()
        assert lib.nf_field_set_uv(ctypes.byref(h), uv.ctypes.data, uv.ctypes.data, 3, NF_F64, 0, numpy.nan) == 0
        assert lib.nf_field_set_tracer(ctypes.byref(h), uv.ctypes.data, 3, NF_F64, 0, numpy.nan) == 0
        for name in CALLS:
            for carry in (0, 1):
                assert _compute(name, ctypes.byref(h), carry, rows) == NF_ERR_STATE, name
                assert b'set_bounds' in lib.nf_last_error() and name.encode() in lib.nf_last_error()
        assert not rows.any()
    finally:
        assert lib.nf_field_del(ctypes.byref(h)) == 0
