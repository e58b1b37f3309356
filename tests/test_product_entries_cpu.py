"""The entry path of the fourteen per-step products of the Field handle without a GPU: both forms of every product (the
synchronous one and `_async`) are declared, exported and bound, refuse null arguments and a bad `carry` under their own name,
and answer a handle that is not ready with one exact code and message -- pinned here for a fresh handle and for one with
set_uv, set_tracer, set_class_edges and set_depth_edges called, for both forms and every carry.  Three products (area profile,
gross profile, crossings) ask for a device before the grid: where there is none they return NF_ERR_NO_DEVICE at that point,
on a GPU machine the message of the grid check.  Nothing a refused call is given is written."""
import ctypes
import os
import re
import subprocess

import numpy
import pytest

from conftest import ROOT

NF_ERR_ARG, NF_ERR_STATE, NF_ERR_NO_DEVICE = 1, 2, 4
NF_F64 = 0
GRID = ': set_bounds, set_thickness and set_uv first'
NO_GPU = 'no usable AMD GPU (hipGetDeviceCount); nemoflux_amd has no CPU fallback'
S = '{s}'           # the symbol called, `_async` included

# stem, takes carry, the name of the rows in the header (host form; the `_async` form has `_dev`), then what the call answers
# on a fresh handle and on the handle with uv, tracer, class edges and depth edges: one entry, or one per carry (0, 1).
# An entry is the message (NF_ERR_STATE), or ('device', name): the product wants a device first, then `name` + GRID.
PRODUCTS = [
    ('nf_field_compute_profile', False, 'prof', 'compute_profile' + GRID, 'compute_profile' + GRID),
    ('nf_field_compute_tracer_profile', False, 'prof', S + ': set_tracer first', 'compute_tracer_profile' + GRID),
    ('nf_field_compute_area_profile', False, 'rows', S + ': set_tracer first', ('device', 'compute_area_profile')),
    ('nf_field_compute_gross_profile', True, 'rows', (('device', 'compute_gross_profile'), S + ': set_tracer first'),
     ('device', 'compute_gross_profile')),
    ('nf_field_compute_crossings', True, 'out', (('device', 'compute_crossings'), S + ': set_tracer first'),
     ('device', 'compute_crossings')),
    ('nf_field_compute_class_transport', False, 'rows', S + ': set_tracer first', S + GRID),
    ('nf_field_compute_class_tracer_transport', False, 'rows', S + ': set_tracer first', S + GRID),
    ('nf_field_compute_class_remap', True, 'rows', S + ': set_tracer first', S + GRID),
    ('nf_field_compute_depth_transport', True, 'rows', S + ': set_depth_edges first', S + GRID),
    ('nf_field_compute_surface_transport', True, 'rows', S + ': set_depth_surfaces first', S + ': set_depth_surfaces first'),
    ('nf_field_compute_joint_class_transport', True, 'rows', S + ': set_tracer first', S + ': set_class_tracer first'),
    ('nf_field_compute_gross_class_transport', True, 'rows', S + ': set_tracer first', S + GRID),
    ('nf_field_compute_gross_class_remap', True, 'rows', S + ': set_tracer first', S + GRID),
    ('nf_field_compute_class_area', False, 'rows', S + ': set_tracer first', S + GRID),
]
FORMS = [(p, suffix) for p in PRODUCTS for suffix in ('', '_async')]
IDS = [p[0][len('nf_field_compute_'):] + suffix for p, suffix in FORMS]


def _lib():
    from nemoflux_amd import _lib
    return _lib


def _has_device():
    """the library's own probe (not torch): how many GPUs the HIP runtime it is linked to can see"""
    n = ctypes.c_int(-1)
    assert _lib().lib.nf_device_count(ctypes.byref(n)) == 0
    return n.value > 0


def _call(symbol, has_carry, h, carry, rows):
    L = _lib()
    fn = getattr(L.lib, symbol)
    if rows is not None:
        rows = ctypes.c_void_p(rows.ctypes.data) if symbol.endswith('_async') else L.dptr(rows)
    return fn(h, 0, carry, rows) if has_carry else fn(h, 0, rows)


def _expected(entry, symbol, k, device):
    """(code, message) of entry `entry` of the table for carry number k"""
    if isinstance(entry, tuple) and entry[0] != 'device':
        entry = entry[k]
    if isinstance(entry, tuple):
        return (NF_ERR_STATE, entry[1] + GRID) if device else (NF_ERR_NO_DEVICE, NO_GPU)
    return NF_ERR_STATE, entry.format(s=symbol)


def test_the_table_names_fourteen_products():
    assert len(PRODUCTS) == 14 and len({p[0] for p in PRODUCTS}) == 14
    assert sum(1 for p in PRODUCTS if p[1]) == 8


@pytest.fixture(scope='module')
def exported():
    out = subprocess.run(['nm', '-D', '--defined-only', _lib()._SO], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stderr
    return {ln.split()[-1] for ln in out.stdout.splitlines() if ln.split()}


@pytest.fixture(scope='module')
def header():
    with open(os.path.join(ROOT, 'include', 'nemoflux_amd.h')) as fh:
        return re.sub(r'/\*.*?\*/', '', fh.read(), flags=re.S)


@pytest.mark.parametrize('product,suffix', FORMS, ids=IDS)
def test_declared_exported_and_bound(product, suffix, exported, header):
    stem, has_carry, rows_name = product[:3]
    symbol = stem + suffix
    m = re.search(r'\bint\s+' + symbol + r'\s*\(([^)]*)\)\s*;', header)
    assert m, f'{symbol} is not declared in include/nemoflux_amd.h'
    want = 'nf_field **self, long tIndex, ' + ('int carry, ' if has_carry else '') + 'double *' + rows_name + \
        ('_dev' if suffix else '_host')
    assert ' '.join(m.group(1).split()) == want
    assert symbol in exported
    fn = getattr(_lib().lib, symbol)
    assert fn.restype is ctypes.c_int
    rows_type = ctypes.c_void_p if suffix else _lib().c_double_p
    want_types = [ctypes.c_long] + ([ctypes.c_int] if has_carry else []) + [rows_type]
    assert len(fn.argtypes) == 1 + len(want_types)
    assert fn.argtypes[0]._type_ is ctypes.c_void_p           # nf_field **: a pointer to the opaque handle
    assert all(a is b for a, b in zip(fn.argtypes[1:], want_types))


@pytest.mark.parametrize('product,suffix', FORMS, ids=IDS)
def test_null_arguments_and_bad_carry(product, suffix):
    stem, has_carry = product[:2]
    symbol = stem + suffix
    lib = _lib().lib
    rows = numpy.zeros(256)
    assert _call(symbol, has_carry, None, 0, rows) == NF_ERR_ARG
    assert lib.nf_last_error().decode() == symbol + ': null argument'
    null_handle = ctypes.c_void_p()                       # a handle that was never made: *self is null
    assert _call(symbol, has_carry, ctypes.byref(null_handle), 0, rows) == NF_ERR_ARG
    assert lib.nf_last_error().decode() == symbol + ': null argument'
    h = ctypes.c_void_p()
    assert lib.nf_field_new(ctypes.byref(h)) == 0
    try:
        assert _call(symbol, has_carry, ctypes.byref(h), 0, None) == NF_ERR_ARG
        assert lib.nf_last_error().decode() == symbol + ': null argument'
        if has_carry:
            for carry in (2, -1):
                assert _call(symbol, has_carry, ctypes.byref(h), carry, rows) == NF_ERR_ARG
                assert lib.nf_last_error().decode() == symbol + ': carry must be 0 or 1'
                assert _call(symbol, has_carry, ctypes.byref(h), carry, None) == NF_ERR_ARG     # null comes first
                assert lib.nf_last_error().decode() == symbol + ': null argument'
    finally:
        assert lib.nf_field_del(ctypes.byref(h)) == 0
    assert not rows.any()


@pytest.fixture(scope='module')
def handles():
    """(fresh handle, handle with uv, tracer, class edges and depth edges set from host pointers)"""
    L = _lib()
    lib = L.lib
    fresh, some = ctypes.c_void_p(), ctypes.c_void_p()
    assert lib.nf_field_new(ctypes.byref(fresh)) == 0 and lib.nf_field_new(ctypes.byref(some)) == 0
    uv = numpy.zeros(16)
    edges = numpy.array([1., 2., 3.])
    assert lib.nf_field_set_uv(ctypes.byref(some), uv.ctypes.data, uv.ctypes.data, 3, NF_F64, 0, numpy.nan) == 0
    assert lib.nf_field_set_tracer(ctypes.byref(some), uv.ctypes.data, 3, NF_F64, 0, numpy.nan) == 0
    assert lib.nf_field_set_class_edges(ctypes.byref(some), L.dptr(edges), 3) == 0
    assert lib.nf_field_set_depth_edges(ctypes.byref(some), L.dptr(edges), 3, 0.0) == 0
    yield fresh, some, uv
    assert lib.nf_field_del(ctypes.byref(fresh)) == 0 and lib.nf_field_del(ctypes.byref(some)) == 0


@pytest.mark.parametrize('state', [0, 1], ids=['fresh', 'uv_tracer_edges'])
@pytest.mark.parametrize('product,suffix', FORMS, ids=IDS)
def test_first_state_message(product, suffix, state, handles):
    stem, has_carry = product[:2]
    symbol = stem + suffix
    lib = _lib().lib
    device = _has_device()
    rows = numpy.zeros(256)
    for k, carry in enumerate((0, 1) if has_carry else (0,)):
        code, message = _expected(product[3 + state], symbol, k, device)
        got = _call(symbol, has_carry, ctypes.byref(handles[state]), carry, rows)
        assert (got, lib.nf_last_error().decode()) == (code, message), (symbol, carry)
    assert not rows.any()


def test_which_calls_ask_for_a_device_before_the_grid():
    """which (product, state, carry) ask for a device before the grid: both forms alike"""
    want = {('area_profile', 1, 0), ('gross_profile', 0, 0), ('gross_profile', 1, 0), ('gross_profile', 1, 1),
            ('crossings', 0, 0), ('crossings', 1, 0), ('crossings', 1, 1)}
    got = set()
    for p in PRODUCTS:
        for state in (0, 1):
            for k in range(2 if p[1] else 1):
                if _expected(p[3 + state], p[0], k, False)[0] == NF_ERR_NO_DEVICE:
                    got.add((p[0][len('nf_field_compute_'):], state, k))
    assert got == want
