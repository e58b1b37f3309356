"""Gross (inflow / outflow) transports in tracer classes (nf_field_compute_gross_class_transport,
Field.computeGrossClassTransport, fluxplot --gross-classes), the part that needs no GPU: the reference of
tests/gross_class_reference.py pinned to a naive loop with math.fsum on a 12 x 9 x 3 case with land, both markers and the
Sverdrup scale, in every form (volume, carried tracer that is the class field, carried tracer with a class field of its own;
scalar, static and time-varying thickness); its sum over the classes against the gross profile reference; the two calls
declared, exported and bound, and the errors they decide before they need a device; the Field method; the fluxplot argument
checks."""
import ctypes
import math
import os
import re
import subprocess
import sys

import numpy
import pytest

from conftest import ROOT
from gross_class_reference import GrossClassReference
from gross_reference import (FILL, MIN_ABS_Q, MISSING, THFILL, THMISSING, GrossReference, array_values, gross_thickness,
                             gross_velocities, inputs_are_safe)
from test_gross_cpu import LINES, NT, NX, NY, NZ, REF, TFILL, TH, TMISSING, _tracer, _weights  # noqa: F401  (LINES: _weights)

EPS = numpy.finfo(numpy.float64).eps
NF_ERR_ARG, NF_ERR_STATE = 1, 2
NF_F64 = 0
CALLS = ('nf_field_compute_gross_class_transport', 'nf_field_compute_gross_class_transport_async')
SFILL, SMISSING = -8888., 5.e15
EDGES = numpy.array([26.25, 26.75, 27., 27.125, 27.75])


def _class_field(real, shape, seed):
    rng = numpy.random.default_rng(seed)
    dt = numpy.dtype(real).type
    sig = (27. + 1.2 * rng.standard_normal(shape)).astype(real)
    sig[rng.random(shape) < 0.05] = dt(EDGES[2])                  # values on an edge: the edge belongs to the class above
    for m in (SFILL, SMISSING, numpy.nan):
        sig[rng.random(shape) < 0.06] = dt(m)
    return sig


def _naive(ce, w, sg, arc, tr_off, a, t, cell_thickness, edges, class_marks):
    """P[r], N[r] of both forms as math.fsum of their terms, one (entry, level) at a time from the full arrays"""
    dt = a['uo'].dtype.type
    nseg, ntr = int(tr_off[-1]), len(tr_off) - 1
    tr_of = [p for p in range(ntr) for _ in range(tr_off[p], tr_off[p + 1])]
    n = len(edges)

    def present(x, marks):
        return not math.isnan(x) and all(x != dt(m) for m in marks)

    def val(name, tt, z, c):
        return a[name][tt, z].reshape(-1)[c]

    def face(name, z, ca, cb, marks):
        """(has a value, the raw value)"""
        xa = val(name, t, z, ca)
        pa = present(xa, marks)
        pb = cb is not None and present(val(name, t, z, cb), marks)
        if pa and pb:
            return True, 0.5 * (float(xa) + float(val(name, t, z, cb)))
        if pa:
            return True, float(xa)
        if pb:
            return True, float(val(name, t, z, cb))
        return False, 0.0

    terms = {'volume': {}, 'carried': {}}
    min_q = math.inf
    for e in range(len(ce)):
        c, slot, s = int(ce[e]) // 4, int(ce[e]) % 4, int(sg[e])
        j, i = divmod(c, NX)
        if slot == 0:
            if j == 0:
                continue
            ca, cb = c - NX, c
        elif slot == 1:
            ca, cb = c, (c + 1 if i < NX - 1 else c + 1 - NX)
        elif slot == 2:
            ca, cb = c, (c + NX if j < NY - 1 else None)
        else:
            ca, cb = (c - 1 if i > 0 else c - 1 + NX), c
        east = slot in (1, 3)
        for z in range(NZ):
            x = val('uo' if east else 'vo', t, z, ca)
            vel = float(x) if present(x, (FILL, MISSING)) else 0.0
            if cell_thickness:
                h = val('e3u' if east else 'e3v', t if a['e3u'].shape[0] > 1 else 0, z, ca)
                h = float(h) if present(h, (THFILL, THMISSING)) else 0.0
            else:
                h = float(TH[z])
            has_t, xt = face('tracer', z, ca, cb, (TFILL, TMISSING))
            tf = xt - REF if has_t else 0.0
            has_s, xs = face('class', z, ca, cb, class_marks)
            r = sum(1 for ed in edges if ed <= xs) if has_s and not math.isnan(xs) else n + 1
            al = float(arc[ca, 1]) if east else -float(arc[ca, 2])
            q = float(w[e]) * (((h * vel) * al) * (6371000.0 / 1.e6))
            cc = float(w[e]) * (((h * (vel * tf)) * al) * (6371000.0 / 1.e6))
            if q == 0.0:
                continue
            min_q = min(min_q, abs(q))
            part = 0 if q > 0 else 1
            for col in (s, nseg + tr_of[s]):
                terms['volume'].setdefault((part, r, col), []).append(q)
                terms['carried'].setdefault((part, r, col), []).append(cc)
    out = {'min_abs_q': min_q}
    for nm in terms:
        want, mag = numpy.zeros((2, n + 2, nseg + ntr)), numpy.zeros((2, n + 2, nseg + ntr))
        for idx, xs in terms[nm].items():
            want[idx], mag[idx] = math.fsum(xs), math.fsum(abs(x) for x in xs)
        out[nm] = (want, mag)
    return out


@pytest.mark.parametrize('own_class', [False, True], ids=['one-tracer', 'class-tracer'])
@pytest.mark.parametrize('thick', ['scalar', 'static', 'timevarying'])
@pytest.mark.parametrize('real', ['float64', 'float32'])
def test_reference_is_the_naive_loop_and_sums_to_the_gross_profile(oracle, real, thick, own_class):
    ce, wt, sg, arc, tr_off = _weights(oracle)
    shape = (NT, NZ, NY, NX)
    u, v = gross_velocities(real, shape, seed=5)
    arrays = {'uo': u, 'vo': v}
    if own_class:
        arrays['tracer'], arrays['class'] = _tracer(real, shape, seed=7), _class_field(real, shape, seed=13)
        class_marks, edges = (SFILL, SMISSING), EDGES
    else:
        arrays['tracer'] = arrays['class'] = _tracer(real, shape, seed=7)
        class_marks, edges = (TFILL, TMISSING), numpy.array([0.5, 2.75, REF, 5.])
    cell = thick != 'scalar'
    if cell:
        arrays['e3u'], arrays['e3v'] = gross_thickness(real, (NT if thick == 'timevarying' else 1, NZ, NY, NX), seed=9)
    assert inputs_are_safe(u, v, (arrays['e3u'], arrays['e3v']) if cell else ())
    kw = dict(uv_markers=(FILL, MISSING), tracer_markers=(TFILL, TMISSING), thick_markers=(THFILL, THMISSING), reference=REF,
              wrap=True, sverdrup=True, cell_thickness=cell)
    ref = GrossClassReference(ce, wt, sg, arc, TH, tr_off, NX, NY, class_markers=class_marks, **kw)
    prof = GrossReference(ce, wt, sg, arc, TH, tr_off, NX, NY, **kw)
    seen = numpy.zeros((2, edges.size + 2), bool)
    for t in range(NT):
        got = ref.gross_class_step(array_values(arrays, t), edges)
        want = _naive(ce, wt, sg, arc, tr_off, arrays, t, cell, edges, class_marks)
        assert got['min_abs_q'] == want['min_abs_q'] >= MIN_ABS_Q
        for nm in ('volume', 'carried'):
            (g_, gm_), (w_, m_) = got[nm], want[nm]
            assert g_.shape == w_.shape == gm_.shape == (2, edges.size + 2, ref.row_length), nm
            seen |= m_.max(axis=2) > 0
            assert numpy.all(numpy.abs(g_ - w_) <= 4 * EPS * m_), (nm, t)
            assert numpy.all(numpy.abs(gm_ - m_) <= 4 * EPS * m_), (nm, t)
        P, N = got['volume'][0]
        assert (P >= 0).all() and (N <= 0).all() and (P > 0).any() and (N < 0).any()
        assert (got['carried'][0][0] < 0).any() and (got['carried'][0][1] > 0).any()      # split by the water, not by its own sign
        # the sum over the classes is the sum over the levels of the gross profile
        by_level = prof.gross_step(array_values(arrays, t))
        for nm in ('volume', 'carried'):
            (g_, gm_), (w_, wm_) = got[nm], by_level[nm]
            assert numpy.all(numpy.abs(g_.sum(axis=1) - w_.sum(axis=1)) <= 8 * EPS * wm_.sum(axis=1)), (nm, t)
            assert numpy.all(numpy.abs(gm_.sum(axis=1) - wm_.sum(axis=1)) <= 8 * EPS * wm_.sum(axis=1)), (nm, t)
    assert seen[:, :-1].all(), 'every class has an inflow and an outflow'
    assert seen[:, -1].any() or not own_class, 'the row of the faces without a class value has terms'
    only_volume = ref.gross_class_step(array_values(arrays, 0), edges, tracer=False, threads=2)
    assert set(only_volume) == {'volume', 'min_abs_q'}
    assert numpy.allclose(only_volume['volume'][0], ref.gross_class_step(array_values(arrays, 0), edges)['volume'][0], rtol=4 * EPS,
                          atol=0)


# ---- ABI -------------------------------------------------------------------------------------------------------------------
def _header():
    with open(os.path.join(ROOT, 'include', 'nemoflux_amd.h')) as fh:
        return re.sub(r'/\*.*?\*/', '', fh.read(), flags=re.S)


def test_header_declares_and_library_exports_the_two_calls():
    from nemoflux_amd import _lib
    header = _header()
    out = subprocess.run(['nm', '-D', '--defined-only', _lib._SO], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stderr
    exported = {ln.split()[-1] for ln in out.stdout.splitlines() if ln.split()}
    for name, last in zip(CALLS, ('double *rows_host', 'double *rows_dev')):
        m = re.search(r'\bint\s+' + name + r'\s*\(([^)]*)\)\s*;', header)
        assert m, f'{name} is not declared in include/nemoflux_amd.h'
        assert ' '.join(m.group(1).split()) == 'nf_field **self, long tIndex, int carry, ' + last, name
        assert name in exported, name
        fn = getattr(_lib.lib, name)
        assert fn.restype is ctypes.c_int and fn.argtypes[1] is ctypes.c_long and fn.argtypes[2] is ctypes.c_int, name
        assert len(fn.argtypes) == 4, name


def _compute(name, h, carry, out):
    from nemoflux_amd import _lib
    fn = getattr(_lib.lib, name)
    if out is None:
        return fn(h, 0, carry, None)
    return fn(h, 0, carry, ctypes.c_void_p(out.ctypes.data) if name.endswith('_async') else _lib.dptr(out))


def test_argument_state_and_device_errors():
    """the words of the class transport's refusals: set_tracer first, then set_class_edges first -- in both forms, since the
    class field is needed either way"""
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
                assert b'set_tracer first' in lib.nf_last_error() and name.encode() in lib.nf_last_error()
        assert lib.nf_field_set_uv(ctypes.byref(h), uv.ctypes.data, uv.ctypes.data, 3, NF_F64, 0, numpy.nan) == 0
        assert lib.nf_field_set_tracer(ctypes.byref(h), uv.ctypes.data, 3, NF_F64, 0, numpy.nan) == 0
        for name in CALLS:
            for carry in (0, 1):
                assert _compute(name, ctypes.byref(h), carry, rows) == NF_ERR_STATE, name
                assert b'set_class_edges first' in lib.nf_last_error() and name.encode() in lib.nf_last_error()
        assert lib.nf_field_set_class_edges(ctypes.byref(h), _lib.dptr(edges), 3) == 0
        for name in CALLS:
            for carry in (0, 1):
                # no grid: like the class transport, the state is checked before a device is needed
                assert _compute(name, ctypes.byref(h), carry, rows) == NF_ERR_STATE, name
                assert b'set_bounds' in lib.nf_last_error() and name.encode() in lib.nf_last_error()
        assert not rows.any()
    finally:
        assert lib.nf_field_del(ctypes.byref(h)) == 0


# ---- Python ----------------------------------------------------------------------------------------------------------------
def test_python_method_checks_its_arguments():
    from nemoflux_amd.field import Field
    f = Field.__new__(Field)
    f.nt, f.nz, f.ny, f.nx = 2, 3, 4, 5
    f._lazy = None
    f._e3 = None
    with pytest.raises(RuntimeError, match='setClassEdges first'):
        f.computeGrossClassTransport(0)
    f._class_edges = numpy.array([1., 2.])
    with pytest.raises(RuntimeError, match='out of range'):
        f.computeGrossClassTransport(2)
    for carry in (False, True):
        with pytest.raises(RuntimeError, match='setTracer first'):
            f.computeGrossClassTransport(0, carry=carry)
    for name in ('grossTransport', 'transportWeightedTracer', 'classStreamfunction'):
        assert 'computeGrossClassTransport' in Field.__dict__[name].__func__.__doc__, name
    # the parts go into the existing helpers as they are
    rng = numpy.random.default_rng(4)
    parts = numpy.stack([rng.random((4, 3)), -rng.random((4, 3))])
    assert numpy.array_equal(Field.grossTransport(parts), parts.sum(axis=1))
    assert Field.classStreamfunction(parts[0] + parts[1]).shape == (2, 3)
    assert Field.transportWeightedTracer(parts, 2. * parts, 1.0).shape == parts.shape


# ---- fluxplot --------------------------------------------------------------------------------------------------------------
def test_fluxplot_gross_classes_options_are_checked():
    from nemoflux_amd.fluxplot import checkGrossClassArgs, main
    checkGrossClassArgs()
    checkGrossClassArgs('26,27,28', 'sigma0')
    with pytest.raises(RuntimeError, match='--gross-classes needs --tracer'):
        checkGrossClassArgs('26,27')
    for kw, opt in ((dict(classes='26,27'), '--classes'), (dict(classes2='34,35'), '--classes2'), (dict(gross=True), '--gross'),
                    (dict(levels=True), '--levels'), (dict(zrange='0,100'), '--zrange'), (dict(decompose=True), '--decompose'),
                    (dict(eddy=True), '--eddy'), (dict(show=True), '--show')):
        with pytest.raises(RuntimeError, match='--gross-classes and ' + opt + ' cannot'):
            checkGrossClassArgs('26,27', 'sigma0', **kw)
    for kw in (dict(tracerRef=1.0), dict(tracerScale=2.0)):
        with pytest.raises(RuntimeError, match='--tracer-ref / --tracer-scale do not apply'):
            checkGrossClassArgs('26,27', 'sigma0', **kw)
    for bad in ('26', '27,26', '26,x', '26,inf'):
        with pytest.raises(RuntimeError, match='--gross-classes'):
            checkGrossClassArgs(bad, 'sigma0')
    # refused before any file is opened: none of these files exists
    files = dict(tFile='/nonexistent/T.nc', uFile='/nonexistent/U.nc', vFile='/nonexistent/V.nc', lonLatPoints='(0,0),(1,1)')
    for kw in (dict(classes='26,27'), dict(classes='26,27', tracer2='so', classes2='34,35'), dict(gross=True), dict(levels=True),
               dict(zrange='0,100'), dict(decompose=True), dict(eddy=True), dict(show=True)):
        with pytest.raises(RuntimeError, match='--gross-classes and'):
            main(grossClasses='26,27', tracer='sigma0', **kw, **files)
    with pytest.raises(RuntimeError, match='--gross-classes needs --tracer'):
        main(grossClasses='26,27', **files)
    with pytest.raises(RuntimeError, match='--carry-ref / --carry-scale need --carry'):
        main(grossClasses='26,27', tracer='sigma0', carryScale=2.0, **files)
    # accepted combinations go on to open the files
    for kw in (dict(), dict(sverdrup=True), dict(cellThickness=True), dict(carry='thetao', carryRef=1.5, carryScale=4.1e-3),
               dict(carry='thetao', cellThickness=True, e3u='e3u_0', sverdrup=True)):
        with pytest.raises(RuntimeError, match='no such file'):
            main(grossClasses='26,27,28', tracer='sigma0', **kw, **files)
    # --gross --classes stays refused, and the net class forms still take no cell thickness
    with pytest.raises(RuntimeError, match='--gross and --classes'):
        main(gross=True, tracer='sigma0', classes='26,27', **files)
    with pytest.raises(RuntimeError, match='--cell-thickness cannot be combined with --classes'):
        main(tracer='sigma0', classes='26,27', cellThickness=True, **files)


def test_fluxplot_command_line_lists_gross_classes():
    out = subprocess.run([sys.executable, '-m', 'nemoflux_amd.fluxplot', '--help'], cwd=ROOT, capture_output=True, text=True,
                         timeout=120)
    assert out.returncode == 0, out.stderr
    assert '--gross-classes' in out.stdout
    bad = subprocess.run([sys.executable, '-m', 'nemoflux_amd.fluxplot', '-t', 'no_T.nc', '-u', 'no_U.nc', '-v', 'no_V.nc',
                          '-l', '[(0,0),(1,1)]', '--tracer', 'sigma0', '--gross-classes', '26,27', '--gross'], cwd=ROOT,
                         capture_output=True, text=True, timeout=120)
    assert bad.returncode != 0 and '--gross-classes and --gross' in bad.stderr
