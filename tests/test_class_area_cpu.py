"""Section area in tracer classes (nf_field_compute_class_area, Field.computeClassArea, Field.classMeanTracer,
Field.classInterfaceDepth, Field.decomposeTracerTransportByClass, fluxplot --class-area), the part that needs no GPU: the
reference of tests/class_area_reference.py pinned to a naive loop with math.fsum on a 12 x 9 x 3 case with land and both
markers, in both forms (the tracer binned by itself, a class field of its own) with the scalar, a static and a time-varying
thickness; its sum over the classes against the area profile reference; the mean tracer and the interface depth against scalar
loops, a closed form and monotonicity; the overturning / gyre split on class rows; the two calls declared, exported and bound,
and the errors they decide before they need a device; the Field method; the fluxplot argument checks."""
import ctypes
import math
import os
import re
import subprocess
import sys

import numpy
import pytest

from conftest import ROOT
from class_area_reference import ClassAreaReference
from gross_reference import FILL, MISSING, THFILL, THMISSING, array_values, gross_thickness, gross_velocities
from section_reference import SectionReference
from test_gross_class_cpu import EDGES, SFILL, SMISSING, _class_field
from test_gross_cpu import LINES, NT, NX, NY, NZ, REF, TFILL, TH, TMISSING, _tracer, _weights  # noqa: F401  (LINES: _weights)

EPS = numpy.finfo(numpy.float64).eps
NF_ERR_ARG, NF_ERR_STATE = 1, 2
NF_F64 = 0
CALLS = ('nf_field_compute_class_area', 'nf_field_compute_class_area_async')


def _naive(ce, w, sg, arc, tr_off, a, t, cell_thickness, edges, class_marks):
    """A[r], B[r] as math.fsum of their terms, one (entry, level) at a time from the full arrays"""
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

    terms = ({}, {})
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
            if not present(val('uo' if east else 'vo', t, z, ca), (FILL, MISSING)):
                continue
            has_t, xt = face('tracer', z, ca, cb, (TFILL, TMISSING))
            if not has_t or not math.isfinite(xt):
                continue
            if cell_thickness:
                h = val('e3u' if east else 'e3v', t if a['e3u'].shape[0] > 1 else 0, z, ca)
                h = float(h) if present(h, (THFILL, THMISSING)) else 0.0
            else:
                h = float(TH[z])
            has_s, xs = face('class', z, ca, cb, class_marks)
            r = sum(1 for ed in edges if ed <= xs) if has_s and not math.isnan(xs) else n + 1
            alpha = abs(float(w[e])) * (h * float(arc[ca, 1] if east else arc[ca, 2]))
            for col in (s, nseg + tr_of[s]):
                terms[0].setdefault((r, col), []).append(alpha)
                terms[1].setdefault((r, col), []).append(alpha * (xt - REF))
    want, mag = numpy.zeros((2, n + 2, nseg + ntr)), numpy.zeros((2, n + 2, nseg + ntr))
    for part in range(2):
        for idx, xs in terms[part].items():
            want[(part,) + idx], mag[(part,) + idx] = math.fsum(xs), math.fsum(abs(x) for x in xs)
    return want, mag


def _case(real, thick, own_class):
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
    kw = dict(uv_markers=(FILL, MISSING), tracer_markers=(TFILL, TMISSING), thick_markers=(THFILL, THMISSING), reference=REF,
              wrap=True, cell_thickness=cell)
    return arrays, class_marks, edges, cell, kw


@pytest.mark.parametrize('own_class', [False, True], ids=['one-tracer', 'class-tracer'])
@pytest.mark.parametrize('thick', ['scalar', 'static', 'timevarying'])
@pytest.mark.parametrize('real', ['float64', 'float32'])
def test_reference_is_the_naive_loop_and_sums_to_the_area_profile(oracle, real, thick, own_class):
    ce, wt, sg, arc, tr_off = _weights(oracle)
    arrays, class_marks, edges, cell, kw = _case(real, thick, own_class)
    ref = ClassAreaReference(ce, wt, sg, arc, TH, tr_off, NX, NY, class_markers=class_marks, **kw)
    prof = SectionReference(ce, wt, sg, arc, TH, tr_off, NX, NY, **kw)
    seen = numpy.zeros(edges.size + 2, bool)
    for t in range(NT):
        got, gmag = ref.class_area_step(array_values(arrays, t), edges)
        want, mag = _naive(ce, wt, sg, arc, tr_off, arrays, t, cell, edges, class_marks)
        assert got.shape == want.shape == gmag.shape == (2, edges.size + 2, ref.row_length)
        seen |= mag[0].max(axis=1) > 0
        assert numpy.all(numpy.abs(got - want) <= 4 * EPS * mag), t
        assert numpy.all(numpy.abs(gmag - mag) <= 4 * EPS * mag), t
        assert (got[0] >= 0).all() and numpy.array_equal(gmag[0], got[0])
        assert (got[1] < 0).any() and (got[1] > 0).any()
        # the sum over the classes is the sum over the levels of the area profile
        by_level = prof.area_step(array_values(arrays, t))
        for part, nm in enumerate(('area_profile', 'tracer_area_profile')):
            w_, wm_ = by_level[nm]
            assert numpy.abs(w_).max() > 0
            assert numpy.all(numpy.abs(got[part].sum(axis=0) - w_.sum(axis=0)) <= 8 * EPS * wm_.sum(axis=0)), (nm, t)
            assert numpy.all(numpy.abs(gmag[part].sum(axis=0) - wm_.sum(axis=0)) <= 8 * EPS * wm_.sum(axis=0)), (nm, t)
    assert seen[:-1].all(), 'every class has some area'
    assert seen[-1] == own_class, 'the row of the faces without a class value has terms exactly with a class field of its own'
    threaded = ref.class_area_step(array_values(arrays, 0), edges, threads=2)
    assert numpy.allclose(threaded[0], ref.class_area_step(array_values(arrays, 0), edges)[0], rtol=4 * EPS, atol=0)


# ---- the host-side helpers ---------------------------------------------------------------------------------------------------
def test_class_mean_tracer_is_the_scalar_loop():
    from nemoflux_amd.field import Field
    rng = numpy.random.default_rng(3)
    A = rng.random((6, 4))
    A[2, 1] = A[5] = 0.0
    B = A * rng.standard_normal((6, 4))
    got = Field.classMeanTracer(numpy.stack([A, B]), reference=1.5)
    assert got.shape == A.shape
    for k in range(6):
        for c in range(4):
            if A[k, c] == 0.0:
                assert math.isnan(got[k, c])
            else:
                assert got[k, c] == B[k, c] / A[k, c] + 1.5
    assert numpy.array_equal(Field.classMeanTracer((A, B))[A != 0], (B / numpy.where(A != 0, A, 1.))[A != 0])
    with pytest.raises(ValueError, match='classMeanTracer'):
        Field.classMeanTracer(numpy.zeros((3, 4)))


def _scalar_depth(C, Z, bd):
    """the interface depths of contiguous levels, one (column, edge) at a time: walk down the levels until the area above holds
    the fraction"""
    nedges, n = C.shape[0] - 2, C.shape[1]
    out = numpy.full((nedges, n), numpy.nan)
    for c in range(n):
        total = 0.0
        for k in range(nedges + 1):
            total += C[k, c]
        gtot = 0.0
        for z in range(Z.shape[0]):
            gtot += Z[z, c]
        if not total > 0.0 or not gtot > 0.0:
            continue
        cum = 0.0
        for k in range(nedges):
            cum += C[k, c]
            target = cum / total * gtot
            d, above = bd[0, 0], 0.0
            if target > 0.0:
                d = bd[-1, 1]
                for z in range(Z.shape[0]):
                    if above + Z[z, c] >= target:
                        d = bd[z, 0] + (target - above) / Z[z, c] * (bd[z, 1] - bd[z, 0]) if Z[z, c] > 0.0 else bd[z, 0]
                        break
                    above += Z[z, c]
            out[k, c] = d
    return out


def _bounds(th, top=0.0):
    b = top + numpy.concatenate([[0.], numpy.cumsum(th)])
    return numpy.stack([b[:-1], b[1:]], axis=1)


def test_class_interface_depth_is_the_scalar_loop_and_monotonic():
    from nemoflux_amd.field import Field
    rng = numpy.random.default_rng(8)
    nz, nedges, n = 7, 9, 6
    bd = _bounds(numpy.array([0.5, 1.0, 0.25, 3.0, 2.0, 10.0, 0.125]), top=2.0)        # unequal levels
    Z = rng.random((nz, n)) + 0.1
    Z[:2, 1] = 0.0                  # nothing in the two top levels of column 1
    Z[3, 2] = 0.0                   # a level without area inside column 2: G is flat there
    Z[:, 4] = 0.0                   # a column without area
    C = rng.random((nedges + 2, n)) + 0.05
    C[:3, 0] = 0.0                  # the three lightest classes are absent from column 0: phi = 0
    C[4:6, 3] = 0.0                 # two empty classes inside column 3
    C[:, 5] = 0.0                   # a column whose classes hold nothing
    got = Field.classInterfaceDepth(C, Z, bd)
    want = _scalar_depth(C, Z, bd)
    assert got.shape == (nedges, n)
    assert numpy.isnan(got[:, 4]).all() and numpy.isnan(got[:, 5]).all() and numpy.isfinite(got[:, :4]).all()
    assert numpy.array_equal(numpy.isnan(got), numpy.isnan(want))
    ok = numpy.isfinite(want)
    assert numpy.all(numpy.abs(got - want)[ok] <= 1e-12 * bd[-1, 1])
    assert numpy.all(numpy.diff(got[:, :4], axis=0) >= 0)                               # non-decreasing in k
    assert numpy.all(got[:, :4] >= bd[0, 0]) and numpy.all(got[:, :4] <= bd[-1, 1])
    assert (got[:3, 0] == bd[0, 0]).all()                                               # phi = 0: the top of the column
    assert got[0, 1] > bd[1, 1]                                                         # below the levels without area
    assert got[5, 3] == got[4, 3] == got[3, 3]                                          # empty classes: the same interface
    # the row of the faces without a class value does not enter
    C2 = C.copy()
    C2[-1] *= 7.0
    assert numpy.array_equal(Field.classInterfaceDepth(C2, Z, bd), got, equal_nan=True)
    # scaling either area changes nothing beyond rounding: only fractions enter
    assert numpy.allclose(Field.classInterfaceDepth(4.0 * C, 0.5 * Z, bd)[:, :4], got[:, :4], rtol=1e-13, atol=0)
    for bad in ((C[:3], Z, bd), (C, Z[:, :3], bd), (C, Z, bd[:-1]), (C, Z, bd[:, ::-1])):
        with pytest.raises(ValueError, match='classInterfaceDepth'):
            Field.classInterfaceDepth(*bad)


def test_class_interface_depth_closed_form(oracle):
    """the class field a strictly increasing function of the level alone, the edges between the values of consecutive levels:
    class k is level k, so the depth of edge k is the bottom of level k"""
    from nemoflux_amd.field import Field
    ce, wt, sg, arc, tr_off = _weights(oracle)
    shape = (NT, NZ, NY, NX)
    th = numpy.array([0.5, 0.25, 2.0])                                                  # unequal levels
    bd = _bounds(th, top=1.0)
    sigma = 24. + numpy.cumsum([0., 1.5, 0.75])                                         # of the level alone
    arrays = {'uo': numpy.ones(shape), 'vo': numpy.ones(shape), 'tracer': numpy.full(shape, 4.0),
              'class': numpy.ascontiguousarray(numpy.broadcast_to(sigma[None, :, None, None], shape))}
    edges = 0.5 * (sigma[:-1] + sigma[1:])
    ref = ClassAreaReference(ce, wt, sg, arc, th, tr_off, NX, NY, reference=REF)
    A = ref.class_area_step(array_values(arrays, 0), edges)[0][0]
    Z = SectionReference(ce, wt, sg, arc, th, tr_off, NX, NY, reference=REF).area_step(array_values(arrays, 0))['area_profile'][0]
    assert (Z > 0).all() and numpy.array_equal(A[:NZ], Z) and not A[NZ].any()
    zero = numpy.zeros((A.shape[0], 1))
    A, Z = numpy.concatenate([A, zero], axis=1), numpy.concatenate([Z, zero[:NZ]], axis=1)   # and a column with zero area
    got = Field.classInterfaceDepth(A, Z, bd)
    assert got.shape == (NZ - 1, ref.row_length + 1)
    assert numpy.isnan(got[:, -1]).all()
    want = numpy.broadcast_to(bd[:NZ - 1, 1][:, None], got[:, :-1].shape)
    assert numpy.all(numpy.abs(got[:, :-1] - want) <= 1e-12 * want)
    # a synthetic case with more levels: the same closed form
    rng = numpy.random.default_rng(21)
    bd = _bounds(rng.uniform(0.1, 50., 11))
    Z = rng.uniform(0.5, 2., (11, 4))
    Z[:, 2] = 0.0
    got = Field.classInterfaceDepth(numpy.concatenate([Z, numpy.zeros((1, 4))]), Z, bd)
    want = numpy.broadcast_to(bd[:10, 1][:, None], (10, 4))
    assert numpy.isnan(got[:, 2]).all()
    assert numpy.all(numpy.abs(got - want)[:, [0, 1, 3]] <= 1e-12 * want[:, [0, 1, 3]])


@pytest.mark.parametrize('own_class', [False, True], ids=['one-tracer', 'class-tracer'])
def test_overturning_gyre_on_class_rows_closes(oracle, own_class):
    """V of the class transport, (A, B) of the class area and H of the tracer transport, all from the references: the three
    parts add up to the total, the means are those of classMeanTracer, and the throughflow is that of the level rows"""
    from nemoflux_amd.field import Field
    from resolved_reference import ResolvedReference
    ce, wt, sg, arc, tr_off = _weights(oracle)
    arrays, class_marks, edges, cell, kw = _case('float64', 'scalar', own_class)
    ref = ClassAreaReference(ce, wt, sg, arc, TH, tr_off, NX, NY, class_markers=class_marks, **kw)
    res = ResolvedReference(ce, wt, sg, arc, TH, tr_off, NX, NY, class_markers=class_marks, **kw)
    for t in range(NT):
        AB = ref.class_area_step(array_values(arrays, t), edges)[0]
        step = res.step(array_values(arrays, t), [edges])
        V, (H, Hmag) = step['volume_classes', 0][0], step['tracer']
        d = Field.overturningGyre(V, (AB[0], AB[1]), H)
        assert set(d) == {'total', 'throughflow', 'overturning', 'gyre', 'mean'} and d['mean'].shape == V.shape
        assert numpy.array_equal(d['total'], H)
        m = Field.classMeanTracer(AB)
        assert numpy.array_equal(d['mean'][AB[0] != 0], m[AB[0] != 0]) and not d['mean'][AB[0] == 0].any()
        M = AB[1].sum(axis=0) / AB[0].sum(axis=0)
        terms = numpy.abs(Hmag) + numpy.abs(V.sum(axis=0) * M) + (numpy.abs(V) * numpy.abs(d['mean'] - M)).sum(axis=0)
        assert numpy.abs(d['overturning']).max() > 0 and numpy.abs(d['gyre']).max() > 0
        assert numpy.all(numpy.abs(d['throughflow'] + d['overturning'] + d['gyre'] - d['total']) <= 1e-12 * terms)
        by_level = SectionReference(ce, wt, sg, arc, TH, tr_off, NX, NY, **kw).area_step(array_values(arrays, t))
        lev = Field.overturningGyre(step['volume_profile'][0], (by_level['area_profile'][0], by_level['tracer_area_profile'][0]), H)
        assert numpy.all(numpy.abs(lev['throughflow'] - d['throughflow']) <= 1e-12 * terms)


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
        assert ' '.join(m.group(1).split()) == 'nf_field **self, long tIndex, ' + last, name
        assert name in exported, name
        fn = getattr(_lib.lib, name)
        assert fn.restype is ctypes.c_int and fn.argtypes[1] is ctypes.c_long and len(fn.argtypes) == 3, name


def _compute(name, h, out):
    from nemoflux_amd import _lib
    fn = getattr(_lib.lib, name)
    if out is None:
        return fn(h, 0, None)
    return fn(h, 0, ctypes.c_void_p(out.ctypes.data) if name.endswith('_async') else _lib.dptr(out))


def test_argument_state_and_device_errors():
    """the words of the class transport's refusals: set_tracer first, then set_class_edges first"""
    from nemoflux_amd import _lib
    lib = _lib.lib
    rows = numpy.zeros(256)
    uv = numpy.zeros(16)
    edges = numpy.array([1., 2., 3.])
    for name in CALLS:
        assert _compute(name, None, rows) == NF_ERR_ARG, name
        assert b'null' in lib.nf_last_error() and name.encode() in lib.nf_last_error()
    h = ctypes.c_void_p()
    assert lib.nf_field_new(ctypes.byref(h)) == 0
    try:
        for name in CALLS:
            assert _compute(name, ctypes.byref(h), None) == NF_ERR_ARG, name
            assert b'null' in lib.nf_last_error() and name.encode() in lib.nf_last_error()
            assert _compute(name, ctypes.byref(h), rows) == NF_ERR_STATE, name
            assert b'set_tracer first' in lib.nf_last_error() and name.encode() in lib.nf_last_error()
        assert lib.nf_field_set_uv(ctypes.byref(h), uv.ctypes.data, uv.ctypes.data, 3, NF_F64, 0, numpy.nan) == 0
        assert lib.nf_field_set_tracer(ctypes.byref(h), uv.ctypes.data, 3, NF_F64, 0, numpy.nan) == 0
        for name in CALLS:
            assert _compute(name, ctypes.byref(h), rows) == NF_ERR_STATE, name
            assert b'set_class_edges first' in lib.nf_last_error() and name.encode() in lib.nf_last_error()
        assert lib.nf_field_set_class_edges(ctypes.byref(h), _lib.dptr(edges), 3) == 0
        for name in CALLS:
            # no grid: like the class transport, the state is checked before a device is needed
            assert _compute(name, ctypes.byref(h), rows) == NF_ERR_STATE, name
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
    for call in (f.computeClassArea, f.decomposeTracerTransportByClass):
        with pytest.raises(RuntimeError, match='setClassEdges first'):
            call(0)
    f._class_edges = numpy.array([1., 2.])
    with pytest.raises(RuntimeError, match='out of range'):
        f.computeClassArea(2)
    with pytest.raises(RuntimeError, match='setTracer first'):
        f.computeClassArea(0)
    assert 'computeClassArea' in Field.__dict__['overturningGyre'].__func__.__doc__
    for name in ('classMeanTracer', 'classInterfaceDepth'):
        assert isinstance(Field.__dict__[name], staticmethod), name


# ---- fluxplot --------------------------------------------------------------------------------------------------------------
def test_fluxplot_class_area_options_are_checked():
    from nemoflux_amd.fluxplot import checkClassAreaArgs, main
    checkClassAreaArgs()
    checkClassAreaArgs('26,27,28', 'sigma0')
    with pytest.raises(RuntimeError, match='--class-area needs --tracer'):
        checkClassAreaArgs('26,27')
    for kw, opt in ((dict(classes='26,27'), '--classes'), (dict(classes2='34,35'), '--classes2'), (dict(gross=True), '--gross'),
                    (dict(grossClasses='26,27'), '--gross-classes'), (dict(levels=True), '--levels'),
                    (dict(zrange='0,100'), '--zrange'), (dict(decompose=True), '--decompose'), (dict(eddy=True), '--eddy'),
                    (dict(show=True), '--show')):
        with pytest.raises(RuntimeError, match='--class-area and ' + opt + ' cannot'):
            checkClassAreaArgs('26,27', 'sigma0', **kw)
    for kw in (dict(tracerRef=1.0), dict(tracerScale=2.0)):
        with pytest.raises(RuntimeError, match='--tracer-ref / --tracer-scale do not apply'):
            checkClassAreaArgs('26,27', 'sigma0', **kw)
    with pytest.raises(RuntimeError, match='--carry-scale does not apply'):
        checkClassAreaArgs('26,27', 'sigma0', carryScale=2.0)
    for bad in ('26', '27,26', '26,x', '26,inf'):
        with pytest.raises(RuntimeError, match='--class-area'):
            checkClassAreaArgs(bad, 'sigma0')
    # refused before any file is opened: none of these files exists
    files = dict(tFile='/nonexistent/T.nc', uFile='/nonexistent/U.nc', vFile='/nonexistent/V.nc', lonLatPoints='(0,0),(1,1)')
    for kw in (dict(classes='26,27'), dict(gross=True), dict(grossClasses='26,27'), dict(levels=True), dict(zrange='0,100'),
               dict(decompose=True), dict(eddy=True), dict(show=True)):
        with pytest.raises(RuntimeError, match='--class-area and'):
            main(classArea='26,27', tracer='sigma0', **kw, **files)
    with pytest.raises(RuntimeError, match='--class-area needs --tracer'):
        main(classArea='26,27', **files)
    with pytest.raises(RuntimeError, match='--carry-ref / --carry-scale need --carry'):
        main(classArea='26,27', tracer='sigma0', carryRef=2.0, **files)
    with pytest.raises(RuntimeError, match='--sigma and --tracer cannot be combined'):
        main(classArea='26,27', tracer='sigma0', sigma='thetao,so', **files)
    # accepted combinations go on to open the files
    for kw in (dict(tracer='sigma0'), dict(tracer='sigma0', sverdrup=True), dict(tracer='sigma0', cellThickness=True),
               dict(tracer='sigma0', carry='thetao', carryRef=1.5), dict(sigma='thetao,so,2000', carry='thetao'),
               dict(tracer='sigma0', carry='thetao', cellThickness=True, e3u='e3u_0')):
        with pytest.raises(RuntimeError, match='no such file'):
            main(classArea='26,27,28', **kw, **files)
    # the refusals of the siblings stand
    with pytest.raises(RuntimeError, match='--sigma needs --classes, --gross-classes or --classes2'):
        main(sigma='thetao,so', **files)
    with pytest.raises(RuntimeError, match='--cell-thickness cannot be combined with --classes'):
        main(tracer='sigma0', classes='26,27', cellThickness=True, **files)


def test_fluxplot_command_line_lists_class_area():
    out = subprocess.run([sys.executable, '-m', 'nemoflux_amd.fluxplot', '--help'], cwd=ROOT, capture_output=True, text=True,
                         timeout=120)
    assert out.returncode == 0, out.stderr
    assert '--class-area' in out.stdout
    bad = subprocess.run([sys.executable, '-m', 'nemoflux_amd.fluxplot', '-t', 'no_T.nc', '-u', 'no_U.nc', '-v', 'no_V.nc',
                          '-l', '[(0,0),(1,1)]', '--tracer', 'sigma0', '--class-area', '26,27', '--gross'], cwd=ROOT,
                         capture_output=True, text=True, timeout=120)
    assert bad.returncode != 0 and '--class-area and --gross' in bad.stderr
