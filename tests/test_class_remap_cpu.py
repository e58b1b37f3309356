"""Conservative (piecewise-linear) remapping of the class transport (nf_field_compute_class_remap, Field.computeClassRemap,
fluxplot --remap linear), the part that needs no GPU: the reference of tests/class_remap_reference.py pinned to a naive scalar
loop with math.fsum at 4 eps x sum |share| per value, on a 12 x 9 x 3 case with land, both markers, NaN, +-inf and values on
class edges in the class field, in every form (volume, carried tracer that is the class field, carried tracer with a class field
of its own) and with a single level; the fallbacks one by one; the fractions of every spread term add up to 1 within 4 eps; the
rows add up to those of the step rule; the two calls declared, exported and bound, and the errors they decide before they need
a device; the Field method; the fluxplot argument checks."""
import ctypes
import math
import os
import re
import subprocess
import sys

import numpy
import pytest

from class_remap_reference import ClassRemapReference, face_intervals, shares
from conftest import ROOT
from gross_reference import FILL, MISSING, array_values, gross_velocities
from test_gross_cpu import LINES, NT, NX, NY, NZ, REF, TFILL, TH, TMISSING, _weights  # noqa: F401  (LINES: _weights)

EPS = numpy.finfo(numpy.float64).eps
NF_ERR_ARG, NF_ERR_STATE = 1, 2
NF_F64 = 0
CALLS = ('nf_field_compute_class_remap', 'nf_field_compute_class_remap_async')
SFILL, SMISSING = -8888., 5.e15
EDGES = numpy.array([-1., 2.5, 3., 3.25, 3.5, 4.75, 6.5])
SV = 6371000.0 / 1.e6


def _lattice(real, shape, seed, marks, inf=True):
    """values on a 2^-10 lattice in [-2, 32] with a trend in z, so that layers span several classes; columns that are constant
    in z (lo == hi), values on an edge, both markers, NaN and (inf: a class field that is not carried) +-inf"""
    rng = numpy.random.default_rng(seed)
    dt = numpy.dtype(real).type
    nz = shape[1]
    x = rng.integers(0, 4 * 1024, shape) / 1024. + 2.5 * numpy.arange(nz)[None, :, None, None] - 2.
    x = numpy.clip(x, -2., 32.).astype(real)
    x[:, :, ::3, ::4] = x[:, :1, ::3, ::4]                         # constant in z
    x[rng.random(shape) < 0.05] = dt(EDGES[2])                     # on an edge: the edge belongs to the class above
    for m in marks + (numpy.nan,) + ((numpy.inf, -numpy.inf) if inf else ()):
        x[rng.random(shape) < 0.04] = dt(m)
    return x


def _naive(ce, w, sg, arc, tr_off, a, t, edges, class_marks, nz):
    """the rows of both forms as math.fsum of their shares, one (entry, level, row) at a time from the full arrays; also the
    largest |sum of the fractions of a spread term - 1|"""
    dt = a['uo'].dtype.type
    nseg, ntr = int(tr_off[-1]), len(tr_off) - 1
    tr_of = [p for p in range(ntr) for _ in range(tr_off[p], tr_off[p + 1])]
    n = len(edges)

    def present(x, marks):
        return not math.isnan(x) and all(x != dt(m) for m in marks)

    def val(name, z, c):
        return a[name][t, z].reshape(-1)[c]

    def face(name, z, ca, cb, marks):
        xa = val(name, z, ca)
        pa = present(xa, marks)
        pb = cb is not None and present(val(name, z, cb), marks)
        if pa and pb:
            return True, 0.5 * (float(xa) + float(val(name, z, cb)))
        if pa:
            return True, float(xa)
        if pb:
            return True, float(val(name, z, cb))
        return False, 0.0

    def row(x):
        return sum(1 for ed in edges if ed <= x)

    def fractions(z, ca, cb):
        """[(row, fraction or None for the whole term)]"""
        has, f = face('class', z, ca, cb, class_marks)
        if not has or math.isnan(f):
            return [(n + 1, None)]
        g = []
        for zz in (z - 1, z + 1):
            hn, fn = face('class', zz, ca, cb, class_marks) if 0 <= zz < nz else (False, 0.0)
            g.append(0.5 * (fn + f) if hn else f)
        if not (math.isfinite(g[0]) and math.isfinite(g[1]) and math.isfinite(g[1] - g[0])):
            return [(row(f), None)]
        lo, hi = min(g), max(g)
        if lo == hi:
            return [(row(lo), None)]
        out = []
        for j in range(row(lo), row(hi) + 1):
            left = lo if j == row(lo) else float(edges[j - 1])
            right = hi if j == row(hi) else float(edges[j])
            if right != left:
                out.append((j, (right - left) / (hi - lo)))
        return out

    terms = {'volume': {}, 'carried': {}}
    worst = 0.0
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
        for z in range(nz):
            x = val('uo' if east else 'vo', z, ca)
            vel = float(x) if present(x, (FILL, MISSING)) else 0.0
            h = float(TH[z])
            has_t, xt = face('tracer', z, ca, cb, (TFILL, TMISSING))
            tf = xt - REF if has_t else 0.0
            al = float(arc[ca, 1]) if east else -float(arc[ca, 2])
            q = float(w[e]) * (((h * vel) * al) * SV)
            cc = float(w[e]) * (((h * (vel * tf)) * al) * SV)
            fr = fractions(z, ca, cb)
            if fr[0][1] is not None:
                worst = max(worst, abs(math.fsum(x for _, x in fr) - 1.0))
            for r, x in fr:
                for col in (s, nseg + tr_of[s]):
                    terms['volume'].setdefault((r, col), []).append(q if x is None else q * x)
                    terms['carried'].setdefault((r, col), []).append(cc if x is None else cc * x)
    out = {'fraction_error': worst}
    for nm in terms:
        want, mag = numpy.zeros((n + 2, nseg + ntr)), numpy.zeros((n + 2, nseg + ntr))
        for idx, xs in terms[nm].items():
            want[idx], mag[idx] = math.fsum(xs), math.fsum(abs(x) for x in xs)
        out[nm] = (want, mag)
    return out


def _tracer(real, shape, seed):
    rng = numpy.random.default_rng(seed)
    dt = numpy.dtype(real).type
    tau = (REF + 2. * rng.standard_normal(shape)).astype(real)
    for m in (TFILL, TMISSING, numpy.nan):
        tau[rng.random(shape) < 0.05] = dt(m)
    return tau


@pytest.mark.parametrize('nz', [NZ, 1], ids=['three-levels', 'one-level'])
@pytest.mark.parametrize('own_class', [False, True], ids=['one-tracer', 'class-tracer'])
@pytest.mark.parametrize('real', ['float64', 'float32'])
def test_reference_is_the_naive_loop(oracle, real, own_class, nz):
    ce, wt, sg, arc, tr_off = _weights(oracle)
    shape = (NT, nz, NY, NX)
    u, v = gross_velocities(real, (NT, NZ, NY, NX), seed=5)
    arrays = {'uo': u[:, :nz], 'vo': v[:, :nz]}
    if own_class:
        arrays['tracer'], arrays['class'], marks = _tracer(real, shape, 7), _lattice(real, shape, 13, (SFILL, SMISSING)), (SFILL, SMISSING)
    else:
        arrays['tracer'] = arrays['class'] = _lattice(real, shape, 13, (TFILL, TMISSING), inf=False)
        marks = (TFILL, TMISSING)
    cls = arrays['class']
    assert numpy.isnan(cls).any() and (cls == EDGES[2]).any()
    assert not own_class or (numpy.isposinf(cls).any() and numpy.isneginf(cls).any())
    kw = dict(uv_markers=(FILL, MISSING), tracer_markers=(TFILL, TMISSING), reference=REF, wrap=True, sverdrup=True)
    ref = ClassRemapReference(ce, wt, sg, arc, TH[:nz], tr_off, NX, NY, class_markers=marks, **kw)
    seen = numpy.zeros(EDGES.size + 2, bool)
    for t in range(NT):
        got = ref.remap_step(array_values(arrays, t), EDGES)
        want = _naive(ce, wt, sg, arc, tr_off, arrays, t, EDGES, marks, nz)
        for nm in ('volume', 'carried'):
            (g_, gm_), (w_, m_) = got[nm], want[nm]
            assert g_.shape == w_.shape == gm_.shape == (EDGES.size + 2, ref.row_length), nm
            seen |= m_.max(axis=1) > 0
            assert numpy.all(numpy.abs(g_ - w_) <= 4 * EPS * m_), (nm, t)
            assert numpy.all(numpy.abs(gm_ - m_) <= 4 * EPS * m_), (nm, t)
        # the fractions of every spread term add up to 1
        assert got['fraction_error'] <= 4 * EPS and want['fraction_error'] <= 4 * EPS
        if nz == 1:
            assert got['spread_terms'] == 0 and got['rows_per_term'] == 1.0      # one level: no interfaces, the step rule
        else:
            assert got['spread_terms'] > 50 and got['rows_per_term'] > 1.5
        # conservation: the rows add up to the rows of the step rule, the class rows of ResolvedReference
        step = ref.step(array_values(arrays, t), [EDGES])
        for nm, key in (('volume', 'volume_classes'), ('carried', 'tracer_classes')):
            (g_, gm_), (w_, wm_) = got[nm], step[key, 0]
            assert numpy.all(numpy.abs(g_.sum(axis=0) - w_.sum(axis=0)) <= 8 * EPS * wm_.sum(axis=0)), (nm, t)
            assert numpy.all(numpy.abs(gm_.sum(axis=0) - wm_.sum(axis=0)) <= 8 * EPS * wm_.sum(axis=0)), (nm, t)
            if nz == 1:
                assert numpy.array_equal(g_, w_) and numpy.array_equal(gm_, wm_), (nm, t)
    assert seen.all() or nz == 1, 'every row, the one of the faces without a class value included, has terms'
    only_volume = ref.remap_step(array_values(arrays, 0), EDGES, tracer=False, threads=2)
    assert 'carried' not in only_volume
    assert numpy.allclose(only_volume['volume'][0], ref.remap_step(array_values(arrays, 0), EDGES)['volume'][0], rtol=4 * EPS, atol=0)


def test_the_fallbacks_one_by_one():
    e = numpy.array([0., 1., 2., 4.])
    n, inf, nan = e.size, numpy.inf, numpy.nan

    def one(cur, up=None, dn=None):
        wrap = lambda p: None if p is None else (numpy.array([p[0]]), numpy.array([float(p[1])]))   # noqa: E731
        ent, row, frac = shares(*face_intervals(wrap(cur), wrap(up), wrap(dn)), e)
        assert not ent.any()
        return list(zip(row.tolist(), frac.tolist()))

    assert one((False, 1.5), (True, 0.5), (True, 2.5)) == [(n + 1, 1.0)]          # no class value
    assert one((True, nan), (True, 0.5), (True, 2.5)) == [(n + 1, 1.0)]           # NaN (+inf beside -inf)
    assert one((True, 1.5)) == [(2, 1.0)]                                         # a single level: the step rule
    assert one((True, 1.5), (False, 9.), (False, -9.)) == [(2, 1.0)]              # no value above or below
    assert one((True, 1.5), (True, inf), (True, 2.5)) == [(2, 1.0)]               # a non-finite interface
    assert one((True, 1.5), (True, nan), (True, 2.5)) == [(2, 1.0)]
    assert one((True, inf), (True, 1.), (True, 2.)) == [(n, 1.0)]
    assert one((True, -inf), (True, 1.), (True, 2.)) == [(0, 1.0)]
    big = numpy.finfo(numpy.float64).max
    assert one((True, big), (True, big), (True, 1.)) == [(n, 1.0)]                # f_{z-1} + f_z overflows
    assert one((True, 1.5), (True, 1.5), (True, 1.5)) == [(2, 1.0)]               # lo == hi
    assert one((True, 1.), (True, 1.), (True, 1.)) == [(2, 1.0)]                  # ... on an edge: the class above
    assert one((True, 1.25), (True, 1.75), (True, 1.25)) == [(2, 1.0)]            # inside one class: (hi - lo) / (hi - lo)
    assert one((True, 1.5), (True, 0.5), (True, 2.5)) == [(2, 1.0)]               # lo and hi on edges: the zero-width row 3 gets nothing
    assert one((True, 1.5), (True, 0.5)) == [(2, 1.0)]                            # [1, 1.5]
    assert one((True, 1.), (True, 0.), (True, 4.)) == [(1, 0.25), (2, 0.5), (3, 0.25)]      # [0.5, 2.5]
    assert one((True, 1.), (True, 4.), (True, 0.)) == [(1, 0.25), (2, 0.5), (3, 0.25)]      # the same, inverted in z
    assert one((True, 2.), (True, -6.), (True, 10.)) == [(0, 0.25), (1, 0.125), (2, 0.125), (3, 0.25), (4, 0.25)]   # [-2, 6]


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
    """the words of the class transport's refusals, in both forms: set_tracer first, then set_class_edges first, then the
    grid -- all decided before a device is needed"""
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
                assert (name + ': set_tracer first').encode() in lib.nf_last_error()
        assert lib.nf_field_set_uv(ctypes.byref(h), uv.ctypes.data, uv.ctypes.data, 3, NF_F64, 0, numpy.nan) == 0
        assert lib.nf_field_set_tracer(ctypes.byref(h), uv.ctypes.data, 3, NF_F64, 0, numpy.nan) == 0
        for name in CALLS:
            for carry in (0, 1):
                assert _compute(name, ctypes.byref(h), carry, rows) == NF_ERR_STATE, name
                assert (name + ': set_class_edges first').encode() in lib.nf_last_error()
        assert lib.nf_field_set_class_edges(ctypes.byref(h), _lib.dptr(edges), 3) == 0
        for name in CALLS:
            for carry in (0, 1):
                assert _compute(name, ctypes.byref(h), carry, rows) == NF_ERR_STATE, name
                assert b'set_bounds' in lib.nf_last_error() and name.encode() in lib.nf_last_error()
        assert not rows.any()
    finally:
        assert lib.nf_field_del(ctypes.byref(h)) == 0


# ---- Python ----------------------------------------------------------------------------------------------------------------
def test_python_method_checks_its_arguments():
    import inspect
    from nemoflux_amd.field import Field
    assert str(inspect.signature(Field.computeClassRemap)) == '(self, tIndex, carry=False, out=None, prefetch_next=None)'
    f = Field.__new__(Field)
    f.nt, f.nz, f.ny, f.nx = 2, 3, 4, 5
    f._lazy = None
    f._e3 = None
    with pytest.raises(RuntimeError, match='setClassEdges first'):
        f.computeClassRemap(0)
    f._class_edges = numpy.array([1., 2.])
    with pytest.raises(RuntimeError, match='out of range'):
        f.computeClassRemap(2)
    for carry in (False, True):
        with pytest.raises(RuntimeError, match='setTracer first'):
            f.computeClassRemap(0, carry=carry)
    # the rows go into the class-space helpers as they are
    rows = numpy.random.default_rng(4).standard_normal((6, 3))
    assert Field.classStreamfunction(rows).shape == (4, 3)


# ---- fluxplot --------------------------------------------------------------------------------------------------------------
def test_fluxplot_remap_options_are_checked():
    from nemoflux_amd.fluxplot import main
    files = dict(tFile='/nonexistent/T.nc', uFile='/nonexistent/U.nc', vFile='/nonexistent/V.nc', lonLatPoints='(0,0),(1,1)')
    with pytest.raises(RuntimeError, match="--remap must be 'linear'"):
        main(tracer='sigma0', classes='26,27', remap='cubic', **files)
    with pytest.raises(RuntimeError, match='--remap needs --classes'):
        main(tracer='sigma0', remap='linear', **files)
    with pytest.raises(RuntimeError, match='--remap needs --classes'):
        main(remap='linear', **files)
    for kw, opt in ((dict(tracer2='so', classes2='34,35'), '--classes2'), (dict(levels=True), '--levels'),
                    (dict(decompose=True), '--decompose'), (dict(eddy=True), '--eddy')):
        with pytest.raises(RuntimeError, match='--remap and ' + opt + ' cannot'):
            main(tracer='sigma0', classes='26,27', remap='linear', **kw, **files)
    with pytest.raises(RuntimeError, match='--cell-thickness cannot be combined with --classes'):
        main(tracer='sigma0', classes='26,27', remap='linear', cellThickness=True, **files)
    # accepted combinations go on to open the files
    for kw in (dict(tracer='sigma0'), dict(tracer='sigma0', sverdrup=True), dict(tracer='sigma0', carry='thetao', carryRef=1.5),
               dict(sigma='thetao,so'), dict(sigma='thetao,so', carry='thetao')):
        with pytest.raises(RuntimeError, match='no such file'):
            main(classes='26,27,28', remap='linear', **kw, **files)


def test_fluxplot_command_line_lists_remap():
    out = subprocess.run([sys.executable, '-m', 'nemoflux_amd.fluxplot', '--help'], cwd=ROOT, capture_output=True, text=True,
                         timeout=120)
    assert out.returncode == 0, out.stderr
    assert '--remap' in out.stdout
