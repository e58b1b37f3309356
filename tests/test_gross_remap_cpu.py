"""Remapped gross class transports (nf_field_compute_gross_class_remap, Field.computeGrossClassRemap, fluxplot --gross-remap
linear), the part that needs no GPU: the reference of tests/gross_remap_reference.py pinned to a naive scalar loop with math.fsum
at 4 eps x sum |share| per value, on a 12 x 9 x 3 case with land, both markers and NaN in the velocities, both tracers and the
thickness, +-inf in a class field of its own, zero thicknesses and values on class edges, in every form (volume, carried tracer
that is the class field, carried tracer with a class field of its own; scalar, static and time-varying thickness) and with a single
level; the fractions of every spread term add up to 1 within 4 eps; the fallbacks one by one; the branches that the inputs of
tests/test_gpu_gross_remap.py take; the two calls declared, exported and bound, and the errors they decide before they need a
device; the Field method; the fluxplot argument checks."""
import ctypes
import math
import os
import re
import subprocess
import sys

import numpy
import pytest

from class_remap_reference import face_intervals, shares
from conftest import ROOT
from depth_remap_reference import GPU_E3_SEED as GPU_DEPTH_E3_SEED, depth_thickness
from gross_class_reference import GrossClassReference
from gross_reference import FILL, MIN_ABS_Q, MISSING, THFILL, THMISSING, array_values, gross_thickness, gross_velocities
from gross_remap_reference import GPU_EDGES, GPU_LINES, SFILL, SMISSING, GrossRemapReference, remap_lattice
from test_depth_remap_cpu import GPU_LINES as DEPTH_GPU_LINES, _gpu_weights
from test_gross_cpu import GPU_GRIDS, GPU_NT, GPU_NZ, GPU_UV_SEED, LINES, NT, NX, NY, NZ, REF, TFILL, TH, TMISSING, _weights  # noqa: F401

EPS = numpy.finfo(numpy.float64).eps
NF_ERR_ARG, NF_ERR_STATE = 1, 2
NF_F64 = 0
CALLS = ('nf_field_compute_gross_class_remap', 'nf_field_compute_gross_class_remap_async')
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
    x[:, :, ::3, ::4] = x[:, :1, ::3, ::4]
    x[rng.random(shape) < 0.05] = dt(EDGES[2])
    for m in marks + (numpy.nan,) + ((numpy.inf, -numpy.inf) if inf else ()):
        x[rng.random(shape) < 0.04] = dt(m)
    return x


def _tracer(real, shape, seed):
    rng = numpy.random.default_rng(seed)
    dt = numpy.dtype(real).type
    tau = (REF + 2. * rng.standard_normal(shape)).astype(real)
    for m in (TFILL, TMISSING, numpy.nan):
        tau[rng.random(shape) < 0.05] = dt(m)
    return tau


def _naive(ce, w, sg, arc, tr_off, a, t, edges, class_marks, nz, cell):
    """P and N of both forms as math.fsum of their shares, one (entry, level, row) at a time from the full arrays; also the
    largest |sum of the fractions of a spread term - 1| and how many terms had q == 0"""
    dt = a['uo'].dtype.type
    nseg, ntr = int(tr_off[-1]), len(tr_off) - 1
    tr_of = [p for p in range(ntr) for _ in range(tr_off[p], tr_off[p + 1])]
    n = len(edges)

    def present(x, marks):
        return not math.isnan(x) and all(x != dt(m) for m in marks)

    def val(name, z, c):
        arr = a[name]
        return arr[t if arr.shape[0] > 1 else 0, z].reshape(-1)[c]

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
    worst, still = 0.0, 0
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
            if cell:
                h = val('e3u' if east else 'e3v', z, ca)
                h = float(h) if present(h, (THFILL, THMISSING)) else 0.0
            else:
                h = float(TH[z])
            has_t, xt = face('tracer', z, ca, cb, (TFILL, TMISSING))
            tf = xt - REF if has_t else 0.0
            al = float(arc[ca, 1]) if east else -float(arc[ca, 2])
            q = float(w[e]) * (((h * vel) * al) * SV)
            cc = float(w[e]) * (((h * (vel * tf)) * al) * SV)
            if q == 0.0:
                still += 1
                continue
            part = 0 if q > 0 else 1
            fr = fractions(z, ca, cb)
            if fr[0][1] is not None:
                worst = max(worst, abs(math.fsum(x for _, x in fr) - 1.0))
            for r, x in fr:
                for col in (s, nseg + tr_of[s]):
                    terms['volume'].setdefault((part, r, col), []).append(q if x is None else q * x)
                    terms['carried'].setdefault((part, r, col), []).append(cc if x is None else cc * x)
    out = {'fraction_error': worst, 'still': still}
    for nm in terms:
        want, mag = numpy.zeros((2, n + 2, nseg + ntr)), numpy.zeros((2, n + 2, nseg + ntr))
        for idx, xs in terms[nm].items():
            want[idx], mag[idx] = math.fsum(xs), math.fsum(abs(x) for x in xs)
        out[nm] = (want, mag)
    return out


@pytest.mark.parametrize('nz', [NZ, 1], ids=['three-levels', 'one-level'])
@pytest.mark.parametrize('thick', ['scalar', 'static', 'timevarying'])
@pytest.mark.parametrize('own_class', [False, True], ids=['one-tracer', 'class-tracer'])
@pytest.mark.parametrize('real', ['float64', 'float32'])
def test_reference_is_the_naive_loop(oracle, real, own_class, thick, nz):
    ce, wt, sg, arc, tr_off = _weights(oracle)
    shape = (NT, nz, NY, NX)
    dt = numpy.dtype(real).type
    u, v = gross_velocities(real, (NT, NZ, NY, NX), seed=5)
    arrays = {'uo': u[:, :nz], 'vo': v[:, :nz]}
    assert numpy.isnan(u).any() and (u == dt(FILL)).any() and (v == dt(MISSING)).any()
    if own_class:
        arrays['tracer'], arrays['class'], marks = _tracer(real, shape, 7), _lattice(real, shape, 13, (SFILL, SMISSING)), (SFILL, SMISSING)
    else:
        arrays['tracer'] = arrays['class'] = _lattice(real, shape, 13, (TFILL, TMISSING), inf=False)
        marks = (TFILL, TMISSING)
    cls, tau = arrays['class'], arrays['tracer']
    assert numpy.isnan(cls).any() and (cls == EDGES[2]).any() and (cls == dt(marks[0])).any() and (cls == dt(marks[1])).any()
    assert numpy.isnan(tau).any() and (tau == dt(TFILL)).any() and (tau == dt(TMISSING)).any()
    assert not own_class or (numpy.isposinf(cls).any() and numpy.isneginf(cls).any())
    cell = thick != 'scalar'
    if cell:
        e3 = gross_thickness(real, (NT if thick == 'timevarying' else 1, NZ, NY, NX), seed=9)
        arrays['e3u'], arrays['e3v'] = e3[0][:, :nz], e3[1][:, :nz]
        for a in e3:
            assert numpy.isnan(a).any() and (a == 0).any() and (a == dt(THFILL)).any() and (a == dt(THMISSING)).any()
    kw = dict(uv_markers=(FILL, MISSING), tracer_markers=(TFILL, TMISSING), thick_markers=(THFILL, THMISSING), reference=REF,
              wrap=True, sverdrup=True, cell_thickness=cell)
    ref = GrossRemapReference(ce, wt, sg, arc, TH[:nz], tr_off, NX, NY, class_markers=marks, **kw)
    step = GrossClassReference(ce, wt, sg, arc, TH[:nz], tr_off, NX, NY, class_markers=marks, **kw)
    seen = numpy.zeros((2, EDGES.size + 2), bool)
    for t in range(NT):
        got = ref.gross_remap_step(array_values(arrays, t), EDGES)
        want = _naive(ce, wt, sg, arc, tr_off, arrays, t, EDGES, marks, nz, cell)
        assert want['still'] > 0                                             # q == 0: in neither part
        for nm in ('volume', 'carried'):
            (g_, gm_), (w_, m_) = got[nm], want[nm]
            assert g_.shape == w_.shape == gm_.shape == (2, EDGES.size + 2, ref.row_length), nm
            seen |= m_.max(axis=2) > 0
            assert numpy.all(numpy.abs(g_ - w_) <= 4 * EPS * m_), (nm, t)
            assert numpy.all(numpy.abs(gm_ - m_) <= 4 * EPS * m_), (nm, t)
        vol = got['volume'][0]
        assert numpy.all(vol[0] >= 0) and numpy.all(vol[1] <= 0) and vol[0].max() > 0 and vol[1].min() < 0
        assert got['fraction_error'] <= 4 * EPS and want['fraction_error'] <= 4 * EPS
        assert MIN_ABS_Q <= got['min_abs_q'] < numpy.inf
        if nz == 1:
            assert got['spread_terms'] == 0                                  # one level: no interfaces, the step rule
        else:
            assert got['spread_terms'] > 50
        # conservation: over the rows the parts are those of the step rule; with a single level they are its rows
        flat = step.gross_class_step(array_values(arrays, t), EDGES)
        assert flat['min_abs_q'] == got['min_abs_q']
        for nm in ('volume', 'carried'):
            (g_, gm_), (w_, wm_) = got[nm], flat[nm]
            assert numpy.all(numpy.abs(g_.sum(axis=1) - w_.sum(axis=1)) <= 8 * EPS * wm_.sum(axis=1)), (nm, t)
            assert numpy.all(numpy.abs(gm_.sum(axis=1) - wm_.sum(axis=1)) <= 8 * EPS * wm_.sum(axis=1)), (nm, t)
            if nz == 1:
                assert numpy.array_equal(g_, w_) and numpy.array_equal(gm_, wm_), (nm, t)
    assert seen.any(axis=0).all() or nz == 1, 'every row, the one of the faces without a class value included, has terms'
    assert (seen[0].sum() > 5 and seen[1].sum() > 5) or nz == 1
    only_volume = ref.gross_remap_step(array_values(arrays, 0), EDGES, tracer=False, threads=2)
    assert 'carried' not in only_volume
    assert numpy.allclose(only_volume['volume'][0], ref.gross_remap_step(array_values(arrays, 0), EDGES)['volume'][0],
                          rtol=4 * EPS, atol=0)


def test_the_fallbacks_one_by_one():
    """the row rule is class_remap_reference's, used unchanged: the cases that matter here, and lo == hi"""
    e = numpy.array([0., 1., 2., 4.])
    n, inf, nan = e.size, numpy.inf, numpy.nan

    def one(cur, up=None, dn=None):
        wrap = lambda p: None if p is None else (numpy.array([p[0]]), numpy.array([float(p[1])]))   # noqa: E731
        ent, row, frac = shares(*face_intervals(wrap(cur), wrap(up), wrap(dn)), e)
        assert not ent.any()
        return list(zip(row.tolist(), frac.tolist()))

    assert one((False, 1.5), (True, 0.5), (True, 2.5)) == [(n + 1, 1.0)]          # no class value (a marker or NaN on both sides)
    assert one((True, nan), (True, 0.5), (True, 2.5)) == [(n + 1, 1.0)]           # NaN (+inf beside -inf)
    assert one((True, 1.5)) == [(2, 1.0)]                                         # a single level: the step rule
    assert one((True, 1.5), (False, 9.), (False, -9.)) == [(2, 1.0)]              # markers above and below
    assert one((True, 1.5), (True, inf), (True, 2.5)) == [(2, 1.0)]               # +inf in the class field above
    assert one((True, 1.5), (True, 0.5), (True, -inf)) == [(2, 1.0)]              # -inf below
    assert one((True, inf), (True, 1.), (True, 2.)) == [(n, 1.0)]
    assert one((True, -inf), (True, 1.), (True, 2.)) == [(0, 1.0)]
    assert one((True, 1.5), (True, 1.5), (True, 1.5)) == [(2, 1.0)]               # lo == hi
    assert one((True, 1.), (True, 1.), (True, 1.)) == [(2, 1.0)]                  # ... on an edge: the class above
    assert one((True, 1.), (True, 0.), (True, 4.)) == [(1, 0.25), (2, 0.5), (3, 0.25)]      # [0.5, 2.5]


def _one_face(uo, cls, tau, th, edges, e3=None):
    """one east entry of weight 1 on a 2 x 1 grid, nz = len(uo): P and N of both forms"""
    nz = len(uo)
    col = lambda x: numpy.array(x, dtype=numpy.float64).reshape(1, nz, 1, 1).repeat(2, axis=3)   # noqa: E731
    arrays = {'uo': col(uo), 'vo': col([0.] * nz), 'class': col(cls), 'tracer': col(tau)}
    if e3 is not None:
        arrays['e3u'] = arrays['e3v'] = col(e3)
    arc = numpy.ones((2, 4))
    ref = GrossRemapReference([1], [1.0], [0], arc, numpy.array(th, dtype=numpy.float64), [0, 1], 2, 1, uv_markers=(FILL, MISSING),
                              tracer_markers=(TFILL, TMISSING), class_markers=(SFILL, SMISSING), thick_markers=(THFILL, THMISSING),
                              reference=1.0, cell_thickness=e3 is not None)
    out = ref.gross_remap_step(array_values(arrays, 0), numpy.asarray(edges, dtype=numpy.float64))
    return out['volume'][0][:, :, 0], out['carried'][0][:, :, 0], out


def test_the_sign_of_the_water_picks_the_part_and_a_zero_thickness_neither():
    e = [0., 1., 2., 4.]
    # two levels, class values 1 and 3: level 0 has [1, 2] -> row 2 whole; level 1 has [2, 3] -> row 3 whole
    vol, car, out = _one_face([2., -4.], [1., 3.], [3., 3.], [0.5, 0.25], e)
    assert vol[0].tolist() == [0., 0., 1., 0., 0., 0.] and vol[1].tolist() == [0., 0., 0., -1., 0., 0.]
    assert car[0].tolist() == [0., 0., 2., 0., 0., 0.] and car[1].tolist() == [0., 0., 0., -2., 0., 0.]    # tf = 3 - 1
    # the carried term's own sign does not matter: tau below the reference goes where the water goes
    vol, car, out = _one_face([2., -4.], [1., 3.], [0., 0.], [0.5, 0.25], e)
    assert car[0].tolist() == [0., 0., -1., 0., 0., 0.] and car[1].tolist() == [0., 0., 0., 1., 0., 0.]
    # a spread term: class values 0.5, 3 -> level 0 [0.5, 1.75]: 0.4 to row 1, 0.6 to row 2
    vol, car, out = _one_face([-2., 0.], [0.5, 3.], [2., 2.], [1.0, 1.0], e)
    assert numpy.allclose(vol[1], [0., -0.8, -1.2, 0., 0., 0.], rtol=4 * EPS, atol=0) and not vol[0].any()
    assert out['spread_terms'] == 1 and out['min_abs_q'] == 2.0
    # a zero / missing / NaN thickness: q == 0, in neither part; so with a missing or NaN velocity
    for h in (0.0, THFILL, THMISSING, numpy.nan):
        vol, car, out = _one_face([2., -4.], [1., 3.], [3., 3.], [0.5, 0.25], e, e3=[h, 0.25])
        assert not vol[0].any() and vol[1].tolist() == [0., 0., 0., -1., 0., 0.] and not car[0].any()
    for x in (FILL, MISSING, numpy.nan, 0.0):
        vol, car, out = _one_face([x, -4.], [1., 3.], [3., 3.], [0.5, 0.25], e)
        assert not vol[0].any() and vol[1].tolist() == [0., 0., 0., -1., 0., 0.] and not car[0].any()
    # a face without a carried value carries 0 where the water goes; without a class value the term goes to row n + 1
    vol, car, out = _one_face([2., -4.], [1., 3.], [TFILL, numpy.nan], [0.5, 0.25], e)
    assert vol[0][2] == 1.0 and not car.any()
    vol, car, out = _one_face([2., -4.], [SFILL, numpy.nan], [3., 3.], [0.5, 0.25], e)
    assert vol[0].tolist() == [0., 0., 0., 0., 0., 1.] and vol[1].tolist() == [0., 0., 0., 0., 0., -1.]
    # a single level
    vol, car, out = _one_face([2.], [1.5], [3.], [0.5], e)
    assert vol[0].tolist() == [0., 0., 1., 0., 0., 0.] and not vol[1].any() and out['spread_terms'] == 0


# ---- the inputs of the GPU tests -----------------------------------------------------------------------------------------
@pytest.mark.parametrize('own', [False, True], ids=['one-tracer', 'class-tracer'])
@pytest.mark.parametrize('grid', GPU_GRIDS, ids=lambda g: f'{g[0]}x{g[1]}')
@pytest.mark.parametrize('real', ['float64', 'float32'])
def test_generated_inputs_take_every_branch(oracle, real, grid, own):
    """conditions on the inputs of tests/test_gpu_gross_remap.py, checked without a GPU: with its lattice, thickness lattice
    and edge sets terms are spread over several rows, terms have lo == hi, interface values are exactly an edge, every segment
    of every transect has water of both signs, and no |q| is near underflow"""
    assert GPU_LINES == DEPTH_GPU_LINES
    nx, ny = grid
    ce, wt, sg, arc, tr_off = _gpu_weights(oracle, grid)
    shape = (GPU_NT, GPU_NZ, ny, nx)
    u, v = gross_velocities(real, shape, seed=GPU_UV_SEED)
    lat = remap_lattice(real, shape, own, (TFILL_GPU, TMISSING_GPU))
    marks = (SFILL, SMISSING) if own else (TFILL_GPU, TMISSING_GPU)
    arrays = {'uo': u, 'vo': v, 'class': lat}
    arrays['e3u'], arrays['e3v'] = depth_thickness(real, shape, seed=GPU_DEPTH_E3_SEED)
    ref = GrossRemapReference(ce, wt, sg, arc, numpy.ones(GPU_NZ), tr_off, nx, ny, uv_markers=(FILL, MISSING),
                              class_markers=marks, thick_markers=(THFILL, THMISSING), cell_thickness=True)
    for n, edges in GPU_EDGES.items():
        got = ref.gross_remap_step(array_values(arrays, n % GPU_NT), edges, tracer=False)
        assert got['spread_terms'] > 100 and got['flat_terms'] > 0, n
        assert got['on_edge'] > 0 or 16. not in edges, n                     # the lattice puts 16 on a twentieth of the cells
        assert got['fraction_error'] <= 4 * EPS
        assert got['min_abs_q'] >= MIN_ABS_Q
        signs = got['signs']
        for p in range(len(tr_off) - 1):
            assert signs[0, tr_off[p]:tr_off[p + 1]].any() and signs[1, tr_off[p]:tr_off[p + 1]].any(), (n, p)
        P, N = got['volume'][0]
        assert P[:, int(tr_off[-1]):].max(axis=0).min() > 0 and N[:, int(tr_off[-1]):].min(axis=0).max() < 0


TFILL_GPU, TMISSING_GPU = -32768., 12345.    # the tracer markers of tests/test_gpu_cellthick.py (asserted equal on the GPU side)


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
    """the words of the gross class transport's refusals, in both forms: null, carry, set_tracer first, set_class_edges first,
    then the grid -- all decided before a device is needed"""
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
    assert (str(inspect.signature(Field.computeGrossClassRemap)) == str(inspect.signature(Field.computeGrossClassTransport))
            == '(self, tIndex, carry=False, out=None, prefetch_next=None)')
    assert 'computeGrossClassRemap' in Field._SPLIT_METHODS and 'computeGrossClassRemap' in Field.meanEddySplit.__doc__
    f = Field.__new__(Field)
    f.nt, f.nz, f.ny, f.nx = 2, 3, 4, 5
    f._lazy = None
    f._e3 = None
    with pytest.raises(RuntimeError, match='setClassEdges first'):
        f.computeGrossClassRemap(0)
    f._class_edges = numpy.array([1., 2.])
    with pytest.raises(RuntimeError, match='out of range'):
        f.computeGrossClassRemap(2)
    for carry in (False, True):
        with pytest.raises(RuntimeError, match='setTracer first'):
            f.computeGrossClassRemap(0, carry=carry)
    with pytest.raises(RuntimeError, match='method must be one of computeTracerFlux.*computeGrossClassRemap'):
        f.meanEddySplit('computeGrossRemap')
    # the parts go into the helpers as they are
    parts = numpy.random.default_rng(4).standard_normal((2, 6, 3))
    assert Field.grossTransport(parts).shape == (2, 3)
    assert Field.classStreamfunction(parts[0] + parts[1]).shape == (4, 3)


# ---- fluxplot --------------------------------------------------------------------------------------------------------------
def test_fluxplot_gross_remap_options_are_checked():
    from nemoflux_amd.fluxplot import grossRemapSeries, main  # noqa: F401
    files = dict(tFile='/nonexistent/T.nc', uFile='/nonexistent/U.nc', vFile='/nonexistent/V.nc', lonLatPoints='(0,0),(1,1)')
    with pytest.raises(RuntimeError, match='--gross-remap needs --gross-classes'):
        main(tracer='sigma0', grossRemap='linear', **files)
    with pytest.raises(RuntimeError, match='--gross-remap needs --gross-classes'):
        main(grossRemap='linear', **files)
    with pytest.raises(RuntimeError, match="--gross-remap must be 'linear'"):
        main(tracer='sigma0', grossClasses='26,27', grossRemap='cubic', **files)
    with pytest.raises(RuntimeError, match='--gross-remap and --classes cannot be combined'):
        main(tracer='sigma0', classes='26,27', grossRemap='linear', **files)
    with pytest.raises(RuntimeError, match='cannot be combined'):
        main(tracer='sigma0', classes='26,27', grossClasses='26,27', grossRemap='linear', **files)
    # --remap keeps its own checks
    with pytest.raises(RuntimeError, match='--remap needs --classes'):
        main(tracer='sigma0', grossClasses='26,27', remap='linear', **files)
    with pytest.raises(RuntimeError, match='--cell-thickness cannot be combined with --classes'):
        main(tracer='sigma0', classes='26,27', remap='linear', cellThickness=True, **files)
    # accepted combinations go on to open the files
    for kw in (dict(tracer='sigma0'), dict(tracer='sigma0', sverdrup=True), dict(tracer='sigma0', carry='thetao', carryRef=1.5),
               dict(tracer='sigma0', cellThickness=True), dict(tracer='sigma0', carry='thetao', cellThickness=True),
               dict(sigma='thetao,so'), dict(sigma='thetao,so', carry='thetao', cellThickness=True)):
        with pytest.raises(RuntimeError, match='no such file'):
            main(grossClasses='26,27,28', grossRemap='linear', **kw, **files)


def test_fluxplot_command_line_lists_gross_remap():
    out = subprocess.run([sys.executable, '-m', 'nemoflux_amd.fluxplot', '--help'], cwd=ROOT, capture_output=True, text=True,
                         timeout=120)
    assert out.returncode == 0, out.stderr
    assert '--gross-remap' in out.stdout
