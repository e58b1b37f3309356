"""Transports between surfaces (nf_field_compute_surface_transport, Field.computeSurfaceTransport, fluxplot --depth-surfaces),
the part that needs no GPU: the reference of tests/surface_transport_reference.py pinned to a naive scalar loop with math.fsum at
4 eps x sum |share| per value on the 12 x 9 x 3 case of the sibling tests, in both forms, with the scalar, a static and a
time-varying thickness, static and time-varying surfaces, `top` 0 and -1.5 and a rank's slab; the fractions of every spread term
add up to 1 within 4 eps; the fallbacks one by one; the conditions on the inputs of tests/test_gpu_surface_transport.py; the
argument and state errors of the five C calls, decided before a device is needed; the refusals of the Field methods and of the
fluxplot options."""
import ctypes
import math
import re
import subprocess
import sys

import numpy
import pytest

from conftest import ROOT
from depth_remap_reference import GPU_E3_SEED, GPU_TH, depth_thickness
from gross_reference import FILL, MISSING, THFILL, THMISSING, gross_velocities
from surface_transport_reference import (GPU_M, GPU_SURFACE_SEED, SFILL, SMISSING, SurfaceReference, gpu_case, shares,
                                         surface_fields, surface_values)
from test_class_remap_cpu import _tracer
from test_depth_remap_cpu import _gpu_weights
from test_gross_cpu import GPU_GRIDS, GPU_NT, GPU_NZ, GPU_UV_SEED, NT, NX, NY, NZ, REF, TFILL, TH, TMISSING, _weights

EPS = numpy.finfo(numpy.float64).eps
SV = 6371000.0 / 1.e6
NF_ERR_ARG, NF_ERR_STATE = 1, 2
NF_F64, NF_F32 = 0, 1
CALLS = ('nf_field_compute_surface_transport', 'nf_field_compute_surface_transport_async')
SET = 'nf_field_set_depth_surfaces'


def _small_surfaces(real, nt_s, m, seed):
    """surfaces for the 12 x 9 x 3 case, whose columns are at most 2.75 (scalar) or 12 (cell thickness) deep: multiples of 1/8
    in overlapping bands, both markers, NaN and both infinities scattered"""
    rng = numpy.random.default_rng(seed)
    dt = numpy.dtype(real).type
    shape = (nt_s, NY, NX)
    out = numpy.empty((nt_s, m, NY, NX), real)
    for k in range(m):
        a = (numpy.floor(8. * 0.75 * (4. / m) * k) / 8. + rng.integers(0, int(8 * 4 / m) + 1, shape) / 8.).astype(real)
        for mark in (SFILL, SMISSING, numpy.nan, numpy.inf, -numpy.inf):
            a[rng.random(shape) < 0.05 / math.sqrt(m)] = dt(mark)
        out[:, k] = a
    return out


def _naive(ce, w, sg, arc, tr_off, a, t, m, top, cell_thickness, levels, swrap):
    """the rows of both forms as math.fsum of their shares, one (entry, level, row) at a time from the full arrays; also the
    largest |sum of the fractions of a spread term - 1|"""
    dt = a['uo'].dtype.type
    nseg, ntr = int(tr_off[-1]), len(tr_off) - 1
    tr_of = [p for p in range(ntr) for _ in range(tr_off[p], tr_off[p + 1])]
    nz = a['uo'].shape[1]

    def present(x, marks):
        return not math.isnan(x) and all(x != dt(mk) for mk in marks)

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

    def fractions(e, d0, d1):
        """[(row, fraction or None for the whole term)]; e: the edges of the face, None without an edge set"""
        if e is None or not (math.isfinite(d0) and math.isfinite(d1) and math.isfinite(d1 - d0)):
            return [(m + 1, None)]
        row = lambda x: sum(1 for ed in e if ed <= x)   # noqa: E731
        lo, hi = min(d0, d1), max(d0, d1)
        if lo == hi:
            return [(row(lo), None)]
        out = []
        for j in range(row(lo), row(hi) + 1):
            left = lo if j == row(lo) else e[j - 1]
            right = hi if j == row(hi) else e[j]
            if right != left:
                out.append((j, (right - left) / (hi - lo)))
        return out

    terms = {'volume': {}, 'carried': {}}
    worst = 0.0
    for k in range(len(ce)):
        c, slot, s = int(ce[k]) // 4, int(ce[k]) % 4, int(sg[k])
        j, i = divmod(c, NX)
        if slot == 0:
            if j == 0:
                continue
            ca, cb, cbs = c - NX, c, c
        elif slot == 1:
            ca = c
            cb = c + 1 if i < NX - 1 else c + 1 - NX
            cbs = cb if (i < NX - 1 or swrap) else None
        elif slot == 2:
            ca, cb = c, (c + NX if j < NY - 1 else None)
            cbs = cb
        else:
            ca, cb = (c - 1 if i > 0 else c - 1 + NX), c
            cbs = cb if (i > 0 or swrap) else None
        # the edge set of the face: the running max of the surfaces' face values, or none
        e = []
        for q in range(m):
            has, x = face('surface', q, ca, cbs, (SFILL, SMISSING))
            if not has or not math.isfinite(x):
                e = None
                break
            e.append(x if not e else max(e[-1], x))
        east = slot in (1, 3)
        depth = float(top)
        for z in range(nz):
            if cell_thickness:
                h = val('e3u' if east else 'e3v', z, ca)
                h = float(h) if present(h, (THFILL, THMISSING)) else 0.0
            else:
                h = float(TH[z])
            d0, depth = depth, depth + h
            if not levels[0] <= z < levels[1]:
                continue
            x = val('uo' if east else 'vo', z, ca)
            vel = float(x) if present(x, (FILL, MISSING)) else 0.0
            has_t, xt = face('tracer', z, ca, cb, (TFILL, TMISSING))
            tf = xt - REF if has_t else 0.0
            al = float(arc[ca, 1]) if east else -float(arc[ca, 2])
            q_ = float(w[k]) * (((h * vel) * al) * SV)
            cc = float(w[k]) * (((h * (vel * tf)) * al) * SV)
            fr = fractions(e, d0, depth)
            if fr[0][1] is not None:
                worst = max(worst, abs(math.fsum(x for _, x in fr) - 1.0))
            for r, x in fr:
                for col in (s, nseg + tr_of[s]):
                    terms['volume'].setdefault((r, col), []).append(q_ if x is None else q_ * x)
                    terms['carried'].setdefault((r, col), []).append(cc if x is None else cc * x)
    out = {'fraction_error': worst}
    for nm in terms:
        want, mag = numpy.zeros((m + 2, nseg + ntr)), numpy.zeros((m + 2, nseg + ntr))
        for idx, xs in terms[nm].items():
            want[idx], mag[idx] = math.fsum(xs), math.fsum(abs(x) for x in xs)
        out[nm] = (want, mag)
    return out


@pytest.mark.parametrize('top,swrap', [(0.0, True), (-1.5, False)])
@pytest.mark.parametrize('thick', ['scalar', 'static', 'timevarying'])
@pytest.mark.parametrize('real', ['float64', 'float32'])
def test_reference_is_the_naive_loop(oracle, real, thick, top, swrap):
    ce, wt, sg, arc, tr_off = _weights(oracle)
    shape = (NT, NZ, NY, NX)
    u, v = gross_velocities(real, shape, seed=5)
    arrays = {'uo': u, 'vo': v, 'tracer': _tracer(real, shape, 7)}
    cell = thick != 'scalar'
    if cell:
        arrays['e3u'], arrays['e3v'] = depth_thickness(real, (NT if thick == 'timevarying' else 1, NZ, NY, NX), seed=9)
    kw = dict(uv_markers=(FILL, MISSING), tracer_markers=(TFILL, TMISSING), thick_markers=(THFILL, THMISSING), reference=REF,
              wrap=True, sverdrup=True, surface_markers=(SFILL, SMISSING), surface_wrap=swrap)
    ref = SurfaceReference(ce, wt, sg, arc, TH, tr_off, NX, NY, cell_thickness=cell, **kw)
    for m in (1, 3, 8):
        nt_s = NT if (m == 3) != (thick == 'static') else 1
        arrays['surface'] = _small_surfaces(real, nt_s, m, seed=20 + m)
        s = arrays['surface']
        dt = s.dtype.type
        assert numpy.isnan(s).any() and (s == dt(SFILL)).any() and (s == dt(SMISSING)).any() and numpy.isinf(s).any()
        seen = numpy.zeros(m + 2, bool)
        for t in range(NT):
            for levels in ((0, NZ), (1, NZ), (0, 2)):
                got = ref.surface_step(surface_values(arrays, t), m, top=top, levels=levels)
                want = _naive(ce, wt, sg, arc, tr_off, arrays, t, m, top, cell, levels, swrap)
                for nm in ('volume', 'carried'):
                    (g_, gm_), (w_, m_) = got[nm], want[nm]
                    assert g_.shape == w_.shape == gm_.shape == (m + 2, ref.row_length), nm
                    seen |= m_.max(axis=1) > 0
                    assert numpy.all(numpy.abs(g_ - w_) <= 4 * EPS * m_), (nm, m, t, levels)
                    assert numpy.all(numpy.abs(gm_ - m_) <= 4 * EPS * m_), (nm, m, t, levels)
                assert got['fraction_error'] <= 4 * EPS and want['fraction_error'] <= 4 * EPS
            got = ref.surface_step(surface_values(arrays, t), m, top=top)
            assert got['unbinned'] > 0 and (m != 3 or got['max_acted'] > 0) and got['spread_terms'] > 0
            # conservation: the rows add up to the profile rows of ResolvedReference under the same thickness
            step = ref.step(surface_values(arrays, t))
            for nm, key in (('volume', 'volume_profile'), ('carried', 'tracer_profile')):
                (g_, gm_), (w_, wm_) = got[nm], step[key]
                assert numpy.all(numpy.abs(g_.sum(axis=0) - w_.sum(axis=0)) <= 8 * EPS * wm_.sum(axis=0)), (nm, t)
                assert numpy.all(numpy.abs(gm_.sum(axis=0) - wm_.sum(axis=0)) <= 8 * EPS * wm_.sum(axis=0)), (nm, t)
        assert seen[0] and seen[-1] and seen.sum() >= min(m + 2, 4), (m, seen)
    only_volume = ref.surface_step(surface_values(arrays, 0), 8, top=top, tracer=False)
    assert 'carried' not in only_volume
    assert numpy.array_equal(only_volume['volume'][0], ref.surface_step(surface_values(arrays, 0), 8, top=top)['volume'][0])


def test_the_share_rule_with_an_edge_set_per_term():
    inf = numpy.inf
    E = numpy.array([[0., 1., 1.], [1., 1., 2.], [2., 3., 2.]])       # three terms, each with its own non-decreasing edges
    ent, row, frac = shares(numpy.array([True, True, True]), numpy.array([0.5, 0.5, 0.5]), numpy.array([2.5, 2.5, 2.5]), E)
    got = {(int(a), int(b)): float(c) for a, b, c in zip(ent, row, frac)}
    # term 0: edges 0, 1, 2 -> rows 1, 2, 3;  term 1: edges 1, 1, 3: row 1 has zero width and gets nothing;  term 2: 1, 2, 2
    assert got == {(0, 1): 0.25, (0, 2): 0.5, (0, 3): 0.25, (1, 0): 0.25, (1, 2): 0.75, (2, 0): 0.25, (2, 1): 0.5, (2, 3): 0.25}
    ent, row, frac = shares(numpy.array([False, True, True]), numpy.array([0., 1., 7.]), numpy.array([0., 1., inf]), E)
    # no edge set: row m + 1;  lo == hi on a double edge: the row below both;  (an infinite hi never reaches shares)
    assert list(zip(ent.tolist(), row.tolist()))[:2] == [(0, 4), (1, 2)] and frac[:2].tolist() == [1.0, 1.0]


def _one_face(surfaces, e3u, uo, top=0.0, neighbour=None, swrap=True):
    """the rows of ONE entry -- the east slot of cell 4 of a 3 x 3 grid, weight 1, arc 1 -- with the surfaces' values at the cell
    (`surfaces`) and at its east neighbour (`neighbour`, default: the same)"""
    nz, m = len(uo), len(surfaces)
    full = lambda col: numpy.repeat(numpy.asarray(col, dtype=numpy.float64)[None, :, None], 9, axis=2).reshape(1, -1, 3, 3)  # noqa: E731
    arrays = {'uo': full(uo), 'vo': full(uo), 'e3u': full(e3u), 'e3v': full(e3u), 'surface': full(surfaces)}
    if neighbour is not None:
        arrays['surface'][0, :, 1, 2] = neighbour
    ref = SurfaceReference([4 * 4 + 1], [1.0], [0], numpy.ones((9, 4)), numpy.ones(nz), [0, 1], 3, 3,
                           thick_markers=(THFILL, THMISSING), cell_thickness=True, surface_markers=(SFILL, SMISSING),
                           surface_wrap=swrap)
    with numpy.errstate(invalid='ignore'):
        out = ref.surface_step(surface_values(arrays, 0), m, top=top, tracer=False)
    return out['volume'][0][:, 0].tolist(), out


def test_the_fallbacks_one_by_one():
    inf, nan = numpy.inf, numpy.nan
    # two layers of thickness 2 under surfaces at 1 and 3: [0, 2] a half each to rows 0, 1; [2, 4] a half each to rows 1, 2
    rows, out = _one_face([1., 3.], [2., 2.], [1., 1.])
    assert rows == [1.0, 2.0, 1.0, 0.0] and out['spread_terms'] == 2 and out['unbinned'] == 0 and out['max_acted'] == 0
    # the face value is the mean of the two cells; one missing: the other one's
    assert _one_face([1., 3.], [2., 2.], [1., 1.], neighbour=[3., 3.])[0] == [2.0, 1.0, 1.0, 0.0]         # edges 2, 3
    assert _one_face([1., 3.], [2., 2.], [1., 1.], neighbour=[SFILL, nan])[0] == [1.0, 2.0, 1.0, 0.0]
    # a missing surface on both sides, or +-inf on one: every level of the face whole to row m + 1
    for bad in (SFILL, SMISSING, nan):
        rows, out = _one_face([1., bad], [2., 2.], [1., 1.])
        assert rows == [0.0, 0.0, 0.0, 4.0] and out['unbinned'] == 1
    for bad in (inf, -inf):
        assert _one_face([1., 3.], [2., 2.], [1., 1.], neighbour=[1., bad])[0] == [0.0, 0.0, 0.0, 4.0]
    assert _one_face([inf, 3.], [2., 2.], [1., 1.])[0] == [0.0, 0.0, 0.0, 4.0]
    # a surface above the previous one is taken at that one: edges 3, 3 -- row 1 has zero width and gets nothing
    rows, out = _one_face([3., 1.], [2., 2.], [1., 1.])
    assert rows == [3.0, 0.0, 1.0, 0.0] and out['max_acted'] == 1
    # x_k == D_z: the interface on an edge; the layer above stays above, the layer below goes below
    rows, out = _one_face([2.], [2., 2.], [1., 1.])
    assert rows == [2.0, 2.0, 0.0] and out['on_edge'] == 1 and out['spread_terms'] == 0
    # a single level
    assert _one_face([1., 3.], [4.], [2.])[0] == [2.0, 4.0, 2.0, 0.0]
    # a zero thickness: lo == hi, the term (+0) whole to row(lo) -- on an edge, the row below it
    rows, out = _one_face([2.], [2., 0., 1.], [1., 1., 1.])
    assert rows == [2.0, 1.0, 0.0] and out['flat_terms'] == 1
    # an infinite thickness: that level and every level below to row m + 1; `top` moves every interface
    rows, out = _one_face([2.], [1., inf, 1.], [1., 0.5, 1.])
    assert rows[:2] == [1.0, 0.0] and rows[2] == inf
    assert _one_face([1.], [2., 2.], [1., 1.], top=-1.0)[0] == [2.0, 2.0, 0.0]


@pytest.mark.parametrize('thick', ['scalar', 'timevarying'])
@pytest.mark.parametrize('grid', GPU_GRIDS, ids=lambda g: f'{g[0]}x{g[1]}')
@pytest.mark.parametrize('real', ['float64', 'float32'])
def test_generated_inputs_meet_the_conditions_of_the_gpu_tests(oracle, real, grid, thick):
    """over the entries of the three transects of the GPU tests: terms are spread over several rows, terms have lo == hi,
    interface depths lie exactly on an edge, the running max acts for every m >= 2, and at most a quarter of the faces of any
    case go to row m + 1"""
    nx, ny = grid
    ce, wt, sg, arc, tr_off = _gpu_weights(oracle, grid)
    shape = (GPU_NT, GPU_NZ, ny, nx)
    u, v = gross_velocities(real, shape, seed=GPU_UV_SEED)
    arrays = {'uo': u, 'vo': v}
    cell = thick != 'scalar'
    if cell:
        arrays['e3u'], arrays['e3v'] = depth_thickness(real, shape, seed=GPU_E3_SEED)
    ref = SurfaceReference(ce, wt, sg, arc, GPU_TH, tr_off, nx, ny, uv_markers=(FILL, MISSING),
                           thick_markers=(THFILL, THMISSING), cell_thickness=cell, surface_markers=(SFILL, SMISSING))
    for k, m in enumerate(GPU_M):
        acted = 0
        for nt_s in (1, GPU_NT):      # every m meets a static and a time-varying set on every grid (gpu_case)
            arrays['surface'] = surface_fields(real, (nt_s, ny, nx), m, GPU_SURFACE_SEED)
            x = arrays['surface']
            x = x[numpy.isfinite(x) & (x != x.dtype.type(SFILL)) & (x != x.dtype.type(SMISSING))].astype(numpy.float64)
            assert x.min() >= 0 and x.max() <= 24. and numpy.array_equal(8. * x, numpy.round(8. * x))
            t, top = gpu_case(k, 0)[1:3]
            got = ref.surface_step(surface_values(arrays, t), m, top=top, tracer=False)
            label = (m, nt_s, {q: got[q] for q in ('spread_terms', 'flat_terms', 'on_edge', 'max_acted', 'unbinned', 'faces')})
            assert got['spread_terms'] > 0 and got['on_edge'] > 0, label
            assert got['flat_terms'] > 0 or not cell, label              # a scalar thickness > 0 never stands still
            acted += got['max_acted']
            assert 0 < 4 * got['unbinned'] <= got['faces'], label
            assert got['fraction_error'] <= 4 * EPS
        assert acted > 0 or m < 2, m


# ---- C ABI -----------------------------------------------------------------------------------------------------------------
def _header():
    import os
    with open(os.path.join(ROOT, 'include', 'nemoflux_amd.h')) as fh:
        return re.sub(r'/\*.*?\*/', '', fh.read(), flags=re.S)


def test_header_declares_and_library_exports_the_five_calls():
    from nemoflux_amd import _lib
    header = _header()
    out = subprocess.run(['nm', '-D', '--defined-only', _lib._SO], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stderr
    exported = {ln.split()[-1] for ln in out.stdout.splitlines() if ln.split()}
    args = {CALLS[0]: 'nf_field **self, long tIndex, int carry, double *rows_host',
            CALLS[1]: 'nf_field **self, long tIndex, int carry, double *rows_dev',
            SET: 'nf_field **self, const void *const *surfaces, int m, long nt_s, int dtype, int on_device, double fill_value, '
                 'double top',
            SET + '_missing_value': 'nf_field **self, double missing_value',
            SET + '_wrap': 'nf_field **self, int wrap_x'}
    for name, want in args.items():
        mt = re.search(r'\bint\s+' + name + r'\s*\(([^)]*)\)\s*;', header)
        assert mt, f'{name} is not declared in include/nemoflux_amd.h'
        assert ' '.join(mt.group(1).split()) == want, name
        assert name in exported, name
        fn = getattr(_lib.lib, name)
        assert fn.restype is ctypes.c_int and len(fn.argtypes) == want.count(',') + 1, name
    assert _lib.lib.nf_version() == 100


def _compute(name, h, carry, out):
    from nemoflux_amd import _lib
    fn = getattr(_lib.lib, name)
    if out is None:
        return fn(h, 0, carry, None)
    return fn(h, 0, carry, ctypes.c_void_p(out.ctypes.data) if name.endswith('_async') else _lib.dptr(out))


def _ptrs(arrays):
    return (ctypes.c_void_p * len(arrays))(*[a.ctypes.data for a in arrays])


def test_set_depth_surfaces_checks_its_arguments():
    from nemoflux_amd import _lib
    lib = _lib.lib
    plane = numpy.zeros(16)
    one = _ptrs([plane])
    assert lib.nf_field_set_depth_surfaces(None, one, 1, 1, NF_F64, 0, numpy.nan, 0.0) == NF_ERR_ARG
    assert b'nf_field_set_depth_surfaces: null field' in lib.nf_last_error()
    for fn in (lib.nf_field_set_depth_surfaces_missing_value, lib.nf_field_set_depth_surfaces_wrap):
        assert fn(None, 1) == NF_ERR_ARG and b'null field' in lib.nf_last_error()
    h = ctypes.c_void_p()
    assert lib.nf_field_new(ctypes.byref(h)) == 0
    try:
        hp = ctypes.byref(h)
        rows = numpy.zeros(64)
        for m in (0, -1, 9):
            many = _ptrs([plane] * max(m, 1))
            assert lib.nf_field_set_depth_surfaces(hp, many, m, 1, NF_F64, 0, numpy.nan, 0.0) == NF_ERR_ARG, m
            assert b'nf_field_set_depth_surfaces: need 1 <= m <= 8 surfaces' in lib.nf_last_error()
        holes = (ctypes.c_void_p * 2)(plane.ctypes.data, None)
        assert lib.nf_field_set_depth_surfaces(hp, holes, 2, 1, NF_F64, 0, numpy.nan, 0.0) == NF_ERR_ARG
        assert b'nf_field_set_depth_surfaces: null argument' in lib.nf_last_error()
        assert lib.nf_field_set_depth_surfaces(hp, one, 1, 1, 7, 0, numpy.nan, 0.0) == NF_ERR_ARG
        assert b'dtype must be NF_F64/NF_F32' in lib.nf_last_error()
        for top in (numpy.nan, numpy.inf, -numpy.inf):
            assert lib.nf_field_set_depth_surfaces(hp, one, 1, 1, NF_F64, 0, numpy.nan, top) == NF_ERR_ARG
            assert b'nf_field_set_depth_surfaces: top must be a finite number' in lib.nf_last_error()
        for nt_s in (0, -2):
            assert lib.nf_field_set_depth_surfaces(hp, one, 1, nt_s, NF_F64, 0, numpy.nan, 0.0) == NF_ERR_ARG
            assert b'need nt_s = 1 (static) or the nt of uo/vo' in lib.nf_last_error()
        assert lib.nf_field_set_depth_surfaces(hp, one, 1, 1, NF_F64, 0, numpy.nan, 0.0) == NF_ERR_STATE
        assert b'nf_field_set_depth_surfaces: set_uv first' in lib.nf_last_error()
        assert lib.nf_field_set_uv(hp, plane.ctypes.data, plane.ctypes.data, 3, NF_F64, 0, numpy.nan) == 0
        assert lib.nf_field_set_depth_surfaces(hp, one, 1, 2, NF_F64, 0, numpy.nan, 0.0) == NF_ERR_ARG
        assert b'has nt = 2 time steps, need 1 (static) or the 3 of uo/vo' in lib.nf_last_error()
        assert lib.nf_field_set_depth_surfaces(hp, one, 1, 3, NF_F32, 0, numpy.nan, 0.0) == NF_ERR_ARG
        assert b"the depth surfaces's dtype is float32, uo/vo are float64" in lib.nf_last_error()
        # a static host set is uploaded at the call: that needs the grid
        assert lib.nf_field_set_depth_surfaces(hp, one, 1, 1, NF_F64, 0, numpy.nan, 0.0) == NF_ERR_STATE
        assert b'nf_field_set_depth_surfaces: set_bounds first' in lib.nf_last_error()
        # none of the refused calls set anything
        assert _compute(CALLS[0], hp, 0, rows) == NF_ERR_STATE
        assert b'set_depth_surfaces first' in lib.nf_last_error()
        # a time-varying host set and a device set are borrowed: no device needed; NULL clears
        assert lib.nf_field_set_depth_surfaces(hp, _ptrs([plane] * 8), 8, 3, NF_F64, 0, -999., -1.5) == 0
        assert lib.nf_field_set_depth_surfaces_missing_value(hp, 1e20) == 0 and lib.nf_field_set_depth_surfaces_wrap(hp, 0) == 0
        assert _compute(CALLS[0], hp, 0, rows) == NF_ERR_STATE and b'set_bounds' in lib.nf_last_error()
        assert lib.nf_field_set_depth_surfaces(hp, None, 0, 0, NF_F64, 0, numpy.nan, 0.0) == 0
        assert _compute(CALLS[0], hp, 0, rows) == NF_ERR_STATE and b'set_depth_surfaces first' in lib.nf_last_error()
        assert not rows.any()
    finally:
        assert lib.nf_field_del(ctypes.byref(h)) == 0


def test_argument_and_state_errors_of_the_two_computes():
    """null, carry, then set_depth_surfaces first, then (carry) set_tracer first, then the grid -- all before a device is needed"""
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
        hp = ctypes.byref(h)
        for name in CALLS:
            assert _compute(name, hp, 0, None) == NF_ERR_ARG, name
            assert b'null' in lib.nf_last_error() and name.encode() in lib.nf_last_error()
            for carry in (2, -1):
                assert _compute(name, hp, carry, rows) == NF_ERR_ARG, name
                assert b'carry must be 0 or 1' in lib.nf_last_error() and name.encode() in lib.nf_last_error()
            for carry in (0, 1):
                assert _compute(name, hp, carry, rows) == NF_ERR_STATE, name
                assert (name + ': set_depth_surfaces first').encode() in lib.nf_last_error()
        # the depth and class edges are other sets: the surface calls do not see them, and the depth calls not the surfaces
        assert lib.nf_field_set_class_edges(hp, _lib.dptr(edges), 3) == 0
        assert lib.nf_field_set_depth_edges(hp, _lib.dptr(edges), 3, 0.0) == 0
        for name in CALLS:
            assert _compute(name, hp, 0, rows) == NF_ERR_STATE, name
            assert (name + ': set_depth_surfaces first').encode() in lib.nf_last_error()
        assert lib.nf_field_set_uv(hp, uv.ctypes.data, uv.ctypes.data, 3, NF_F64, 0, numpy.nan) == 0
        assert lib.nf_field_set_depth_surfaces(hp, _ptrs([uv, uv]), 2, 3, NF_F64, 0, numpy.nan, 0.0) == 0
        for name in CALLS:
            assert _compute(name, hp, 1, rows) == NF_ERR_STATE, name
            assert (name + ': set_tracer first').encode() in lib.nf_last_error()
            assert _compute(name, hp, 0, rows) == NF_ERR_STATE, name            # the volume form needs no tracer
            assert b'set_bounds' in lib.nf_last_error() and name.encode() in lib.nf_last_error()
        assert lib.nf_field_set_tracer(hp, uv.ctypes.data, 3, NF_F64, 0, numpy.nan) == 0
        for name in CALLS:
            for carry in (0, 1):
                assert _compute(name, hp, carry, rows) == NF_ERR_STATE, name
                assert b'set_bounds' in lib.nf_last_error() and name.encode() in lib.nf_last_error()
        assert lib.nf_field_set_depth_surfaces(hp, None, 0, 0, NF_F64, 0, numpy.nan, 0.0) == 0
        fn = lib.nf_field_compute_depth_transport
        assert fn(hp, 0, 0, _lib.dptr(rows)) == NF_ERR_STATE and b'set_bounds' in lib.nf_last_error()
        assert not rows.any()
    finally:
        assert lib.nf_field_del(ctypes.byref(h)) == 0


# ---- Python ----------------------------------------------------------------------------------------------------------------
def test_python_methods_check_their_arguments():
    import inspect
    from nemoflux_amd import _lib
    from nemoflux_amd.field import Field
    assert str(inspect.signature(Field.computeSurfaceTransport)) == '(self, tIndex, carry=False, out=None, prefetch_next=None)'
    assert (str(inspect.signature(Field.setDepthSurfaces)) ==
            '(self, surfaces, top=0.0, fill_value=None, missing_value=None, wrapX=True)')
    assert Field._SPLIT_METHODS[-1] == 'computeSurfaceTransport' and Field._SPLIT_METHODS[0] == 'computeTracerFlux'
    f = Field.__new__(Field)
    f.nt, f.nz, f.ny, f.nx = 2, 3, 4, 5
    f._lazy = None
    f._e3 = None
    f._uv_code = _lib.NF_F32
    with pytest.raises(RuntimeError, match='setDepthSurfaces first'):
        f.computeSurfaceTransport(0)
    good = numpy.zeros((4, 5), numpy.float32)
    for bad in ([], [good] * 9):
        with pytest.raises(RuntimeError, match='a list of 1 to 8 surfaces'):
            f.setDepthSurfaces(bad)
    for top in (numpy.nan, numpy.inf):
        with pytest.raises(RuntimeError, match='top must be a finite number'):
            f.setDepthSurfaces([good], top=top)
    for shape in ((5, 4), (3, 4, 5), (2, 3, 4, 5), (5,)):
        with pytest.raises(RuntimeError, match='surface 1 has shape'):
            f.setDepthSurfaces([good, numpy.zeros(shape)])
    with pytest.raises(RuntimeError, match='all static or all per time step'):
        f.setDepthSurfaces([good, numpy.zeros((2, 4, 5))])
    with pytest.raises(RuntimeError, match='need a float array'):
        f.setDepthSurfaces([numpy.zeros((4, 5), numpy.int32)])
    with pytest.raises(RuntimeError, match='surface 0 is float64, uo/vo are float32'):
        f.setDepthSurfaces([_lib.DeviceArray(4096, (4, 5), numpy.float64)])
    with pytest.raises(RuntimeError, match='all be host arrays .* or all be device arrays'):
        f.setDepthSurfaces([good, _lib.DeviceArray(4096, (4, 5), numpy.float32)])
    assert getattr(f, '_surfaces', None) is None
    f._surfaces = dict(items=[good], buf=[None], step=-1)
    with pytest.raises(RuntimeError, match='out of range'):
        f.computeSurfaceTransport(2)
    with pytest.raises(RuntimeError, match='setTracer first'):
        f.computeSurfaceTransport(0, carry=True)
    # the rows go into the class-space helper as they are: the transport above every surface
    rows = numpy.random.default_rng(4).standard_normal((6, 3))
    assert numpy.array_equal(Field.classStreamfunction(rows), numpy.cumsum(rows[:4], axis=0))


# ---- fluxplot --------------------------------------------------------------------------------------------------------------
def test_fluxplot_depth_surfaces_options_are_checked():
    from nemoflux_amd.fluxplot import main
    files = dict(tFile='/nonexistent/T.nc', uFile='/nonexistent/U.nc', vFile='/nonexistent/V.nc', lonLatPoints='(0,0),(1,1)')
    for text in ('a,,b', ',', 'a,b,c,d,e,f,g,h,i'):
        with pytest.raises(RuntimeError, match='--depth-surfaces must be NAME'):
            main(depthSurfaces=text, **files)
    with pytest.raises(RuntimeError, match='--surface-file needs --depth-surfaces'):
        main(surfaceFile='x.nc', **files)
    with pytest.raises(RuntimeError, match='--depth-top needs --depth-bins'):
        main(depthTop=2.0, **files)
    with pytest.raises(RuntimeError, match='--depth-top must be a finite number'):
        main(depthSurfaces='mld', depthTop=numpy.inf, **files)
    for kw, opt in ((dict(depthBins='0,100'), '--depth-bins'), (dict(tracer='sigma0', classes='26,27'), '--classes'),
                    (dict(classes2='34,35'), '--classes2'), (dict(grossClasses='26,27'), '--gross-classes'),
                    (dict(classArea='26,27'), '--class-area'), (dict(crossings='x.npz'), '--crossings'),
                    (dict(gross=True), '--gross'), (dict(levels=True), '--levels'), (dict(decompose=True), '--decompose'),
                    (dict(eddy=True), '--eddy'), (dict(show=True), '--show'), (dict(carry='thetao'), '--carry'),
                    (dict(sigma='thetao,so'), '--sigma'), (dict(zrange='0,100'), '--zrange'), (dict(remap='linear'), '--remap'),
                    (dict(thicknessWeighted=True), '--thickness-weighted')):
        with pytest.raises(RuntimeError, match='--depth-surfaces and ' + opt + ' cannot be combined'):
            main(depthSurfaces='mld,iso20', **kw, **files)
    with pytest.raises(RuntimeError, match='--tracer-ref / --tracer-scale need --tracer'):
        main(depthSurfaces='mld', tracerRef=1.0, **files)
    with pytest.raises(RuntimeError, match='need --cell-thickness'):
        main(depthSurfaces='mld', e3u='e3u_0', **files)
    # accepted combinations go on to open the files
    for kw in (dict(), dict(sverdrup=True), dict(depthTop=-1.5), dict(surfaceFile='/nonexistent/S.nc'),
               dict(tracer='thetao', tracerRef=1.5, tracerScale=4.1e-3), dict(cellThickness=True)):
        with pytest.raises(RuntimeError, match='no such file'):
            main(depthSurfaces='mld,iso20,bottom200', **kw, **files)


def test_fluxplot_command_line_lists_depth_surfaces():
    out = subprocess.run([sys.executable, '-m', 'nemoflux_amd.fluxplot', '--help'], cwd=ROOT, capture_output=True, text=True,
                         timeout=120)
    assert out.returncode == 0, out.stderr
    assert '--depth-surfaces' in out.stdout and '--surface-file' in out.stdout
