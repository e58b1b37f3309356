"""Section area and area-weighted tracer (nf_field_compute_area_profile, Field.computeAreaProfile, Field.overturningGyre,
fluxplot --decompose), the part that needs no GPU: the reference of tests/section_reference.py pinned to a naive loop with
math.fsum on two tiny grids; the two calls declared, exported and bound, and the errors they decide before they need a device;
overturningGyre against a plain Python loop; the fluxplot argument checks; the closed form of a zonal line's area from the
weights alone."""
import ctypes
import math
import os
import re
import subprocess
import sys

import numpy
import pytest

from conftest import ROOT, transect_xyz
from section_reference import SectionReference, array_values
from test_resolved_reference_cpu import CFILL, CMISSING, FILL, GRIDS, MISSING, NT, NZ, REF, _arrays

EPS = numpy.finfo(numpy.float64).eps
NF_ERR_ARG, NF_ERR_STATE, NF_ERR_NO_DEVICE = 1, 2, 4
NF_F64 = 0
THFILL, THMISSING = -1.e30, 9.e9
CALLS = ('nf_field_compute_area_profile', 'nf_field_compute_area_profile_async')


# ---- the reference against a naive loop ------------------------------------------------------------------------------------
def _naive(ce, w, sg, arc, th, tr_off, nx, ny, a, t, wrap, cell_thickness):
    """A(z) and T(z) as math.fsum of their terms, one (entry, level) at a time from the full arrays"""
    dt = a['uo'].dtype.type
    nseg, ntr = int(tr_off[-1]), len(tr_off) - 1
    tr_of = [p for p in range(ntr) for _ in range(tr_off[p], tr_off[p + 1])]

    def present(x, marks):
        return not math.isnan(x) and all(x != dt(m) for m in marks)

    def val(name, tt, z, c):
        return a[name][tt, z].reshape(-1)[c]

    terms = {'area_profile': {}, 'tracer_area_profile': {}}
    for e in range(len(ce)):
        c, slot, s = int(ce[e]) // 4, int(ce[e]) % 4, int(sg[e])
        j, i = divmod(c, nx)
        if slot == 0:
            if j == 0:
                continue
            ca, cb = c - nx, c
        elif slot == 1:
            ca, cb = c, (c + 1 if i < nx - 1 else (c + 1 - nx if wrap else None))
        elif slot == 2:
            ca, cb = c, (c + nx if j < ny - 1 else None)
        else:
            ca = c - 1 if i > 0 else c - 1 + nx
            cb = c if (i > 0 or wrap) else None
        east = slot in (1, 3)
        for z in range(NZ):
            alpha = beta = 0.0
            xa = val('tracer', t, z, ca)
            pa = present(xa, (CFILL, CMISSING))
            pb = cb is not None and present(val('tracer', t, z, cb), (CFILL, CMISSING))
            x = None
            if pa and pb:
                x = 0.5 * (float(xa) + float(val('tracer', t, z, cb)))
            elif pa:
                x = float(xa)
            elif pb:
                x = float(val('tracer', t, z, cb))
            if present(val('uo' if east else 'vo', t, z, ca), (FILL, MISSING)) and x is not None and math.isfinite(x):
                if cell_thickness:
                    tt = t if a['e3u'].shape[0] > 1 else 0
                    h = val('e3u' if east else 'e3v', tt, z, ca)
                    h = float(h) if present(h, (THFILL, THMISSING)) else 0.0
                else:
                    h = float(th[z])
                alpha = abs(float(w[e])) * (h * float(arc[ca, 1 if east else 2]))
                beta = alpha * (x - REF)
            for col in (s, nseg + tr_of[s]):
                terms['area_profile'].setdefault((z, col), []).append(alpha)
                terms['tracer_area_profile'].setdefault((z, col), []).append(beta)
    out = {}
    for nm in terms:
        want, mag = numpy.zeros((NZ, nseg + ntr)), numpy.zeros((NZ, nseg + ntr))
        for idx, xs in terms[nm].items():
            want[idx], mag[idx] = math.fsum(xs), math.fsum(abs(x) for x in xs)
        out[nm] = (want, mag)
    return out


@pytest.mark.parametrize('thick', ['scalar', 'static', 'timevarying'])
@pytest.mark.parametrize('grid', sorted(GRIDS))
@pytest.mark.parametrize('real', ['float64', 'float32'])
def test_section_reference_is_the_naive_loop(oracle, real, grid, thick):
    g = GRIDS[grid]
    nx, ny = g['nx'], g['ny']
    o = oracle.DataGen(nx, ny, NZ, NT, *g['box'], lat_uses_dx=False)
    pts = oracle.assemble_points(o.bounds_lon, o.bounds_lat)
    arc = oracle.arc_lengths(pts)
    ws = [oracle.polyline_weights(pts, transect_xyz(s), periodX=g['periodX']) for s in g['lines']]
    tr_off = numpy.concatenate([[0], numpy.cumsum([w.nseg for w in ws])])
    ce = numpy.concatenate([w.cell_edge for w in ws])
    wt = numpy.concatenate([w.weight for w in ws])
    sg = numpy.concatenate([w.seg + tr_off[p] for p, w in enumerate(ws)])
    assert ce.size > 40 and set((ce % 4).tolist()) == {0, 1, 2, 3} and (wt < 0).any() and (wt > 0).any()
    th = numpy.array([0.5, 0.25, 2.0])
    a = _arrays(real, nx, ny, seed=nx * 100 + ny)
    rng = numpy.random.default_rng(nx + ny)
    dt = numpy.dtype(real).type
    flat = a['tracer'].reshape(-1)
    flat[rng.choice(flat.size, flat.size // 15, replace=False)] = dt(numpy.inf)     # a face value that is not finite
    if thick != 'scalar':
        for name in ('e3u', 'e3v'):
            e3 = rng.uniform(0.2, 3., (NT if thick == 'timevarying' else 1, NZ, ny, nx)).astype(dt)
            for m in (THFILL, THMISSING, numpy.nan, 0.0):
                e3.reshape(-1)[rng.choice(e3.size, e3.size // 12, replace=False)] = dt(m)
            a[name] = e3
    ref = SectionReference(ce, wt, sg, arc, th, tr_off, nx, ny, uv_markers=(FILL, MISSING), tracer_markers=(CFILL, CMISSING),
                           thick_markers=(THFILL, THMISSING), reference=REF, wrap=g['wrap'], sverdrup=g['sverdrup'],
                           cell_thickness=thick != 'scalar')
    for t in range(NT):
        got = ref.area_step(array_values(a, t))
        want = _naive(ce, wt, sg, arc, th, tr_off, nx, ny, a, t, g['wrap'], thick != 'scalar')
        for nm, (w_, m_) in want.items():
            g_, gm_ = got[nm]
            assert g_.shape == w_.shape == m_.shape == (NZ, ref.row_length), nm
            assert m_.max() > 0, nm
            worst = (numpy.abs(g_ - w_) / numpy.maximum(m_, 1e-300)).max()
            assert numpy.all(numpy.abs(g_ - w_) <= 4 * EPS * m_), (nm, t, worst)
            assert numpy.all(numpy.abs(gm_ - m_) <= 4 * EPS * m_), (nm, t)
        A, T = got['area_profile'][0], got['tracer_area_profile'][0]
        assert (A >= 0).all() and (T > 0).any()
        assert numpy.array_equal(got['area_profile'][0], got['area_profile'][1])       # every area term is >= 0


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
    assert _lib.lib.nf_version() == 100


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


def test_argument_state_and_device_errors():
    from nemoflux_amd import _lib
    lib = _lib.lib
    rows = numpy.zeros(64)
    uv = numpy.zeros(16)
    for name in CALLS:
        assert _compute(name, None, rows) == NF_ERR_ARG, name
        assert b'null' in lib.nf_last_error() and name.encode() in lib.nf_last_error()
    h = _new()
    try:
        for name in CALLS:
            assert _compute(name, ctypes.byref(h), None) == NF_ERR_ARG, name
            assert b'null' in lib.nf_last_error() and name.encode() in lib.nf_last_error()
            assert _compute(name, ctypes.byref(h), rows) == NF_ERR_STATE, name            # nothing set
            assert b'set_tracer first' in lib.nf_last_error() and name.encode() in lib.nf_last_error()
        assert lib.nf_field_set_uv(ctypes.byref(h), uv.ctypes.data, uv.ctypes.data, 3, NF_F64, 0, numpy.nan) == 0
        for name in CALLS:
            assert _compute(name, ctypes.byref(h), rows) == NF_ERR_STATE, name            # uo / vo, no tracer
            assert b'set_tracer first' in lib.nf_last_error()
        assert lib.nf_field_set_tracer(ctypes.byref(h), uv.ctypes.data, 3, NF_F64, 0, numpy.nan) == 0
        for name in CALLS:
            rc = _compute(name, ctypes.byref(h), rows)
            if _lib.device_count() > 0:          # a tracer, but no grid
                assert rc == NF_ERR_STATE and b'set_bounds' in lib.nf_last_error(), name
            else:                                # no device: the loud failure of every compute call
                assert rc == NF_ERR_NO_DEVICE, name
                assert b'no usable AMD GPU' in lib.nf_last_error() and b'no CPU fallback' in lib.nf_last_error()
    finally:
        assert lib.nf_field_del(ctypes.byref(h)) == 0


def test_python_methods_exist_and_refuse_without_a_tracer():
    from nemoflux_amd.field import Field
    f = Field.__new__(Field)
    f.nt, f.nz, f.ny, f.nx = 2, 3, 4, 5
    f._lazy = None
    f._e3 = None
    with pytest.raises(RuntimeError, match='setTracer first'):
        f.computeAreaProfile(0)
    with pytest.raises(RuntimeError, match='out of range'):
        f.computeAreaProfile(2)
    assert callable(Field.decomposeTracerTransport) and isinstance(Field.__dict__['overturningGyre'], staticmethod)


# ---- the decomposition -----------------------------------------------------------------------------------------------------
def test_overturning_gyre_is_the_plain_loop_and_adds_up():
    from nemoflux_amd.field import Field
    rng = numpy.random.default_rng(3)
    nz, n = 7, 5
    V = rng.standard_normal((nz, n))
    A = rng.uniform(0.5, 2., (nz, n))
    T = A * (4. + rng.standard_normal((nz, n)))
    H = rng.standard_normal(n) * 10.
    A[2, 1] = T[2, 1] = 0.0          # a level without area
    A[:, 3] = T[:, 3] = 0.0          # a column without area at all
    d = Field.overturningGyre(V, (A, T), H)
    assert set(d) == {'total', 'throughflow', 'overturning', 'gyre', 'mean'} and d['mean'].shape == (nz, n)
    for c in range(n):
        sA, sT = math.fsum(A[:, c]), math.fsum(T[:, c])
        M = sT / sA if sA != 0.0 else 0.0
        m = [T[z, c] / A[z, c] if A[z, c] != 0.0 else 0.0 for z in range(nz)]
        through = math.fsum(V[:, c]) * M
        over_terms = [V[z, c] * (m[z] - M) for z in range(nz)]
        over = math.fsum(over_terms)
        tol = 8 * EPS * (abs(M) * math.fsum(abs(V[:, c])) + math.fsum(abs(x) for x in over_terms) + abs(H[c]))
        assert numpy.array_equal(d['mean'][:, c], m)
        assert abs(d['throughflow'][c] - through) <= tol and abs(d['overturning'][c] - over) <= tol, c
        assert abs(d['gyre'][c] - (H[c] - through - over)) <= tol, c
        assert d['total'][c] == H[c]
        parts = (d['throughflow'][c], d['overturning'][c], d['gyre'][c])
        assert abs(math.fsum(parts) - d['total'][c]) <= 4 * EPS * math.fsum(abs(x) for x in parts), c
    assert d['mean'][2, 1] == 0.0 and d['throughflow'][3] == 0.0 and d['overturning'][3] == 0.0 and d['gyre'][3] == H[3]
    # segments and totals alike: any trailing column count; shapes are checked
    with pytest.raises(ValueError, match='overturningGyre'):
        Field.overturningGyre(V, (A, T[:-1]), H)
    with pytest.raises(ValueError, match='overturningGyre'):
        Field.overturningGyre(V, (A, T), H[:-1])


# ---- fluxplot --------------------------------------------------------------------------------------------------------------
def test_fluxplot_decompose_options_are_checked():
    from nemoflux_amd.fluxplot import checkDecomposeArgs, main
    checkDecomposeArgs()
    checkDecomposeArgs(True, 'thetao')
    with pytest.raises(RuntimeError, match='--decompose needs --tracer'):
        checkDecomposeArgs(True)
    for kw, opt in ((dict(classes='26,27'), '--classes'), (dict(levels=True), '--levels'), (dict(zrange='0,100'), '--zrange'),
                    (dict(show=True), '--show')):
        with pytest.raises(RuntimeError, match='--decompose and ' + opt):
            checkDecomposeArgs(True, 'thetao', **kw)
    # refused before any file is opened: none of these files exists
    files = dict(tFile='/nonexistent/T.nc', uFile='/nonexistent/U.nc', vFile='/nonexistent/V.nc', lonLatPoints='(0,0),(1,1)')
    for kw in (dict(), dict(tracer='thetao', classes='26,27'), dict(tracer='thetao', levels=True),
               dict(tracer='thetao', zrange='0,10'), dict(tracer='thetao', show=True)):
        with pytest.raises(RuntimeError, match='--decompose'):
            main(decompose=True, **kw, **files)
    # accepted combinations go on to open the files
    for kw in (dict(), dict(sverdrup=True, tracerScale=4.1e-3, tracerRef=1.5), dict(cellThickness=True)):
        with pytest.raises(RuntimeError, match='no such file'):
            main(decompose=True, tracer='thetao', **kw, **files)


def test_fluxplot_command_line_lists_decompose():
    out = subprocess.run([sys.executable, '-m', 'nemoflux_amd.fluxplot', '--help'], cwd=ROOT, capture_output=True, text=True,
                         timeout=120)
    assert out.returncode == 0, out.stderr
    assert '--decompose' in out.stdout
    bad = subprocess.run([sys.executable, '-m', 'nemoflux_amd.fluxplot', '-t', 'no_T.nc', '-u', 'no_U.nc', '-v', 'no_V.nc',
                          '-l', '[(0,0),(1,1)]', '--tracer', 'thetao', '--decompose', '--levels'], cwd=ROOT, capture_output=True,
                         text=True, timeout=120)
    assert bad.returncode != 0 and '--decompose and --levels' in bad.stderr


# ---- closed form from the weights alone ------------------------------------------------------------------------------------
ZONAL = dict(nx=36, ny=18, line="(-130,25),(-30,25)", row=11, i0=5, i1=15)   # 10-degree cells: row 11 spans 20..30 N


def zonal_line_area(arc, nx, row, i0, i1):
    """half the summed south-edge arcs plus the summed north-edge arcs of cells (row, i0 .. i1 - 1)"""
    cells = row * nx + numpy.arange(i0, i1)
    return 0.5 * (math.fsum(arc[cells, 0]) + math.fsum(arc[cells, 2]))


def test_zonal_line_area_from_the_weights(oracle):
    """a zonal line at the mid-latitude of one row of an un-rotated regular grid, spanning whole cells: sum |w| arc is the mean
    of the row's south-edge and north-edge lengths over the span"""
    nx, ny = ZONAL['nx'], ZONAL['ny']
    o = oracle.DataGen(nx, ny, 1, 1, -180., 180., -90., 90., lat_uses_dx=False)
    pts = oracle.assemble_points(o.bounds_lon, o.bounds_lat)
    arc = oracle.arc_lengths(pts).reshape(-1, 4)
    w = oracle.polyline_weights(pts, transect_xyz(ZONAL['line']), periodX=360.)
    cell, slot = w.cell_edge // 4, w.cell_edge % 4
    assert set((cell // nx).tolist()) <= {ZONAL['row'] - 1, ZONAL['row'], ZONAL['row'] + 1}
    # the arc of a slot is the arc of its face: the south slot's is the north edge of the south cell, the west slot's the
    # east edge of the west cell
    a = numpy.select([slot == 0, slot == 1, slot == 2],
                     [arc[numpy.maximum(cell - nx, 0), 2], arc[cell, 1], arc[cell, 2]],
                     arc[numpy.where(cell % nx > 0, cell - 1, cell - 1 + nx), 1])
    got = math.fsum(numpy.abs(w.weight) * a)
    want = zonal_line_area(arc, nx, ZONAL['row'], ZONAL['i0'], ZONAL['i1'])
    print(f'zonal line area: sum |w| arc = {got!r}, closed form = {want!r}')
    assert abs(got - want) <= 1e-12 * want and want > 1.0
