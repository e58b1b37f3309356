"""Gross (inflow / outflow) transports (nf_field_compute_gross_profile, Field.computeGrossProfile, Field.grossTransport,
Field.transportWeightedTracer, fluxplot --gross), the part that needs no GPU: the reference of tests/gross_reference.py pinned
to a naive loop with math.fsum on a 12 x 9 x 3 case with land, both markers and the Sverdrup scale; P + N against the profile
references; no |q| of the generated inputs near underflow; the two calls declared, exported and bound, and the errors they
decide before they need a device; the three Field methods; the fluxplot argument checks."""
import ctypes
import math
import os
import re
import subprocess
import sys

import numpy
import pytest

from conftest import ROOT, transect_xyz
from cellthick_reference import CellThickReference
from gross_reference import (FILL, MIN_ABS_Q, MISSING, THFILL, THMISSING, GrossReference, array_values, gross_thickness,
                             gross_velocities, inputs_are_safe)
from resolved_reference import ResolvedReference

EPS = numpy.finfo(numpy.float64).eps
NF_ERR_ARG, NF_ERR_STATE, NF_ERR_NO_DEVICE = 1, 2, 4
NF_F64 = 0
CALLS = ('nf_field_compute_gross_profile', 'nf_field_compute_gross_profile_async')
NX, NY, NZ, NT = 12, 9, 3, 2
TFILL, TMISSING = 9999., -7777.
REF = 3.25
TH = numpy.array([0.5, 0.25, 2.0])
LINES = ["(150,-50),(179,-20),(200,35),(160,70)", "(-175,-88),(-100,-62),(-170,20),(-185,75)", "(-20,-89),(175,-89)",
         "(-170,89),(10,88),(10,-10)"]
# the shapes and seeds of the inputs of tests/test_gpu_gross.py
GPU_GRIDS = [(72, 36), (73, 37)]
GPU_NZ, GPU_NT, GPU_UV_SEED, GPU_E3_SEED = 7, 3, 11, 61


def _tracer(real, shape, seed):
    rng = numpy.random.default_rng(seed)
    dt = numpy.dtype(real).type
    tau = (REF + 2. * rng.standard_normal(shape)).astype(real)     # tf of either sign
    for m in (TFILL, TMISSING, numpy.nan):
        tau[rng.random(shape) < 0.05] = dt(m)
    return tau


def _naive(ce, w, sg, arc, tr_off, a, t, cell_thickness):
    """P(z), N(z) of both forms as math.fsum of their terms, one (entry, level) at a time from the full arrays"""
    dt = a['uo'].dtype.type
    nseg, ntr = int(tr_off[-1]), len(tr_off) - 1
    tr_of = [p for p in range(ntr) for _ in range(tr_off[p], tr_off[p + 1])]

    def present(x, marks):
        return not math.isnan(x) and all(x != dt(m) for m in marks)

    def val(name, tt, z, c):
        return a[name][tt, z].reshape(-1)[c]

    terms = {'volume': {}, 'carried': {}}
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
            xa = val('tracer', t, z, ca)
            pa = present(xa, (TFILL, TMISSING))
            pb = cb is not None and present(val('tracer', t, z, cb), (TFILL, TMISSING))
            tf = 0.0
            if pa and pb:
                tf = 0.5 * (float(xa) + float(val('tracer', t, z, cb))) - REF
            elif pa:
                tf = float(xa) - REF
            elif pb:
                tf = float(val('tracer', t, z, cb)) - REF
            al = float(arc[ca, 1]) if east else -float(arc[ca, 2])
            q = float(w[e]) * (((h * vel) * al) * (6371000.0 / 1.e6))
            cc = float(w[e]) * (((h * (vel * tf)) * al) * (6371000.0 / 1.e6))
            if q == 0.0:
                continue
            part = 0 if q > 0 else 1
            for col in (s, nseg + tr_of[s]):
                terms['volume'].setdefault((part, z, col), []).append(q)
                terms['carried'].setdefault((part, z, col), []).append(cc)
    out = {}
    for nm in terms:
        want, mag = numpy.zeros((2, NZ, nseg + ntr)), numpy.zeros((2, NZ, nseg + ntr))
        for idx, xs in terms[nm].items():
            want[idx], mag[idx] = math.fsum(xs), math.fsum(abs(x) for x in xs)
        out[nm] = (want, mag)
    return out


def _weights(oracle):
    o = oracle.DataGen(NX, NY, NZ, NT, -180., 180., -90., 90., lat_uses_dx=False)
    pts = oracle.assemble_points(o.bounds_lon, o.bounds_lat)
    arc = oracle.arc_lengths(pts)
    ws = [oracle.polyline_weights(pts, transect_xyz(s), periodX=360.) for s in LINES]
    tr_off = numpy.concatenate([[0], numpy.cumsum([w.nseg for w in ws])])
    ce = numpy.concatenate([w.cell_edge for w in ws])
    wt = numpy.concatenate([w.weight for w in ws])
    sg = numpy.concatenate([w.seg + tr_off[p] for p, w in enumerate(ws)])
    return ce, wt, sg, numpy.asarray(arc).reshape(-1, 4), tr_off


@pytest.mark.parametrize('thick', ['scalar', 'static', 'timevarying'])
@pytest.mark.parametrize('real', ['float64', 'float32'])
def test_gross_reference_is_the_naive_loop_and_adds_up_to_the_profiles(oracle, real, thick):
    ce, wt, sg, arc, tr_off = _weights(oracle)
    assert ce.size > 40 and set((ce % 4).tolist()) == {0, 1, 2, 3} and (wt < 0).any() and (wt > 0).any()
    shape = (NT, NZ, NY, NX)
    u, v = gross_velocities(real, shape, seed=5)
    dt = numpy.dtype(real).type
    for a in (u, v):
        assert numpy.isnan(a).any() and (a == dt(FILL)).any() and (a == dt(MISSING)).any() and (a == 0).any()
    arrays = {'uo': u, 'vo': v, 'tracer': _tracer(real, shape, seed=7)}
    cell = thick != 'scalar'
    if cell:
        arrays['e3u'], arrays['e3v'] = gross_thickness(real, (NT if thick == 'timevarying' else 1, NZ, NY, NX), seed=9)
    assert inputs_are_safe(u, v, (arrays['e3u'], arrays['e3v']) if cell else ())
    kw = dict(uv_markers=(FILL, MISSING), tracer_markers=(TFILL, TMISSING), thick_markers=(THFILL, THMISSING), reference=REF,
              wrap=True, sverdrup=True)
    ref = GrossReference(ce, wt, sg, arc, TH, tr_off, NX, NY, cell_thickness=cell, **kw)
    for t in range(NT):
        got = ref.gross_step(array_values(arrays, t))
        want = _naive(ce, wt, sg, arc, tr_off, arrays, t, cell)
        assert got['min_abs_q'] >= MIN_ABS_Q
        for nm, (w_, m_) in want.items():
            g_, gm_ = got[nm]
            assert g_.shape == w_.shape == m_.shape == (2, NZ, ref.row_length), nm
            assert m_[0].max() > 0 and m_[1].max() > 0, nm
            worst = (numpy.abs(g_ - w_) / numpy.maximum(m_, 1e-300)).max()
            assert numpy.all(numpy.abs(g_ - w_) <= 4 * EPS * m_), (nm, t, worst)
            assert numpy.all(numpy.abs(gm_ - m_) <= 4 * EPS * m_), (nm, t)
        P, N = got['volume'][0]
        assert (P >= 0).all() and (N <= 0).all() and (P > 0).any() and (N < 0).any()
        assert numpy.array_equal(got['volume'][0][0], got['volume'][1][0]) and numpy.array_equal(-N, got['volume'][1][1])
        assert (got['carried'][0][0] < 0).any() and (got['carried'][0][1] > 0).any()    # split by the water, not by its own sign
        # P + N is the profile row of the existing references
        if cell:
            net = CellThickReference(ce, wt, sg, arc, TH, tr_off, NX, NY, **kw).step(array_values(arrays, t))
            forms = (('volume', 'volume_profile'),)
        else:
            net = ResolvedReference(ce, wt, sg, arc, TH, tr_off, NX, NY, uv_markers=(FILL, MISSING),
                                    tracer_markers=(TFILL, TMISSING), reference=REF, wrap=True,
                                    sverdrup=True).step(array_values(dict(arrays, **{'class': arrays['tracer']}), t))
            forms = (('volume', 'volume_profile'), ('carried', 'tracer_profile'))
        for nm, prof in forms:
            (g_, m_), (w_, wm_) = got[nm], net[prof]
            assert numpy.all(numpy.abs(g_[0] + g_[1] - w_) <= 4 * EPS * wm_), (nm, t)
            assert numpy.all(numpy.abs(m_[0] + m_[1] - wm_) <= 4 * EPS * wm_), (nm, t)


@pytest.mark.parametrize('grid', GPU_GRIDS, ids=lambda g: f'{g[0]}x{g[1]}')
@pytest.mark.parametrize('real', ['float64', 'float32'])
def test_generated_inputs_keep_every_q_far_from_underflow(real, grid):
    """the inputs of the GPU tests: velocities of magnitude in [0.01, 1] (or 0, or missing), thicknesses >= 0.2 (or 0, or
    missing); with weights and arcs that are ratios and angles of a degree-sized grid no non-zero |q| comes near 1e-200, so a
    sign cannot differ between device and reference through underflow (the GPU tests assert min_abs_q of the reference)"""
    nx, ny = grid
    u, v = gross_velocities(real, (GPU_NT, GPU_NZ, ny, nx), seed=GPU_UV_SEED)
    e3 = gross_thickness(real, (GPU_NT, GPU_NZ, ny, nx), seed=GPU_E3_SEED)
    assert inputs_are_safe(u, v, e3)
    bad = u.copy()
    bad.reshape(-1)[3] = 1e-3
    assert not inputs_are_safe(bad, v, e3)
    thin = e3[0].copy()
    thin.reshape(-1)[3] = 0.1
    assert not inputs_are_safe(u, v, (thin, e3[1]))
    for a in (u, v) + tuple(e3):
        assert numpy.isnan(a).any() and (a == 0).any()


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
    assert _lib.lib.nf_version() == 100


def test_gross_chunk_knob_takes_the_built_chunks_only():
    from nemoflux_amd import _lib
    for ok in (2, 4, 8, 0):
        assert _lib.lib.nf_tuning_set(b'gross_chunk', ok) == 0, ok
    for bad in (1, 3, 16, -4):
        assert _lib.lib.nf_tuning_set(b'gross_chunk', bad) != 0, bad
    assert _lib.lib.nf_tuning_set(b'gross_chunk', 0) == 0


def _new():
    from nemoflux_amd import _lib
    h = ctypes.c_void_p()
    assert _lib.lib.nf_field_new(ctypes.byref(h)) == 0
    return h


def _compute(name, h, carry, out):
    from nemoflux_amd import _lib
    fn = getattr(_lib.lib, name)
    if out is None:
        return fn(h, 0, carry, None)
    return fn(h, 0, carry, ctypes.c_void_p(out.ctypes.data) if name.endswith('_async') else _lib.dptr(out))


def test_argument_state_and_device_errors():
    from nemoflux_amd import _lib
    lib = _lib.lib
    rows = numpy.zeros(64)
    uv = numpy.zeros(16)
    for name in CALLS:
        assert _compute(name, None, 0, rows) == NF_ERR_ARG, name
        assert b'null' in lib.nf_last_error() and name.encode() in lib.nf_last_error()
    h = _new()
    try:
        for name in CALLS:
            assert _compute(name, ctypes.byref(h), 0, None) == NF_ERR_ARG, name
            assert b'null' in lib.nf_last_error() and name.encode() in lib.nf_last_error()
            for carry in (2, -1):
                assert _compute(name, ctypes.byref(h), carry, rows) == NF_ERR_ARG, name
                assert b'carry must be 0 or 1' in lib.nf_last_error() and name.encode() in lib.nf_last_error()
            assert _compute(name, ctypes.byref(h), 1, rows) == NF_ERR_STATE, name            # nothing set
            assert b'set_tracer first' in lib.nf_last_error() and name.encode() in lib.nf_last_error()
        assert lib.nf_field_set_uv(ctypes.byref(h), uv.ctypes.data, uv.ctypes.data, 3, NF_F64, 0, numpy.nan) == 0
        for name in CALLS:
            assert _compute(name, ctypes.byref(h), 1, rows) == NF_ERR_STATE, name            # uo / vo, no tracer
            assert b'set_tracer first' in lib.nf_last_error() and name.encode() in lib.nf_last_error()
        assert lib.nf_field_set_tracer(ctypes.byref(h), uv.ctypes.data, 3, NF_F64, 0, numpy.nan) == 0
        for name in CALLS:
            for carry in (0, 1):
                rc = _compute(name, ctypes.byref(h), carry, rows)
                if _lib.device_count() > 0:          # no grid
                    assert rc == NF_ERR_STATE and b'set_bounds' in lib.nf_last_error(), name
                else:                                # no device: the loud failure of every compute call
                    assert rc == NF_ERR_NO_DEVICE, name
                    assert b'no usable AMD GPU' in lib.nf_last_error() and b'no CPU fallback' in lib.nf_last_error()
    finally:
        assert lib.nf_field_del(ctypes.byref(h)) == 0


# ---- Python ----------------------------------------------------------------------------------------------------------------
def test_python_methods_exist_and_check_their_arguments():
    from nemoflux_amd.field import Field
    f = Field.__new__(Field)
    f.nt, f.nz, f.ny, f.nx = 2, 3, 4, 5
    f._lazy = None
    f._e3 = None
    with pytest.raises(RuntimeError, match='setTracer first'):
        f.computeGrossProfile(0, carry=True)
    with pytest.raises(RuntimeError, match='out of range'):
        f.computeGrossProfile(2)
    assert isinstance(Field.__dict__['grossTransport'], staticmethod)
    assert isinstance(Field.__dict__['transportWeightedTracer'], staticmethod)


def test_gross_transport_is_the_depth_sum_or_the_band_sum():
    from nemoflux_amd.field import Field, _band_sum
    rng = numpy.random.default_rng(2)
    nz, n = 5, 4
    parts = numpy.stack([rng.random((nz, n)), -rng.random((nz, n))])
    got = Field.grossTransport(parts)
    assert got.shape == (2, n) and numpy.array_equal(got, parts.sum(axis=1))
    bounds = numpy.array([[0., 1.], [1., 3.], [3., 6.], [6., 10.], [10., 15.]])
    band = Field.grossTransport(parts, 2., 8., bounds_depth=bounds)
    for k in (0, 1):
        want = 0.5 * parts[k, 1] + parts[k, 2] + 0.5 * parts[k, 3]
        assert numpy.allclose(band[k], want, rtol=4 * EPS, atol=0)
        assert numpy.array_equal(band[k], _band_sum(parts[k], bounds, 2., 8.))
    whole = Field.grossTransport(parts, 0., 15., bounds_depth=bounds)
    assert numpy.allclose(whole, got, rtol=8 * EPS, atol=0)
    assert (band[0] >= 0).all() and (band[1] <= 0).all()
    for bad in (dict(ztop=1.), dict(ztop=1., zbot=2.), dict(ztop=3., zbot=2., bounds_depth=bounds),
                dict(ztop=1., zbot=2., bounds_depth=bounds[:-1])):
        with pytest.raises(ValueError, match='grossTransport'):
            Field.grossTransport(parts, **bad)
    with pytest.raises(ValueError, match='grossTransport'):
        Field.grossTransport(parts[0])


def test_transport_weighted_tracer_is_the_ratio_plus_the_reference():
    from nemoflux_amd.field import Field
    V = numpy.array([[2., 0., 4.], [-1., -2., 0.]])
    C = numpy.array([[6., 0., -2.], [-5., 1., 0.]])
    m = Field.transportWeightedTracer(V, C, reference=1.5)
    assert m.shape == V.shape
    assert numpy.array_equal(m[0, [0, 2]], [6. / 2. + 1.5, -2. / 4. + 1.5]) and numpy.array_equal(m[1, :2], [5. + 1.5, -0.5 + 1.5])
    assert numpy.isnan(m[0, 1]) and numpy.isnan(m[1, 2])
    assert numpy.array_equal(Field.transportWeightedTracer(V[:, :1], C[:, :1]), [[3.], [5.]])
    assert 'present wherever the velocity is' in ' '.join(Field.transportWeightedTracer.__doc__.split())
    with pytest.raises(ValueError, match='transportWeightedTracer'):
        Field.transportWeightedTracer(V, C[:, :2])
    with pytest.raises(ValueError, match='transportWeightedTracer'):
        Field.transportWeightedTracer(V[0], C[0])


# ---- fluxplot --------------------------------------------------------------------------------------------------------------
def test_fluxplot_gross_options_are_checked():
    from nemoflux_amd.fluxplot import checkGrossArgs, main
    checkGrossArgs()
    checkGrossArgs(True)
    for kw, opt in ((dict(classes='26,27'), '--classes'), (dict(levels=True), '--levels'), (dict(decompose=True), '--decompose'),
                    (dict(eddy=True), '--eddy'), (dict(show=True), '--show')):
        with pytest.raises(RuntimeError, match='--gross and ' + opt):
            checkGrossArgs(True, **kw)
    # refused before any file is opened: none of these files exists
    files = dict(tFile='/nonexistent/T.nc', uFile='/nonexistent/U.nc', vFile='/nonexistent/V.nc', lonLatPoints='(0,0),(1,1)')
    for kw in (dict(tracer='thetao', classes='26,27'), dict(levels=True), dict(tracer='thetao', levels=True),
               dict(tracer='thetao', decompose=True), dict(tracer='thetao', eddy=True), dict(show=True)):
        with pytest.raises(RuntimeError, match='--gross and'):
            main(gross=True, **kw, **files)
    # accepted combinations go on to open the files
    for kw in (dict(), dict(zrange='0,100'), dict(cellThickness=True), dict(tracer='thetao', tracerRef=1.5, tracerScale=4.1e-3),
               dict(tracer='thetao', zrange='0,100', cellThickness=True, sverdrup=True)):
        with pytest.raises(RuntimeError, match='no such file'):
            main(gross=True, **kw, **files)
    # without --gross the tracer transport still has no depth band
    with pytest.raises(RuntimeError, match='--tracer and --zrange'):
        main(tracer='thetao', zrange='0,100', **files)


def test_fluxplot_command_line_lists_gross():
    out = subprocess.run([sys.executable, '-m', 'nemoflux_amd.fluxplot', '--help'], cwd=ROOT, capture_output=True, text=True,
                         timeout=120)
    assert out.returncode == 0, out.stderr
    assert '--gross' in out.stdout
    bad = subprocess.run([sys.executable, '-m', 'nemoflux_amd.fluxplot', '-t', 'no_T.nc', '-u', 'no_U.nc', '-v', 'no_V.nc',
                          '-l', '[(0,0),(1,1)]', '--gross', '--levels'], cwd=ROOT, capture_output=True, text=True, timeout=120)
    assert bad.returncode != 0 and '--gross and --levels' in bad.stderr
