"""Per-cell layer thicknesses (nf_field_set_cell_thickness, Field.setCellThickness, fluxplot --cell-thickness), the part that
needs no GPU: the reference of tests/cellthick_reference.py pinned to a naive triple loop with math.fsum; the new symbols
exported, declared and bound with the same argument lists; the argument and state errors the library decides before it needs
a device; the shape / dtype errors of Field.setCellThickness; the fluxplot refusals.

What needs a device and is therefore checked in tests/test_gpu_cellthick.py: set_cell_thickness after set_thickness (the
latter uploads), the refusal of the three forms that do not take cell thicknesses (they check the weights first), and
everything computed."""
import ctypes
import math
import os
import re
import subprocess
import sys

import numpy
import pytest

from conftest import ROOT
from cellthick_reference import CellThickReference, array_values

NF_ERR_ARG, NF_ERR_STATE = 1, 2
NF_F64, NF_F32 = 0, 1
FILL, MISSING = 1.e20, -999.            # uo / vo
THFILL, THMISSING = -1.e30, 9.e9        # e3u / e3v
R_SV = 6371000.0 / 1.e6


def _header():
    with open(os.path.join(ROOT, 'include', 'nemoflux_amd.h')) as fh:
        return re.sub(r'/\*.*?\*/', '', fh.read(), flags=re.S)


# ---- the reference against a naive loop ------------------------------------------------------------------------------------
def _tiny(real, nt_th, seed):
    """a 6 x 5 x 4 x 3 case: random u, v, thicknesses and tracer with markers of every kind, a land block where all four
    fields are markers, made-up weight entries over every cell and slot"""
    rng = numpy.random.default_rng(seed)
    nx, ny, nz, nt = 6, 5, 4, 3
    dt = numpy.dtype(real).type
    shape = (nt, nz, ny, nx)
    a = {'uo': rng.standard_normal(shape).astype(dt), 'vo': rng.standard_normal(shape).astype(dt),
         'e3u': rng.uniform(0.2, 3., (nt_th, nz, ny, nx)).astype(dt), 'e3v': rng.uniform(0.2, 3., (nt_th, nz, ny, nx)).astype(dt),
         'tracer': (10. + rng.standard_normal(shape)).astype(dt)}
    for name, marks in (('uo', (FILL, MISSING, numpy.nan)), ('vo', (FILL, MISSING, numpy.nan)),
                        ('e3u', (THFILL, THMISSING, numpy.nan)), ('e3v', (THFILL, THMISSING, numpy.nan))):
        flat = a[name].reshape(-1)
        for m in marks:
            flat[rng.choice(flat.size, flat.size // 10, replace=False)] = dt(m)
        a[name][:, 1:, 1:3, 2:4] = dt(marks[0])          # land
    a['tracer'].reshape(-1)[rng.choice(a['tracer'].size, 30, replace=False)] = numpy.nan
    ncell = nx * ny
    nent, nseg = 160, 5
    ce = rng.integers(0, ncell * 4, nent)
    ce[:ncell * 4 // 2] = numpy.arange(0, ncell * 4, 2)      # half of all (cell, slot) pairs for sure
    w = rng.standard_normal(nent)
    sg = numpy.sort(rng.integers(0, nseg, nent))
    arc = rng.uniform(0.01, 0.02, (ncell, 4))
    tr_off = numpy.array([0, 2, 5])
    return a, (ce, w, sg, arc, tr_off), (nx, ny, nz, nt)


def _naive(a, entries, sizes, t, sverdrup, wrap, ref):
    """[segments | transects] volume row, tracer row and volume profile of step t: three nested Python loops, math.fsum"""
    ce, w, sg, arc, tr_off = entries
    nx, ny, nz, nt = sizes
    dt = a['uo'].dtype.type

    def fixed(x, marks):
        return 0.0 if (x != x or any(x == dt(m) for m in marks)) else float(x)

    def present(x):
        return not x != x

    tt = t if a['e3u'].shape[0] > 1 else 0
    nseg = int(tr_off[-1])
    vol = [[[] for _ in range(nseg)] for _ in range(nz)]
    trc = [[[] for _ in range(nseg)] for _ in range(nz)]
    for e in range(ce.size):
        c, slot = int(ce[e]) // 4, int(ce[e]) % 4
        j, i = c // nx, c % nx
        if slot == 0 and j == 0:
            continue
        for z in range(nz):
            if slot in (1, 3):                                   # east face of cell (j, ia)
                ia = i if slot == 1 else (i - 1) % nx
                th, x = a['e3u'][tt, z, j, ia], a['uo'][t, z, j, ia]
                sign_arc = +arc[j * nx + ia, 1]
                ta, has_b = a['tracer'][t, z, j, ia], (ia < nx - 1 or wrap)
                tb = a['tracer'][t, z, j, (ia + 1) % nx]
            else:                                                # north face of cell (ja, i)
                ja = j if slot == 2 else j - 1
                th, x = a['e3v'][tt, z, ja, i], a['vo'][t, z, ja, i]
                sign_arc = -arc[ja * nx + i, 2]
                ta, has_b = a['tracer'][t, z, ja, i], ja < ny - 1
                tb = a['tracer'][t, z, min(ja + 1, ny - 1), i]
            pa, pb = present(ta), has_b and present(tb)
            tf = (0.5 * (float(ta) + float(tb)) if pa and pb else float(ta) if pa else float(tb) if pb else None)
            tf = 0.0 if tf is None else tf - ref
            base = fixed(th, (THFILL, THMISSING)) * fixed(x, (FILL, MISSING)) * sign_arc * (R_SV if sverdrup else 1.0)
            vol[z][sg[e]].append(w[e] * base)
            trc[z][sg[e]].append(w[e] * base * tf)

    def rows(terms):
        seg = numpy.array([[math.fsum(terms[z][s]) for s in range(nseg)] for z in range(nz)])
        tot = numpy.array([[math.fsum(x for s in range(tr_off[p], tr_off[p + 1]) for x in terms[z][s])
                            for p in range(tr_off.size - 1)] for z in range(nz)])
        return numpy.concatenate([seg, tot], axis=1)

    def total(terms):
        return rows([[sum((terms[z][s] for z in range(nz)), []) for s in range(nseg)]] + [[[] for _ in range(nseg)]] * (nz - 1))[0]

    return total(vol), total(trc), rows(vol)


@pytest.mark.parametrize('wrap', [True, False], ids=['wrap', 'nowrap'])
@pytest.mark.parametrize('sverdrup', [False, True], ids=['m2', 'sv'])
@pytest.mark.parametrize('nt_th', [1, 3], ids=['static', 'timevarying'])
@pytest.mark.parametrize('real', ['float64', 'float32'])
def test_reference_is_the_naive_triple_loop(real, nt_th, sverdrup, wrap):
    a, entries, sizes = _tiny(real, nt_th, seed=5 + nt_th)
    ce, w, sg, arc, tr_off = entries
    nx, ny, nz, nt = sizes
    ref = CellThickReference(ce, w, sg, arc, numpy.full(nz, numpy.nan), tr_off, nx, ny, uv_markers=(FILL, MISSING),
                             thick_markers=(THFILL, THMISSING), reference=9.5, wrap=wrap, sverdrup=sverdrup)
    for t in range(nt):
        got = ref.step(array_values(a, t))
        vol, trc, prof = _naive(a, entries, sizes, t, sverdrup, wrap, 9.5)
        for key, want in (('volume', vol), ('tracer', trc), ('volume_profile', prof)):
            g, mag = got[key]
            assert g.shape == want.shape and mag.max() > 0, key
            # the reference rounds each term a few times (6.7e-16 x mag) before its long-double sums; fsum does not
            assert numpy.all(numpy.abs(g - want) <= 4e-15 * mag), (key, t, numpy.abs(g - want).max())
        assert numpy.abs(got['volume'][0]).max() > 0 and numpy.abs(got['tracer'][0]).max() > 0
    if nt_th == 3:      # the thickness of another step gives other rows: t' = t is not t' = 0
        static = {k: (v[:1] if k.startswith('e3') else v) for k, v in a.items()}
        assert not numpy.array_equal(ref.step(array_values(static, 2))['volume'][0], ref.step(array_values(a, 2))['volume'][0])


# ---- ABI -------------------------------------------------------------------------------------------------------------------
SETTERS = {
    'nf_field_set_cell_thickness': ('nf_field **self, const void *e3u, const void *e3v, long nt_th, int dtype, int on_device, '
                                    'double fill_value'),
    'nf_field_set_cell_thickness_missing_value': 'nf_field **self, double missing_value',
}
C_TYPES = {'const void *': ctypes.c_void_p, 'long': ctypes.c_long, 'int': ctypes.c_int, 'double': ctypes.c_double}


def test_new_symbols_are_exported_declared_and_bound_alike():
    from nemoflux_amd import _lib
    header = _header()
    out = subprocess.run(['nm', '-D', '--defined-only', _lib._SO], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stderr
    exported = {ln.split()[-1] for ln in out.stdout.splitlines() if ln.split()}
    for name, args in SETTERS.items():
        assert name in exported, name
        m = re.search(r'\bint\s+' + name + r'\s*\(([^)]*)\)\s*;', header)
        assert m, f'{name} is not declared in include/nemoflux_amd.h'
        declared = ' '.join(m.group(1).split())
        assert declared == args, (name, declared)
        fn = getattr(_lib.lib, name)
        want = []
        for a in declared.split(',')[1:]:
            a = a.strip()
            ctype = next(v for k, v in C_TYPES.items() if a.startswith(k + ('' if k.endswith('*') else ' ')))
            want.append(ctype)
        assert fn.restype is ctypes.c_int
        assert list(fn.argtypes[1:]) == want, (name, fn.argtypes)
    assert _lib.lib.nf_version() == 100


def _new():
    from nemoflux_amd import _lib
    h = ctypes.c_void_p()
    assert _lib.lib.nf_field_new(ctypes.byref(h)) == 0
    return h


def test_setter_argument_and_state_errors():
    from nemoflux_amd import _lib
    lib = _lib.lib
    x = numpy.zeros(16)
    p = x.ctypes.data
    assert lib.nf_field_set_cell_thickness(None, p, p, 1, NF_F64, 0, numpy.nan) == NF_ERR_ARG and b'null' in lib.nf_last_error()
    assert lib.nf_field_set_cell_thickness_missing_value(None, 1.0) == NF_ERR_ARG and b'null' in lib.nf_last_error()
    h = _new()
    try:
        # before set_uv
        assert lib.nf_field_set_cell_thickness(ctypes.byref(h), p, p, 1, NF_F64, 0, numpy.nan) == NF_ERR_STATE
        assert b'set_uv' in lib.nf_last_error() and b'set_thickness' in lib.nf_last_error()
        # clearing is always fine, whatever the other arguments say
        assert lib.nf_field_set_cell_thickness(ctypes.byref(h), None, None, 0, 7, 0, numpy.nan) == 0
        assert lib.nf_field_set_cell_thickness_missing_value(ctypes.byref(h), -1.) == 0
        assert lib.nf_field_set_uv(ctypes.byref(h), p, p, 3, NF_F64, 0, numpy.nan) == 0
        assert lib.nf_field_set_cell_thickness(ctypes.byref(h), p, None, 1, NF_F64, 0, numpy.nan) == NF_ERR_ARG
        assert b'e3v' in lib.nf_last_error()
        assert lib.nf_field_set_cell_thickness(ctypes.byref(h), p, p, 1, 7, 0, numpy.nan) == NF_ERR_ARG
        assert b'dtype must be' in lib.nf_last_error()
        assert lib.nf_field_set_cell_thickness(ctypes.byref(h), p, p, 1, NF_F32, 0, numpy.nan) == NF_ERR_ARG
        msg = lib.nf_last_error()
        assert b'float32' in msg and b'float64' in msg and b'dtype' in msg
        for nt_th in (0, 2, 4, -1):
            assert lib.nf_field_set_cell_thickness(ctypes.byref(h), p, p, nt_th, NF_F64, 0, numpy.nan) == NF_ERR_ARG, nt_th
            msg = lib.nf_last_error()
            assert f'nt = {nt_th}'.encode() in msg and b'1 (static)' in msg and b'3' in msg
        # right dtype and step count, but no set_thickness yet: it fixes nz
        for nt_th in (1, 3):
            assert lib.nf_field_set_cell_thickness(ctypes.byref(h), p, p, nt_th, NF_F64, 1, numpy.nan) == NF_ERR_STATE
            assert b'set_thickness first' in lib.nf_last_error()
    finally:
        assert lib.nf_field_del(ctypes.byref(h)) == 0


# ---- Field.setCellThickness: what it decides before it calls the library ---------------------------------------------------
def _bare_field(real='float32'):
    from nemoflux_amd.field import Field
    f = Field.__new__(Field)
    f.nt, f.nz, f.ny, f.nx = 3, 4, 5, 6
    f._uv_code = NF_F32 if real == 'float32' else NF_F64
    f._h = None
    return f


def test_python_shape_and_dtype_errors():
    f = _bare_field('float32')
    ok = numpy.ones((4, 5, 6), numpy.float32)
    for bad in ((4, 5, 7), (2, 4, 5, 6), (3, 4, 5), (5, 6), (3, 4, 5, 6, 1), (4, 4, 5, 6)):
        with pytest.raises(RuntimeError) as e:
            f.setCellThickness(numpy.ones(bad, numpy.float32), ok)
        assert 'e3u' in str(e.value) and str(bad) in str(e.value) and '(3, 4, 5, 6)' in str(e.value), str(e.value)
        with pytest.raises(RuntimeError, match='e3v has shape'):
            f.setCellThickness(ok, numpy.ones(bad, numpy.float32))
    with pytest.raises(RuntimeError, match='both static or both per time step'):
        f.setCellThickness(ok, numpy.ones((3, 4, 5, 6), numpy.float32))
    with pytest.raises(RuntimeError, match='both e3u and e3v'):
        f.setCellThickness(ok, None)
    # a time-varying array of another dtype is not cast; neither is an integer one
    with pytest.raises(RuntimeError) as e:
        f.setCellThickness(numpy.ones((3, 4, 5, 6)), numpy.ones((3, 4, 5, 6)))
    assert 'float64' in str(e.value) and 'float32' in str(e.value)
    with pytest.raises(RuntimeError, match='int32'):
        f.setCellThickness(numpy.ones((4, 5, 6), numpy.int32), numpy.ones((4, 5, 6), numpy.int32))
    g = _bare_field('float64')
    with pytest.raises(RuntimeError) as e:
        g.setCellThickness(numpy.ones((3, 4, 5, 6), numpy.float32), numpy.ones((3, 4, 5, 6), numpy.float32))
    assert 'float32' in str(e.value) and 'float64' in str(e.value)


def test_python_file_pairs_are_checked_before_the_library(tmp_path):
    f = _bare_field('float64')
    p = str(tmp_path / 'U.npz')
    numpy.savez(p, e3u=numpy.ones((2, 4, 5, 6)), thk=numpy.ones((3, 4, 5, 6), numpy.float32))
    with pytest.raises(RuntimeError, match='could not read e3v'):
        f.setCellThickness(numpy.ones((4, 5, 6)), (p, 'e3v'))
    with pytest.raises(RuntimeError, match=r'\(2, 4, 5, 6\)'):
        f.setCellThickness((p, 'e3u'), (p, 'e3u'))
    with pytest.raises(RuntimeError, match='float32'):
        f.setCellThickness((p, 'thk'), (p, 'thk'))


# ---- fluxplot --------------------------------------------------------------------------------------------------------------
def test_fluxplot_cell_thickness_options_are_checked():
    from nemoflux_amd.fluxplot import checkCellThicknessArgs, main
    checkCellThicknessArgs()
    checkCellThicknessArgs(True)
    checkCellThicknessArgs(True, 'thkcello', 'thkcello', 'a.nc', 'b.nc', tracer='thetao')
    checkCellThicknessArgs(True, levels=True)
    for kw in (dict(e3u='x'), dict(e3v='x'), dict(e3FileU='f'), dict(e3FileV='f')):
        with pytest.raises(RuntimeError, match='need --cell-thickness'):
            checkCellThicknessArgs(False, **kw)
    with pytest.raises(RuntimeError, match='--classes'):
        checkCellThicknessArgs(True, classes='1,2', tracer='sigma0')
    with pytest.raises(RuntimeError, match='--carry'):
        checkCellThicknessArgs(True, classes='1,2', tracer='sigma0', carry='thetao')
    with pytest.raises(RuntimeError, match='--levels --tracer'):
        checkCellThicknessArgs(True, levels=True, tracer='thetao')
    # refused before any file is opened: none of these files exists
    files = dict(tFile='/nonexistent/T.nc', uFile='/nonexistent/U.nc', vFile='/nonexistent/V.nc', lonLatPoints='(0,0),(1,1)')
    for kw in (dict(classes='1,2', tracer='sigma0'), dict(classes='1,2', tracer='sigma0', carry='thetao'),
               dict(levels=True, tracer='thetao')):
        with pytest.raises(RuntimeError, match='--cell-thickness cannot be combined'):
            main(cellThickness=True, **kw, **files)
    with pytest.raises(RuntimeError, match='no such file'):      # an accepted combination goes on to open the files
        main(cellThickness=True, zrange='0,10', **files)


def test_fluxplot_command_line_lists_the_cell_thickness_options():
    out = subprocess.run([sys.executable, '-m', 'nemoflux_amd.fluxplot', '--help'], cwd=ROOT, capture_output=True, text=True,
                         timeout=120)
    assert out.returncode == 0, out.stderr
    for opt in ('--cell-thickness', '--e3u', '--e3v', '--e3-file-u', '--e3-file-v'):
        assert opt in out.stdout, opt
