"""Face thicknesses derived from e3t (nf_face_thickness, nemoflux_amd.thickness, fluxplot --e3t), the part that needs no GPU: the
numpy restatement of tests/face_thickness_reference.py pinned bit for bit to a scalar Python loop on every input set of the GPU
tests, against closed forms, and through every fallback of the definition one by one; the branches that the GPU tests' inputs
take, and that the wide inputs (past one column chunk) tell a wrong east neighbour at every chunk boundary; the symbol
exported, declared and bound; every argument error the library decides before it needs a device; the Python
argument checks of face_thickness, FaceThickness, Field.setCellThickness and fluxplot."""
import ctypes
import os
import re
import subprocess

import numpy
import pytest

from conftest import ROOT
import face_thickness_reference as ref

NF_ERR_ARG = 1
NF_F64, NF_F32 = 0, 1
EM, SM = (ref.EFILL, ref.EMISSING), (ref.SFILL, ref.SMISSING)
CASES = ref.raw_cases()
ARGS = ('void *e3u_out_dev, void *e3v_out_dev, const void *e3t_dev, const void *e3t0_dev, const void *e3u0_dev, '
        'const void *e3v0_dev, long nz, long ny, long nx, int dtype, int rule, int wrap_x, double fill, double missing, '
        'double fill0, double missing0, void *hip_stream')


def _restated(case, arrays=None):
    real, nz, ny, nx, rule, wrap = case
    e3t, *statics = ref.case_arrays(case) if arrays is None else arrays
    return ref.face_thickness(e3t, rule, *statics, wrap=wrap, markers=EM, static_markers=SM, with_branches=True)


# ---- 1. the restatement is the scalar loop -------------------------------------------------------------------------------------
@pytest.mark.parametrize('case', CASES, ids=[ref.case_id(c) for c in CASES])
def test_restatement_equals_the_scalar_loop_bit_for_bit(case):
    real, nz, ny, nx, rule, wrap = case
    e3t, *statics = ref.case_arrays(case)
    u, v, _, _ = _restated(case)
    lu, lv = ref.face_thickness_loop(e3t, rule, *statics, wrap=wrap, markers=EM, static_markers=SM)
    assert u.dtype == numpy.dtype(real) and ref.same_bits(u, lu) and ref.same_bits(v, lv)


@pytest.mark.parametrize('rule', ['min', 'mean', 'anomaly'])
@pytest.mark.parametrize('real', ['float64', 'float32'])
def test_restatement_equals_the_scalar_loop_on_the_field_series(real, rule):
    for grid in ((72, 36), (73, 37)):
        e3t, *statics = ref.series(real, grid, 3, 7, rule)
        u, v = ref.want_series(e3t, rule, statics)
        t = 1
        lu, lv = ref.face_thickness_loop(e3t[t], rule, *statics, markers=EM, static_markers=SM)
        assert ref.same_bits(u[t], lu) and ref.same_bits(v[t], lv)


# ---- 2. closed forms --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('real', ['float64', 'float32'])
def test_partial_steps_closed_form(real):
    """e3t = clip(H - D_z, 0, h_z) under min gives clip(min(H_i, H_i+1) - D_z, 0, h_z): rounding is monotone, so min commutes"""
    rng = numpy.random.default_rng(5)
    ny, nx = 9, 13
    h = numpy.array([2.5, 3.0, 2.5, 2.0, 3.5])
    D = numpy.concatenate([[0.], numpy.cumsum(h)[:-1]])
    H = rng.uniform(0.0, 15.0, (ny, nx))

    def cells(Hf):
        return numpy.clip(Hf[None] - D[:, None, None], 0.0, h[:, None, None]).astype(real)

    for wrap in (True, False):
        u, v = ref.face_thickness(cells(H), 'min', wrap=wrap)
        He = numpy.roll(H, -1, axis=1)
        if not wrap:
            He[:, -1] = H[:, -1]
        Hn = numpy.concatenate([H[1:], H[-1:]])
        assert numpy.array_equal(u, cells(numpy.minimum(H, He))) and numpy.array_equal(v, cells(numpy.minimum(H, Hn)))
        assert (u == 0).any() and (u > 0).any() and len(numpy.unique(u)) > 20


@pytest.mark.parametrize('rule', ['min', 'mean'])
@pytest.mark.parametrize('real', ['float64', 'float32'])
def test_uniform_levels_closed_form(real, rule):
    h = numpy.array([2.5, 3.0, 0.1, 2.0, 1. / 3.]).astype(real)
    e3t = numpy.ascontiguousarray(numpy.broadcast_to(h[:, None, None], (5, 6, 7)))
    for wrap in (True, False):
        u, v = ref.face_thickness(e3t, rule, wrap=wrap)
        assert numpy.array_equal(u, e3t) and numpy.array_equal(v, e3t)


@pytest.mark.parametrize('real', ['float64', 'float32'])
def test_constant_anomalies_closed_form(real):
    """e3t = e3t0 + d with d constant per level on the lattice of 1/8: e3u0 + d"""
    rng = numpy.random.default_rng(6)
    shape = (4, 6, 7)
    e3t0, e3u0, e3v0 = ((rng.integers(2, 33, shape) / 8.).astype(real) for _ in range(3))
    d = numpy.array([0.125, -0.25, 0.0, 0.5]).astype(real)[:, None, None]
    for wrap in (True, False):
        u, v = ref.face_thickness(e3t0 + d, 'anomaly', e3t0, e3u0, e3v0, wrap=wrap)
        assert numpy.array_equal(u, e3u0 + d) and numpy.array_equal(v, e3v0 + d)


# ---- 3. every fallback, one by one ------------------------------------------------------------------------------------------------
def _one(real, rule, e3t, e3t0=None, e3u0=None, e3v0=None, wrap=True):
    arrs = [None if a is None else numpy.array(a, dtype=real) for a in (e3t, e3t0, e3u0, e3v0)]
    u, v = ref.face_thickness(arrs[0], rule, *arrs[1:], wrap=wrap, markers=EM, static_markers=SM)
    lu, lv = ref.face_thickness_loop(arrs[0], rule, *arrs[1:], wrap=wrap, markers=EM, static_markers=SM)
    assert ref.same_bits(u, lu) and ref.same_bits(v, lv)
    return u, v


@pytest.mark.parametrize('real', ['float64', 'float32'])
def test_fallbacks_one_by_one(real):
    dt = numpy.dtype(real).type
    nan, inf = numpy.nan, numpy.inf
    zero_bits = dt(0.0).tobytes()
    for bad in (ref.EFILL, ref.EMISSING, nan):
        # a marker, the other marker, NaN in A (cell 1) or B: the faces beside it are +0.0
        e3t = [[[1.0, bad, 2.0, 3.0], [4.0, 5.0, 6.0, 7.0]]]
        for rule, (east, north) in (('min', (2.0, 2.0)), ('mean', (2.5, 4.0))):
            u, v = _one(real, rule, e3t)
            assert u[0, 0, 0].tobytes() == zero_bits and u[0, 0, 1].tobytes() == zero_bits and v[0, 0, 1].tobytes() == zero_bits
            assert u[0, 0, 2] == dt(east) and v[0, 0, 2] == dt(north)
    # the markers of the statics are not markers of e3t, and the other way round
    u, _ = _one(real, 'min', [[[ref.SMISSING, 1.0]]])
    assert u[0, 0, 0] == dt(ref.SMISSING)
    # the last row has no north neighbour: its own value (mean: 0.5 * (A + A) = A); a missing A there is +0.0
    e3t = [[[1.0, 2.0], [3.0, nan]]]
    for rule in ('min', 'mean'):
        _, v = _one(real, rule, e3t)
        assert v[0, 1, 0] == dt(3.0) and v[0, 1, 1].tobytes() == zero_bits
    # the last column: wrapX off takes its own value, wrapX on the first column
    e3t = [[[1.0, 2.0, 4.0]]]
    assert _one(real, 'min', e3t, wrap=False)[0][0, 0, 2] == dt(4.0) and _one(real, 'min', e3t, wrap=True)[0][0, 0, 2] == dt(1.0)
    assert _one(real, 'mean', e3t, wrap=False)[0][0, 0, 2] == dt(4.0) and _one(real, 'mean', e3t, wrap=True)[0][0, 0, 2] == dt(2.5)
    # anomaly: F0 missing is +0.0 whatever the cells hold; a missing A0 (or A) keeps F0
    e3t, e3t0 = [[[1.5, 2.5, 3.0]]], [[[1.0, 2.0, 2.0]]]
    e3v0 = [[[9.0, 9.0, 9.0]]]
    for bad in (ref.SFILL, ref.SMISSING, nan):
        u, v = _one(real, 'anomaly', e3t, e3t0, [[[bad, 3.0, 3.0]]], e3v0, wrap=False)
        assert u[0, 0, 0].tobytes() == zero_bits and u[0, 0, 1] == dt(3.75) and u[0, 0, 2] == dt(4.0) and v[0, 0, 0] == dt(9.5)
        u, _ = _one(real, 'anomaly', e3t, [[[1.0, bad, 2.0]]], [[[7.0, 3.0, 3.0]]], e3v0, wrap=False)
        assert u[0, 0, 0] == dt(7.0) and u[0, 0, 1] == dt(3.0) and u[0, 0, 2] == dt(4.0)
    u, _ = _one(real, 'anomaly', [[[1.5, ref.EMISSING, 3.0]]], e3t0, [[[7.0, 3.0, 3.0]]], e3v0, wrap=True)
    assert u[0, 0, 0] == dt(7.0) and u[0, 0, 1] == dt(3.0) and u[0, 0, 2] == dt(3.75)
    # A == B, and zeros of either sign: B < A is false, A is taken
    u, _ = _one(real, 'min', [[[2.0, 2.0, -0.0, 0.0]]], wrap=False)
    assert u[0, 0, 0] == dt(2.0) and numpy.signbit(u[0, 0, 2]) and not numpy.signbit(u[0, 0, 3])
    # +inf is present: min takes the other cell, mean and anomaly are +inf; negative results are stored as they come
    e3t = [[[inf, 2.0, -3.0]]]
    assert list(_one(real, 'min', e3t, wrap=False)[0][0, 0]) == [dt(2.0), dt(-3.0), dt(-3.0)]
    assert list(_one(real, 'mean', e3t, wrap=False)[0][0, 0]) == [dt(inf), dt(-0.5), dt(-3.0)]
    u, _ = _one(real, 'anomaly', e3t, [[[1.0, 1.0, 1.0]]], [[[1.0, 1.0, 1.0]]], e3v0, wrap=False)
    assert list(u[0, 0]) == [dt(inf), dt(-0.5), dt(-3.0)]
    # a single level, a single row, nx = 1: with wrapX the cell is its own east neighbour
    for wrap in (True, False):
        for rule in ('min', 'mean'):
            u, v = _one(real, rule, [[[2.5]]], wrap=wrap)
            assert u[0, 0, 0] == dt(2.5) and v[0, 0, 0] == dt(2.5)
        u, v = _one(real, 'anomaly', [[[2.5]]], [[[2.0]]], [[[1.0]]], [[[4.0]]], wrap=wrap)
        assert u[0, 0, 0] == dt(1.5) and v[0, 0, 0] == dt(4.5)
    # float32 inputs are widened, the result rounded once
    if real == 'float32':
        a, b = numpy.float32(1.0), numpy.float32(1.0 + 2.0 ** -23)
        u, _ = _one(real, 'mean', [[[a, b]]], wrap=False)
        assert u[0, 0, 0] == numpy.float32(0.5 * (float(a) + float(b)))


# ---- 4. the branches the GPU tests' inputs take ----------------------------------------------------------------------------------
@pytest.mark.parametrize('case', CASES, ids=[ref.case_id(c) for c in CASES])
def test_branch_counts_of_the_gpu_inputs(case):
    real, nz, ny, nx, rule, wrap = case
    u, v, bu, bv = _restated(case)
    if nx == 5:       # one launch of 5 columns: every branch by at least one face (every V face is without a neighbour)
        taken = set(bu.reshape(-1)) | set(bv.reshape(-1))
        assert set(ref.BRANCHES[rule]) <= taken, taken
        return
    for faces, name in ((bu, 'U'), (bv, 'V')):
        for b in ref.BRANCHES[rule]:
            if b == ref.NO_NEIGHBOUR and name == 'U' and wrap:
                assert not (faces == b).any()
                continue
            assert (faces == b).mean() >= 0.01, (name, b, (faces == b).mean())
    assert (u == 0).any() and (v == 0).any() and len(numpy.unique(u[numpy.isfinite(u)])) > 10


@pytest.mark.parametrize('rule', ['min', 'mean', 'anomaly'])
def test_branch_counts_of_the_field_series(rule):
    for grid in ((72, 36), (73, 37)):
        e3t, *statics = ref.series('float32', grid, 3, 7, rule)
        _, _, bu, bv = ref.face_thickness(e3t, rule, *statics, markers=EM, static_markers=SM, with_branches=True)
        for faces in (bu, bv):
            for b in ref.BRANCHES[ref.RULES[rule]]:
                assert (faces == b).mean() >= 0.01 or (b == ref.NO_NEIGHBOUR and faces is bu)


# ---- 5. the raw call ---------------------------------------------------------------------------------------------------------------
def test_symbol_is_exported_declared_and_bound_with_one_argument_list():
    from nemoflux_amd import _lib
    with open(os.path.join(ROOT, 'include', 'nemoflux_amd.h')) as fh:
        header = re.sub(r'/\*.*?\*/', '', fh.read(), flags=re.S)
    out = subprocess.run(['nm', '-D', '--defined-only', _lib._SO], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0
    assert 'nf_face_thickness' in {ln.split()[-1] for ln in out.stdout.splitlines() if ln.split()}
    m = re.search(r'\bint\s+nf_face_thickness\s*\(([^)]*)\)\s*;', header)
    assert m, 'nf_face_thickness is not declared in include/nemoflux_amd.h'
    assert ' '.join(m.group(1).split()) == ARGS
    fn = _lib.lib.nf_face_thickness
    assert fn.restype is ctypes.c_int
    assert list(fn.argtypes) == ([ctypes.c_void_p] * 6 + [ctypes.c_long] * 3 + [ctypes.c_int] * 3 + [ctypes.c_double] * 4 +
                                 [ctypes.c_void_p])
    with open(os.path.join(ROOT, 'nemoflux_amd', 'csrc', 'nf_facethick.hip')) as fh:
        src = fh.read()
    m = re.search(r'extern "C" int nf_face_thickness\s*\(([^)]*)\)', src)
    assert m and ' '.join(m.group(1).split()) == ARGS
    assert 'k_face_thickness' in src and '__shared__' not in src and 'atomic' not in src.lower()
    with open(os.path.join(ROOT, 'nemoflux_amd', 'csrc', 'Makefile')) as fh:
        assert 'nf_facethick.hip' in fh.read()
    assert (_lib.NF_E3_MIN, _lib.NF_E3_MEAN, _lib.NF_E3_ANOMALY) == (ref.MIN, ref.MEAN, ref.ANOMALY)
    for name, code in (('NF_E3_MIN', 0), ('NF_E3_MEAN', 1), ('NF_E3_ANOMALY', 2)):
        assert re.search(rf'#define {name} {code}\b', header)


def test_argument_errors_are_decided_without_a_device():
    """every error listed in the header; the device pointers are never dereferenced (they are not device memory)"""
    from nemoflux_amd import _lib
    lib = _lib.lib
    U, V, T, T0, U0, V0 = (k << 24 for k in range(1, 7))            # stand-ins for device addresses, 16 MiB apart
    nan = numpy.nan
    nbytes = 3 * 4 * 5 * 8

    def call(e3u=U, e3v=V, e3t=T, e3t0=None, e3u0=None, e3v0=None, nz=3, ny=4, nx=5, dtype=NF_F64, rule=0, wrap=1):
        return lib.nf_face_thickness(e3u, e3v, e3t, e3t0, e3u0, e3v0, nz, ny, nx, dtype, rule, wrap, nan, nan, nan, nan, None)

    st = dict(e3t0=T0, e3u0=U0, e3v0=V0)
    bad = [(dict(e3u=None), b'null'), (dict(e3v=None), b'null'), (dict(e3t=None), b'null'),
           (dict(dtype=2), b'dtype'), (dict(dtype=-1), b'dtype'), (dict(rule=3), b'rule'), (dict(rule=-1), b'rule'),
           (dict(nz=0), b'>= 1'), (dict(ny=0), b'>= 1'), (dict(nx=-4), b'>= 1'),
           (dict(rule=0, e3t0=T0), b'anomaly rule only'), (dict(rule=1, e3u0=U0), b'anomaly rule only'),
           (dict(rule=1, **st), b'anomaly rule only'), (dict(rule=0, e3v0=V0), b'anomaly rule only'),
           (dict(rule=2), b'needs'), (dict(rule=2, e3t0=T0, e3u0=U0), b'needs'), (dict(rule=2, e3u0=U0, e3v0=V0), b'needs'),
           (dict(rule=2, e3t0=T0, e3v0=V0), b'needs'),
           (dict(e3u=T), b'overlaps'), (dict(e3v=T), b'overlaps'), (dict(e3v=U), b'overlaps'),
           (dict(e3u=T + nbytes - 8), b'overlaps'), (dict(e3v=T - nbytes + 8), b'overlaps'), (dict(e3v=U + 8), b'overlaps'),
           (dict(rule=2, **dict(st, e3t0=U)), b'overlaps'), (dict(rule=2, e3u=U0 + 16, **st), b'overlaps'),
           (dict(rule=2, e3v=V0 - 16, **st), b'overlaps'), (dict(nz=1 << 40, ny=1 << 40, nx=1 << 40), b'too large')]
    for kw, word in bad:
        assert call(**kw) == NF_ERR_ARG, kw
        err = lib.nf_last_error()
        assert word in err and err.startswith(b'nf_face_thickness:'), (kw, err)
    if _lib.device_count() == 0:
        # what is NOT an error goes on to need a device: ranges that only touch, every rule, both dtypes
        for kw in (dict(), dict(e3u=T + nbytes), dict(e3v=T - nbytes), dict(rule=1, dtype=NF_F32, wrap=0), dict(rule=2, **st),
                   dict(nz=1, ny=1, nx=1)):
            assert call(**kw) not in (0, NF_ERR_ARG), kw
            assert b'no usable AMD GPU' in lib.nf_last_error()


# ---- Python ------------------------------------------------------------------------------------------------------------------------
def test_descriptor_and_raw_call_argument_checks():
    from nemoflux_amd.thickness import FaceThickness, face_thickness
    e3t = numpy.ones((2, 3, 4, 5), numpy.float32)
    st = numpy.ones((3, 4, 5), numpy.float32)
    a = FaceThickness(e3t, fill_value=1.e20)
    assert a.rule == 'min' and a.code == 0 and a.wrapX and a.markers == (1.e20, None) and a.static_markers == (None, None)
    assert a.shape == (2, 3, 4, 5) and a.dtype == numpy.float32 and a.statics == []
    b = FaceThickness(e3t, 'anomaly', st, st, st, wrapX=False, static_fill_value=-1.0, static_missing_value=0.0)
    assert b.code == 2 and len(b.statics) == 3 and not b.wrapX and b.static_markers == (-1.0, 0.0)
    with pytest.raises(RuntimeError, match="rule must be 'min'"):
        FaceThickness(e3t, 'max')
    with pytest.raises(RuntimeError, match="rule 'anomaly' needs the static thicknesses"):
        FaceThickness(e3t, 'anomaly', st, st)
    with pytest.raises(RuntimeError, match="go with rule 'anomaly' only"):
        FaceThickness(e3t, 'mean', e3u0=st)
    with pytest.raises(RuntimeError, match='works on torch CUDA tensors or DeviceArrays; e3t is not one'):
        face_thickness(st)
    with pytest.raises(RuntimeError, match="rule must be 'min'"):
        face_thickness(st, 'thin')
    with pytest.raises(RuntimeError, match="rule 'anomaly' needs"):
        face_thickness(st, 'anomaly')


def _bare_field(nt=2, nz=3, ny=4, nx=5, real='float32'):
    """a Field that holds what setCellThickness needs before the first device call"""
    from nemoflux_amd.field import Field
    f = Field.__new__(Field)
    f.nt, f.nz, f.ny, f.nx = nt, nz, ny, nx
    f._uv_code = NF_F32 if real == 'float32' else NF_F64
    f._h = ctypes.c_void_p()
    return f


def test_set_cell_thickness_refuses_before_it_needs_a_device():
    from nemoflux_amd.thickness import FaceThickness
    f = _bare_field()
    e3t = numpy.ones((2, 3, 4, 5), numpy.float32)
    st = numpy.ones((3, 4, 5), numpy.float64)
    with pytest.raises(RuntimeError, match='leave e3v None'):
        f.setCellThickness(FaceThickness(e3t), e3t)
    with pytest.raises(RuntimeError, match='carries the markers of e3t and of the statics itself'):
        f.setCellThickness(FaceThickness(e3t), fill_value=0.0)
    with pytest.raises(RuntimeError, match='carries the markers'):
        f.setCellThickness(FaceThickness(e3t), missing_value=0.0)
    with pytest.raises(RuntimeError, match='e3t has shape'):
        f.setCellThickness(FaceThickness(e3t[:, :2]))
    with pytest.raises(RuntimeError, match='e3t has shape'):
        f.setCellThickness(FaceThickness(numpy.ones((3, 3, 4, 5), numpy.float32)))
    with pytest.raises(RuntimeError, match='e3u0 has shape'):
        f.setCellThickness(FaceThickness(e3t, 'anomaly', st, numpy.ones((2, 3, 4, 5)), st))
    with pytest.raises(RuntimeError, match='e3t0 is int32'):
        f.setCellThickness(FaceThickness(e3t, 'anomaly', st.astype(numpy.int32), st, st))
    # today's words for the plain forms
    with pytest.raises(RuntimeError, match='needs both e3u and e3v'):
        f.setCellThickness(e3t)


def test_fluxplot_refuses_bad_e3t_options():
    from nemoflux_amd.fluxplot import cellThicknessSource
    files = ('T.npz', 'U.npz', 'V.npz')
    assert cellThicknessSource(False, *files) is None
    assert cellThicknessSource(True, *files, e3u='thku') == (('U.npz', 'thku'), ('V.npz', 'e3v'))
    for kw, words in ((dict(e3t='e3t', e3u='e3u'), 'cannot be combined with --e3u'),
                      (dict(e3t='e3t', e3FileV='x.nc'), 'cannot be combined with --e3u'),
                      (dict(e3tFile='x.nc'), 'need --e3t NAME'), (dict(e3Rule='mean'), 'need --e3t NAME'),
                      (dict(e3Static='m.nc'), 'need --e3t NAME'),
                      (dict(e3t='e3t', e3Rule='max'), 'must be min, mean or anomaly'),
                      (dict(e3t='e3t', e3Rule='anomaly'), 'go together'), (dict(e3t='e3t', e3Static='m.nc'), 'go together'),
                      (dict(e3t='e3t', e3Rule='anomaly', e3Static='m.nc:a,b'), 'three names')):
        with pytest.raises(RuntimeError, match=words):
            cellThicknessSource(True, *files, **kw)
    with pytest.raises(RuntimeError, match='--e3t needs --cell-thickness'):
        cellThicknessSource(False, *files, e3t='e3t')


# ---- 6. past one column chunk: what the wide inputs of the GPU tests can tell apart -------------------------------------------
WIDE = ref.wide_cases()
WIDE_IDS = [ref.wide_id(c) for c in WIDE]


def test_wide_shapes_reach_the_chunk_layouts_they_are_there_for():
    """from the launch code of nf_facethick.hip / nf_sshthick.hip: 256 lanes of VEC = 16 / itemsize values, of one value when a
    base is moved or nx is no multiple of VEC"""
    assert ref.boundary_columns(512, 8) == [255, 511] and ref.boundary_columns(514, 8) == [255, 511, 513]
    assert ref.boundary_columns(1026, 8) == [255, 511, 767, 1023, 1025] and ref.boundary_columns(515, 8) == [255, 511, 514]
    assert ref.boundary_columns(1028, 4) == [255, 511, 767, 1023, 1027] and ref.boundary_columns(72, 8) == [71]
    assert ref.boundary_columns(2052, 4) == [255, 511, 767, 1023, 1279, 1535, 1791, 2047, 2051]
    layouts = {}
    for real, shapes in ref.WIDE_SHAPES.items():
        size = numpy.dtype(real).itemsize
        for nz, ny, nx in shapes:
            layouts[real, nx] = [(v, ref.chunks_of(nx, v), ref.chunk_and_lane(nx - 1, v)) for v in
                                 (ref.lane_width(nx, size), ref.lane_width(nx, size, moved=True))]
    assert layouts['float64', 512] == [(2, 1, (0, 255)), (1, 2, (1, 255))]            # full: the wrap sits on lane 255
    assert layouts['float64', 514] == [(2, 2, (1, 0)), (1, 3, (2, 1))]                # a last chunk of one lane
    assert layouts['float64', 1026] == [(2, 3, (2, 0)), (1, 5, (4, 1))]
    assert layouts['float64', 515] == [(1, 3, (2, 2))] * 2
    assert layouts['float32', 1024] == [(4, 1, (0, 255)), (1, 4, (3, 255))]
    assert layouts['float32', 1028] == [(4, 2, (1, 0)), (1, 5, (4, 3))]
    assert layouts['float32', 2052] == [(4, 3, (2, 0)), (1, 9, (8, 3))]
    assert layouts['float32', 1027] == [(1, 5, (4, 2))] * 2
    assert all(nx <= 73 for _, _, nx in ref.SHAPES) and len(set(WIDE_IDS)) == len(WIDE) == 48
    assert 'float64-2x5x514-min-wrap-vec2x2+vec1x3' in WIDE_IDS and 'float32-2x5x1027-anomaly-nowrap-vec1x5' in WIDE_IDS


@pytest.mark.parametrize('case', WIDE, ids=WIDE_IDS)
def test_wide_restatement_equals_the_scalar_loop_on_two_rows(case):
    """the first level and two rows of every wide case: the wide expected values rest on the definition of the narrow ones"""
    real, nz, ny, nx, rule, wrap = case
    e3t, *statics = (None if a is None else numpy.ascontiguousarray(a[:1, :2]) for a in ref.case_arrays(case))
    u, v = ref.face_thickness(e3t, rule, *statics, wrap=wrap, markers=EM, static_markers=SM)
    lu, lv = ref.face_thickness_loop(e3t, rule, *statics, wrap=wrap, markers=EM, static_markers=SM)
    assert u.shape == (1, 2, nx) and u.dtype == numpy.dtype(real) and ref.same_bits(u, lu) and ref.same_bits(v, lv)


def _with_column(arrays, col, source):
    """the cell inputs (e3t, e3t0) with column col overwritten by column source; the face statics as they are"""
    out = [None if a is None else a.copy() for a in arrays]
    for a in out[:2]:
        if a is not None:
            a[..., col] = a[..., source]
    return out


@pytest.mark.parametrize('case', WIDE, ids=WIDE_IDS)
def test_wide_inputs_tell_a_wrong_east_neighbour_at_every_chunk_boundary(case):
    """a kernel that took column 0 for the east neighbour of a chunk's last column, in either lane form, would give other bits
    in that column; so would one that wrapped without wrapX, or did not wrap with it"""
    real, nz, ny, nx, rule, wrap = case
    arrays = ref.case_arrays(case)
    kw = dict(markers=EM, static_markers=SM)
    true = ref.face_thickness(*arrays[:1], rule, *arrays[1:], wrap=wrap, **kw)[0]
    cols = ref.boundary_columns(nx, numpy.dtype(real).itemsize)
    assert cols[-1] == nx - 1 and len(cols) >= 2
    for b in cols[:-1]:
        e3t, *statics = _with_column(arrays, b + 1, 0)
        wrong = ref.face_thickness(e3t, rule, *statics, wrap=wrap, **kw)[0]
        assert not ref.same_bits(wrong[..., b], true[..., b]), b
    other = ref.face_thickness(*arrays[:1], rule, *arrays[1:], wrap=not wrap, **kw)[0]
    assert not ref.same_bits(other[..., -1], true[..., -1]) and ref.same_bits(other[..., :-1], true[..., :-1])
    if not wrap:      # without wrapX column 0 is nothing to the last column
        e3t, *statics = _with_column(arrays, 0, nx // 2)
        assert not ref.same_bits(e3t[..., 0], arrays[0][..., 0])
        moved = ref.face_thickness(e3t, rule, *statics, wrap=False, **kw)[0]
        assert ref.same_bits(moved[..., -1], true[..., -1]) and not ref.same_bits(moved[..., 0], true[..., 0])


@pytest.mark.parametrize('rule', ['min', 'mean', 'anomaly'])
@pytest.mark.parametrize('real', ['float64', 'float32'])
def test_wide_boundary_columns_take_both_present_and_absent_branches(real, rule):
    taken = set()
    for case in WIDE:
        if case[0] == real and case[4] == ref.RULES[rule]:
            bu = _restated(case)[2]
            taken |= set(bu[..., ref.boundary_columns(case[3], numpy.dtype(real).itemsize)].reshape(-1).tolist())
    absent = set(ref.BRANCHES[ref.RULES[rule]]) - {ref.BOTH}
    assert ref.BOTH in taken and absent <= taken, taken
