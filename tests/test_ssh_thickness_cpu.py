"""z* thicknesses from the sea surface height (nf_column_depth, nf_ssh_thickness, nemoflux_amd.thickness, fluxplot --ssh), the part
that needs no GPU: the numpy restatement of tests/ssh_thickness_reference.py pinned bit for bit to a scalar Python loop on every
input set of the GPU tests, against closed forms, and through every fallback of the definition one by one; the tie to the
anomaly rule of nf_face_thickness on a flat bottom; the branches that the GPU tests' inputs take, and that the wide inputs
(past one column chunk) tell a wrong east neighbour at every chunk boundary; the two symbols exported,
declared and bound; every argument error the library decides before it needs a device; the Python argument checks of
ssh_thickness, SshThickness, Field.setCellThickness and fluxplot."""
import ctypes
import os
import re
import subprocess

import numpy
import pytest

from conftest import ROOT
import face_thickness_reference as fref
import ssh_thickness_reference as ref

NF_ERR_ARG = 1
NF_F64, NF_F32 = 0, 1
EM, SM = ref.EM, ref.SM
CASES = ref.raw_cases()
ARGS = {
    'nf_column_depth': ('double *h_out_dev, const void *e3_0_dev, long nz, long ny, long nx, int dtype, double fill0, '
                        'double missing0, void *hip_stream'),
    'nf_ssh_thickness': ('void *e3u_out_dev, void *e3v_out_dev, const void *ssh_dev, const void *e3u0_dev, '
                         'const void *e3v0_dev, const double *hu0_dev, const double *hv0_dev, const double *area_t_dev, '
                         'const double *area_u_dev, const double *area_v_dev, long nz, long ny, long nx, int dtype, int wrap_x, '
                         'double fill, double missing, double fill0, double missing0, void *hip_stream'),
}
BOUND = {
    'nf_column_depth': [ctypes.c_void_p] * 2 + [ctypes.c_long] * 3 + [ctypes.c_int] + [ctypes.c_double] * 2 + [ctypes.c_void_p],
    'nf_ssh_thickness': ([ctypes.c_void_p] * 10 + [ctypes.c_long] * 3 + [ctypes.c_int] * 2 + [ctypes.c_double] * 4 +
                         [ctypes.c_void_p]),
}


# ---- 1. the restatement is the scalar loop -------------------------------------------------------------------------------------
@pytest.mark.parametrize('case', CASES, ids=[ref.case_id(c) for c in CASES])
def test_restatement_equals_the_scalar_loop_bit_for_bit(case):
    ssh, e3u0, e3v0, kw = ref.case_inputs(case)
    u, v = ref.ssh_thickness(ssh, e3u0, e3v0, **kw)
    lu, lv = ref.ssh_thickness_loop(ssh, e3u0, e3v0, **kw)
    assert u.dtype == numpy.dtype(case[0]) and ref.same_bits(u, lu) and ref.same_bits(v, lv)
    for s in (e3u0, e3v0):
        assert ref.same_bits(ref.column_depth(s, SM), ref.column_depth_loop(s, SM))


@pytest.mark.parametrize('real', ['float64', 'float32'])
def test_restatement_equals_the_scalar_loop_on_the_field_series(real):
    for grid in ((72, 36), (73, 37)):
        c = ref.series(real, grid, 3, 7)
        for areas in (None, c['areas']):
            u, v = ref.ssh_thickness(c['ssh'], c['e3u0'], c['e3v0'], areas=areas, markers=EM, static_markers=SM)
            assert u.shape == (3, 7, grid[1], grid[0])
            lu, lv = ref.ssh_thickness_loop(c['ssh'][1], c['e3u0'], c['e3v0'], areas=areas, markers=EM, static_markers=SM)
            assert ref.same_bits(u[1], lu) and ref.same_bits(v[1], lv)


# ---- 2. closed forms --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('real', ['float64', 'float32'])
def test_zero_ssh_gives_the_statics(real):
    c = ref.make_case(real, 7, 9, 13, seed=3)
    zero = numpy.zeros((9, 13), real)
    for areas in (None, c['areas']):
        for depths in ((None, None), (c['hu0'], c['hv0'])):
            u, v = ref.ssh_thickness(zero, c['e3u0'], c['e3v0'], *depths, areas=areas, static_markers=SM)
            for got, F0 in ((u, c['e3u0']), (v, c['e3v0'])):
                assert numpy.array_equal(got, numpy.where(ref.present(F0, SM), F0, 0))


@pytest.mark.parametrize('real', ['float64', 'float32'])
def test_columns_that_sum_to_eight_are_exact(real):
    """statics and ssh on the lattice of 1/8, H = 8 in every wet column: F0 + F0 * s / 8 in numpy, every step exact"""
    ssh, e3u0, e3v0 = ref.flat_bottom_case(real, 5, 9, 13)
    for wrap in (True, False):
        u, v = ref.ssh_thickness(ssh, e3u0, e3v0, wrap=wrap, static_markers=SM)
        Se, Sn = fref._neighbours(ssh, wrap)
        for got, F0, Sb in ((u, e3u0, Se), (v, e3v0, Sn)):
            ok = ref.present(F0, SM)
            H = ref.column_depth(F0, SM)
            assert set(numpy.unique(H)) == {0.0, 8.0}
            s = 0.5 * (ssh.astype(numpy.float64) + Sb)
            F = F0.astype(numpy.float64)
            with numpy.errstate(all='ignore'):
                want = numpy.where(ok, F + F * s / 8., 0.0)
            assert numpy.array_equal(got, want.astype(real)) and numpy.array_equal(got.astype(numpy.float64), want)
            assert (got != numpy.where(ok, F0, 0)).mean() > 0.3


@pytest.mark.parametrize('real', ['float64', 'float32'])
def test_equal_power_of_two_areas_give_the_rows_without_areas(real):
    c = ref.make_case(real, 7, 9, 13, seed=4)
    plain = ref.ssh_thickness(c['ssh'], c['e3u0'], c['e3v0'], markers=EM, static_markers=SM)
    for a in (0.25, 1.0, 4096.0):
        areas = tuple(numpy.full((9, 13), a) for _ in range(3))
        got = ref.ssh_thickness(c['ssh'], c['e3u0'], c['e3v0'], areas=areas, markers=EM, static_markers=SM)
        assert ref.same_bits(got[0], plain[0]) and ref.same_bits(got[1], plain[1])


def test_the_volume_of_a_column_changes_by_the_face_height():
    """sum_k out[k] = H + s within (nz + 3) eps (H + |s|) per wet column: nz products and nz - 1 additions of the sum, the
    division, the addition of 1 -- the oracle-free check"""
    nz, ny, nx = 7, 12, 17
    rng = numpy.random.default_rng(8)
    e3u0, e3v0 = (rng.uniform(0.25, 4.0, (nz, ny, nx)) for _ in range(2))
    ssh = rng.uniform(-2.0, 2.0, (ny, nx))
    u, v = ref.ssh_thickness(ssh, e3u0, e3v0)
    Se, Sn = fref._neighbours(ssh, True)
    eps = numpy.finfo(numpy.float64).eps
    for got, F0, Sb in ((u, e3u0, Se), (v, e3v0, Sn)):
        H, s = ref.column_depth(F0), 0.5 * (ssh + Sb)
        err = numpy.abs(got.sum(axis=0) - (H + s))
        print('largest error / bound:', float((err / ((nz + 3) * eps * (H + numpy.abs(s)))).max()))
        assert (err <= (nz + 3) * eps * (H + numpy.abs(s))).all()


@pytest.mark.parametrize('real', ['float64', 'float32'])
def test_flat_bottom_tie_to_the_anomaly_rule(real):
    """every column the same levels, e3u0 = e3v0 = e3t0, e3t = e3t0 (1 + ssh / H): the anomaly rule of nf_face_thickness gives
    e3t0 + 0.5 (e3t0 ssh_a / H + e3t0 ssh_b / H), this rule e3t0 (1 + 0.5 (ssh_a + ssh_b) / H): the same within 4 eps"""
    nz, ny, nx = 6, 8, 11
    rng = numpy.random.default_rng(9)
    h = rng.uniform(0.5, 4.0, nz)
    e3t0 = numpy.ascontiguousarray(numpy.broadcast_to(h[:, None, None], (nz, ny, nx))).astype(real)
    ssh = rng.uniform(-2.0, 2.0, (ny, nx)).astype(real)
    H = ref.column_depth(e3t0)
    e3t = (e3t0.astype(numpy.float64) * (1.0 + ssh.astype(numpy.float64) / H)).astype(real)
    u, v = ref.ssh_thickness(ssh, e3t0, e3t0)
    au, av = fref.face_thickness(e3t, 'anomaly', e3t0, e3t0, e3t0)
    eps = numpy.finfo(real).eps
    for a, b in ((u, au), (v, av)):
        rel = numpy.abs(a.astype(numpy.float64) - b) / numpy.abs(b)
        print('largest relative difference in eps:', float(rel.max() / eps))
        assert rel.max() <= 4 * eps


# ---- 3. every fallback, one by one ------------------------------------------------------------------------------------------------
def _one(real, ssh, e3u0, e3v0=None, **kw):
    ssh = numpy.array(ssh, dtype=real)
    e3u0 = numpy.array(e3u0, dtype=real)
    e3v0 = e3u0.copy() if e3v0 is None else numpy.array(e3v0, dtype=real)
    kw.setdefault('markers', EM)
    kw.setdefault('static_markers', SM)
    for k in ('hu0', 'hv0'):
        if kw.get(k) is not None:
            kw[k] = numpy.array(kw[k], dtype=numpy.float64)
    if kw.get('areas') is not None:
        kw['areas'] = tuple(numpy.array(a, dtype=numpy.float64) for a in kw['areas'])
    u, v = ref.ssh_thickness(ssh, e3u0, e3v0, **kw)
    lu, lv = ref.ssh_thickness_loop(ssh, e3u0, e3v0, **kw)
    assert ref.same_bits(u, lu) and ref.same_bits(v, lv)
    return u, v


@pytest.mark.parametrize('real', ['float64', 'float32'])
def test_fallbacks_one_by_one(real):
    dt = numpy.dtype(real).type
    nan, inf = numpy.nan, numpy.inf
    zero_bits = dt(0.0).tobytes()
    st = [[[2.0, 2.0, 2.0, 2.0], [2.0, 2.0, 2.0, 2.0]], [[2.0, 2.0, 2.0, 2.0], [2.0, 2.0, 2.0, 2.0]]]      # H = 4 everywhere
    for bad in (ref.EFILL, ref.EMISSING, nan):
        # a marker, the other marker, NaN in Sa (cell 1) or Sb: the faces beside it keep the static thickness
        u, v = _one(real, [[1.0, bad, 2.0, 4.0], [1.0, 1.0, 2.0, 4.0]], st, wrap=False)
        assert u[0, 0, 0] == dt(2.0) and u[0, 0, 1] == dt(2.0) and v[0, 0, 1] == dt(2.0)
        assert u[0, 0, 2] == dt(2.0 * (1 + 3.0 / 4)) and v[0, 0, 2] == dt(2.0 * (1 + 2.0 / 4)) and v[0, 0, 3] == dt(4.0)
    # the markers of the statics are not markers of ssh
    u, _ = _one(real, [[ref.SMISSING, ref.SMISSING]], [[[2.0, 2.0]]])
    assert u[0, 0, 0] == dt(2.0 * (1 + ref.SMISSING / 2.0))
    # the last row has no north neighbour: Sb := Sa
    _, v = _one(real, [[1.0, 2.0], [2.0, nan]], [[[2.0, 2.0], [2.0, 2.0]]])
    assert v[0, 1, 0] == dt(4.0) and v[0, 1, 1] == dt(2.0) and v[0, 0, 0] == dt(2.0 * (1 + 1.5 / 2))
    # the last column: wrapX off takes its own value, wrapX on the first column
    ssh, F0 = [[1.0, 2.0, 3.0]], [[[4.0, 4.0, 4.0]]]
    assert _one(real, ssh, F0, wrap=False)[0][0, 0, 2] == dt(7.0) and _one(real, ssh, F0, wrap=True)[0][0, 0, 2] == dt(6.0)
    # F0 missing: +0.0 whatever ssh holds; the other levels of the column go on, H leaves the level out
    for bad in (ref.SFILL, ref.SMISSING, nan):
        u, _ = _one(real, [[2.0, 2.0]], [[[bad, 1.0]], [[4.0, 1.0]]], wrap=False)
        assert u[0, 0, 0].tobytes() == zero_bits and u[1, 0, 0] == dt(6.0) and u[0, 0, 1] == dt(2.0)
    # H == 0 (no present level; a column of zeros), a NaN H, a negative H: the factor is 1
    u, _ = _one(real, [[2.0, 2.0, 2.0]], [[[nan, 0.0, 3.0]]], wrap=False)
    assert u[0, 0, 0].tobytes() == zero_bits and u[0, 0, 1].tobytes() == zero_bits and u[0, 0, 2] == dt(5.0)
    for H in (0.0, nan, -2.0):
        u, v = _one(real, [[2.0, 2.0]], [[[3.0, 3.0]]], hu0=[[H, 4.0]], hv0=[[4.0, H]], wrap=False)
        assert list(u[0, 0]) == [dt(3.0), dt(4.5)] and list(v[0, 0]) == [dt(4.5), dt(3.0)]
    # areas: NEMO's weighted mean; a NaN area of either cell, a NaN, zero or negative face area: the factor is 1
    ssh, F0, H = [[1.0, 3.0]], [[[4.0, 4.0]]], [[4.0, 4.0]]
    one = [[1.0, 1.0]]
    u, v = _one(real, ssh, F0, hu0=H, hv0=H, areas=([[2.0, 4.0]], [[4.0, 1.0]], one), wrap=False)
    assert u[0, 0, 0] == dt(4.0 * (1 + (0.5 * (2.0 + 12.0) / 4.0) / 4)) and u[0, 0, 1] == dt(4.0 * (1 + 12.0 / 4))
    assert v[0, 0, 0] == dt(4.0 * (1 + 2.0 / 4)) and v[0, 0, 1] == dt(4.0 * (1 + 12.0 / 4))
    for at, au in (([[nan, 4.0]], one), ([[2.0, nan]], one), ([[2.0, 4.0]], [[nan, 1.0]]), ([[2.0, 4.0]], [[0.0, 1.0]]),
                   ([[2.0, 4.0]], [[-1.0, 1.0]])):
        u, _ = _one(real, ssh, F0, hu0=H, hv0=H, areas=(at, au, one), wrap=True)
        assert u[0, 0, 0] == dt(4.0)
    # one level, nx = 1: with wrapX the cell is its own east neighbour, without there is none -- the same
    for wrap in (True, False):
        u, v = _one(real, [[2.0]], [[[3.0]]], wrap=wrap)
        assert u[0, 0, 0] == dt(5.0) and v[0, 0, 0] == dt(5.0)
    # +-inf in ssh is present and is stored as it comes; inf - inf is NaN; negative results are stored as they come
    u, _ = _one(real, [[inf, -inf, 1.0, -9.0]], [[[2.0, 2.0, 2.0, 2.0]]], wrap=True)
    assert numpy.isnan(u[0, 0, 0]) and u[0, 0, 1] == dt(-inf) and u[0, 0, 2] == dt(-2.0) and u[0, 0, 3] == dt(inf)
    u, _ = _one(real, [[-9.0, -9.0]], [[[2.0, 2.0]]])
    assert u[0, 0, 0] == dt(-7.0)
    # float32 inputs are widened, the result rounded once
    if real == 'float32':
        a, b = numpy.float32(1.0), numpy.float32(1.0 + 2.0 ** -23)
        u, _ = _one(real, [[a, b]], [[[b, b]]], wrap=False)
        H = float(b)
        assert u[0, 0, 0] == numpy.float32(float(b) * (1.0 + (0.5 * (float(a) + float(b))) / H))


# ---- 4. the branches the GPU tests' inputs take ----------------------------------------------------------------------------------
@pytest.mark.parametrize('case', CASES, ids=[ref.case_id(c) for c in CASES])
def test_branch_shares_of_the_gpu_inputs(case):
    real, nz, ny, nx, areas, wrap, supplied = case
    ssh, e3u0, e3v0, kw = ref.case_inputs(case)
    u, v, bu, bv = ref.ssh_thickness(ssh, e3u0, e3v0, with_branches=True, **kw)
    if nx == 5:       # one launch of 5 columns: every branch by at least one face (every V face is without a neighbour)
        for b in ref.branches_of(case):
            assert bu[b].any() or bv[b].any(), b
        return
    for faces, name in ((bu, 'U'), (bv, 'V')):
        for b in ref.branches_of(case):
            if b == ref.NO_NEIGHBOUR and name == 'U' and wrap:
                assert not faces[b].any()
                continue
            assert faces[b].mean() >= 0.01, (name, b, faces[b].mean())
    for got, F0 in ((u, e3u0), (v, e3v0)):
        assert (got == 0).any() and (got != numpy.where(ref.present(F0, SM), F0, 0)).mean() > 0.1
        assert len(numpy.unique(got[numpy.isfinite(got)])) > 10
    if not supplied:      # some columns have no present level at all
        assert (ref.column_depth(e3u0, SM) == 0).mean() >= 0.01


def test_branch_shares_of_the_field_series():
    for grid in ((72, 36), (73, 37)):
        c = ref.series('float32', grid, 3, 7)
        _, _, bu, bv = ref.ssh_thickness(c['ssh'], c['e3u0'], c['e3v0'], areas=c['areas'], markers=EM, static_markers=SM,
                                         with_branches=True)
        for faces in (bu, bv):
            for b, m in faces.items():
                assert m.mean() >= 0.01 or (b == ref.NO_NEIGHBOUR and faces is bu), b


# ---- 5. the raw calls --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('name', sorted(ARGS))
def test_symbols_are_exported_declared_and_bound_with_one_argument_list(name):
    from nemoflux_amd import _lib
    with open(os.path.join(ROOT, 'include', 'nemoflux_amd.h')) as fh:
        header = re.sub(r'/\*.*?\*/', '', fh.read(), flags=re.S)
    out = subprocess.run(['nm', '-D', '--defined-only', _lib._SO], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0
    assert name in {ln.split()[-1] for ln in out.stdout.splitlines() if ln.split()}
    m = re.search(r'\bint\s+' + name + r'\s*\(([^)]*)\)\s*;', header)
    assert m, f'{name} is not declared in include/nemoflux_amd.h'
    assert ' '.join(m.group(1).split()) == ARGS[name]
    fn = getattr(_lib.lib, name)
    assert fn.restype is ctypes.c_int and list(fn.argtypes) == BOUND[name]
    with open(os.path.join(ROOT, 'nemoflux_amd', 'csrc', 'nf_sshthick.hip')) as fh:
        src = fh.read()
    m = re.search(r'extern "C" int ' + name + r'\s*\(([^)]*)\)', src)
    assert m and ' '.join(m.group(1).split()) == ARGS[name]
    assert 'k_ssh_thickness' in src and 'k_column_depth' in src and '__shared__' not in src and 'atomic' not in src.lower()
    with open(os.path.join(ROOT, 'nemoflux_amd', 'csrc', 'Makefile')) as fh:
        assert 'nf_sshthick.hip' in fh.read()


def test_argument_errors_are_decided_without_a_device():
    """every error listed in the header; the device pointers are never dereferenced (they are not device memory)"""
    from nemoflux_amd import _lib
    lib = _lib.lib
    U, V, S, U0, V0, HU, HV, AT, AU, AV = (k << 24 for k in range(1, 11))       # stand-ins for device addresses, 16 MiB apart
    nan = numpy.nan
    nbytes, pbytes = 3 * 4 * 5 * 8, 4 * 5 * 8

    def call(e3u=U, e3v=V, ssh=S, e3u0=U0, e3v0=V0, hu0=HU, hv0=HV, at=None, au=None, av=None, nz=3, ny=4, nx=5, dtype=NF_F64,
             wrap=1):
        return lib.nf_ssh_thickness(e3u, e3v, ssh, e3u0, e3v0, hu0, hv0, at, au, av, nz, ny, nx, dtype, wrap, nan, nan, nan, nan,
                                    None)

    ar = dict(at=AT, au=AU, av=AV)
    bad = [(dict(e3u=None), b'null'), (dict(e3v=None), b'null'), (dict(ssh=None), b'null'), (dict(e3u0=None), b'null'),
           (dict(e3v0=None), b'null'), (dict(hu0=None), b'null'), (dict(hv0=None), b'null'),
           (dict(at=AT), b'go together'), (dict(au=AU), b'go together'), (dict(av=AV), b'go together'),
           (dict(at=AT, au=AU), b'go together'), (dict(at=AT, av=AV), b'go together'), (dict(au=AU, av=AV), b'go together'),
           (dict(dtype=2), b'dtype'), (dict(dtype=-1), b'dtype'),
           (dict(nz=0), b'>= 1'), (dict(ny=0), b'>= 1'), (dict(nx=-4), b'>= 1'),
           (dict(nz=1 << 40, ny=1 << 40, nx=1 << 40), b'too large'),
           (dict(e3v=U), b'overlaps'), (dict(e3v=U + 8), b'overlaps'), (dict(e3u=V + nbytes - 8), b'overlaps'),
           (dict(e3u=U0), b'overlaps'), (dict(e3v=V0 - nbytes + 8), b'overlaps'), (dict(e3u=U0 + nbytes - 8), b'overlaps'),
           (dict(e3u=S), b'overlaps'), (dict(e3v=S + pbytes - 8), b'overlaps'), (dict(e3u=S - nbytes + 8), b'overlaps'),
           (dict(e3u=HU), b'overlaps'), (dict(e3v=HV + pbytes - 8), b'overlaps'), (dict(e3v=HV - nbytes + 8), b'overlaps'),
           (dict(e3u=AT, **ar), b'overlaps'), (dict(e3v=AU + 8, **ar), b'overlaps'), (dict(e3u=AV - 8, **ar), b'overlaps')]
    for kw, word in bad:
        assert call(**kw) == NF_ERR_ARG, kw
        err = lib.nf_last_error()
        assert word in err and err.startswith(b'nf_ssh_thickness:'), (kw, err)

    def depth(h=HU, e3=U0, nz=3, ny=4, nx=5, dtype=NF_F64):
        return lib.nf_column_depth(h, e3, nz, ny, nx, dtype, nan, nan, None)

    bad_depth = [(dict(h=None), b'null'), (dict(e3=None), b'null'), (dict(dtype=2), b'dtype'), (dict(dtype=-1), b'dtype'),
                 (dict(nz=0), b'>= 1'), (dict(ny=-1), b'>= 1'), (dict(nx=0), b'>= 1'),
                 (dict(nz=1 << 40, ny=1 << 40, nx=1 << 40), b'too large'),
                 (dict(h=U0), b'overlaps'), (dict(h=U0 + nbytes - 8), b'overlaps'), (dict(h=U0 - pbytes + 8), b'overlaps'),
                 (dict(h=U0 + nbytes // 2 - 8, dtype=NF_F32), b'overlaps')]
    for kw, word in bad_depth:
        assert depth(**kw) == NF_ERR_ARG, kw
        err = lib.nf_last_error()
        assert word in err and err.startswith(b'nf_column_depth:'), (kw, err)
    if _lib.device_count() == 0:
        # what is NOT an error goes on to need a device: ranges that only touch, areas, both dtypes
        for kw in (dict(), dict(e3u=V + nbytes), dict(e3v=S + pbytes), dict(e3u=HU - nbytes), dict(dtype=NF_F32, wrap=0, **ar),
                   dict(nz=1, ny=1, nx=1)):
            assert call(**kw) not in (0, NF_ERR_ARG), kw
            assert b'no usable AMD GPU' in lib.nf_last_error()
        for kw in (dict(), dict(h=U0 + nbytes), dict(h=U0 - pbytes), dict(h=U0 + nbytes // 2, dtype=NF_F32)):
            assert depth(**kw) not in (0, NF_ERR_ARG), kw
            assert b'no usable AMD GPU' in lib.nf_last_error()


# ---- Python ------------------------------------------------------------------------------------------------------------------------
def test_descriptor_and_raw_call_argument_checks():
    from nemoflux_amd.thickness import SshThickness, column_depth, ssh_thickness
    ssh = numpy.ones((2, 4, 5), numpy.float32)
    st = numpy.ones((3, 4, 5), numpy.float32)
    pl = numpy.ones((4, 5))
    a = SshThickness(ssh, st, st, fill_value=1.e20)
    assert a.wrapX and a.markers == (1.e20, None) and a.static_markers == (None, None) and not a.from_e3t0
    assert a.shape == (2, 4, 5) and a.dtype == numpy.float32 and len(a.statics) == 2 and a.depths is None and a.areas is None
    b = SshThickness(ssh, e3t0=st, hu0=pl, hv0=pl, areas=(pl, pl, pl), wrapX=False, static_fill_value=-1.0,
                     static_missing_value=0.0)
    assert b.from_e3t0 and len(b.statics) == 1 and not b.wrapX and b.static_markers == (-1.0, 0.0)
    assert len(b.depths) == 2 and len(b.areas) == 3 and b.areas[0].dtype == numpy.float64
    for kw, words in ((dict(e3u0=st, e3v0=st, e3t0=st), 'not both'), (dict(e3u0=st, e3t0=st), 'not both'),
                      (dict(e3u0=st), 'needs the static thicknesses'), (dict(), 'needs the static thicknesses'),
                      (dict(e3t0=st, hu0=pl), 'hu0 and hv0 go together'), (dict(e3t0=st, areas=(pl, pl)), 'areas must be'),
                      (dict(e3t0=st, areas=(pl, None, pl)), 'areas must be')):
        with pytest.raises(RuntimeError, match=words):
            SshThickness(ssh, **kw)
    with pytest.raises(RuntimeError, match='works on torch CUDA tensors or DeviceArrays; ssh is not one'):
        ssh_thickness(ssh[0], st, st)
    with pytest.raises(RuntimeError, match='hu0 and hv0 go together'):
        ssh_thickness(ssh[0], st, st, hu0=pl)
    with pytest.raises(RuntimeError, match='areas must be'):
        ssh_thickness(ssh[0], st, st, areas=(pl,))
    with pytest.raises(RuntimeError, match='out must be the pair'):
        ssh_thickness(ssh[0], st, st, out=st)
    with pytest.raises(RuntimeError, match='works on torch CUDA tensors or DeviceArrays; e3_0 is not one'):
        column_depth(st)


def test_more_than_two_static_markers_raise(tmp_path):
    from nemoflux_amd.thickness import SshThickness
    path = str(tmp_path / 'mesh.npz')
    st = numpy.ones((3, 4, 5), numpy.float32)
    numpy.savez(path, e3u_0=st, e3v_0=st, _FillValue_e3u_0=numpy.array(1.e20), _missing_value_e3u_0=numpy.array(-1.0),
                _FillValue_e3v_0=numpy.array(-2.0))
    with pytest.raises(RuntimeError, match='3 different _FillValue / missing_value markers'):
        SshThickness(numpy.ones((2, 4, 5), numpy.float32), (path, 'e3u_0'), (path, 'e3v_0'))


def test_set_cell_thickness_refuses_before_it_needs_a_device():
    from nemoflux_amd.thickness import SshThickness
    from test_face_thickness_cpu import _bare_field
    f = _bare_field()
    ssh = numpy.ones((2, 4, 5), numpy.float32)
    st = numpy.ones((3, 4, 5), numpy.float64)
    pl = numpy.ones((4, 5))
    with pytest.raises(RuntimeError, match='leave e3v None'):
        f.setCellThickness(SshThickness(ssh, st, st), ssh)
    with pytest.raises(RuntimeError, match='carries the markers of ssh and of the statics itself'):
        f.setCellThickness(SshThickness(ssh, st, st), fill_value=0.0)
    with pytest.raises(RuntimeError, match='carries the markers'):
        f.setCellThickness(SshThickness(ssh, st, st), missing_value=0.0)
    with pytest.raises(RuntimeError, match='ssh has shape'):
        f.setCellThickness(SshThickness(ssh[:, :2], st, st))
    with pytest.raises(RuntimeError, match='ssh has shape'):
        f.setCellThickness(SshThickness(numpy.ones((3, 4, 5), numpy.float32), st, st))
    with pytest.raises(RuntimeError, match='ssh is float64'):
        f.setCellThickness(SshThickness(ssh.astype(numpy.float64), st, st))
    with pytest.raises(RuntimeError, match='e3v0 has shape'):
        f.setCellThickness(SshThickness(ssh, st, numpy.ones((2, 3, 4, 5))))
    with pytest.raises(RuntimeError, match='e3t0 is int32'):
        f.setCellThickness(SshThickness(ssh, e3t0=st.astype(numpy.int32)))
    with pytest.raises(RuntimeError, match='hv0 has shape'):
        f.setCellThickness(SshThickness(ssh, st, st, hu0=pl, hv0=pl[:3]))
    with pytest.raises(RuntimeError, match=r'areas\[1\] has shape'):
        f.setCellThickness(SshThickness(ssh, st, st, areas=(pl, pl[:, :2], pl)))
    assert f._e3 is None


def test_fluxplot_refuses_bad_ssh_options():
    from nemoflux_amd.fluxplot import cellThicknessSource
    files = ('T.npz', 'U.npz', 'V.npz')
    assert cellThicknessSource(False, *files) is None
    assert cellThicknessSource(True, *files, e3u='thku') == (('U.npz', 'thku'), ('V.npz', 'e3v'))
    for kw, words in ((dict(ssh='zos', e3t='e3t', e3Static='m.nc'), 'cannot be combined with --e3t'),
                      (dict(ssh='zos', e3u='e3u', e3Static='m.nc'), 'cannot be combined with --e3t'),
                      (dict(ssh='zos', e3v='e3v', e3Static='m.nc'), 'cannot be combined with --e3t'),
                      (dict(ssh='zos', e3Rule='min', e3Static='m.nc'), 'cannot be combined with --e3t'),
                      (dict(ssh='zos'), 'needs --e3-static'),
                      (dict(sshFile='x.nc'), 'need --ssh NAME'), (dict(e3Areas='a,b,c'), 'need --ssh NAME'),
                      (dict(ssh='zos', e3Static='m.nc:a,b,c'), 'two names'),
                      (dict(ssh='zos', e3Static='m.nc', e3Areas='a,b'), 'three names'),
                      # --e3t keeps its words
                      (dict(e3Static='m.nc'), 'need --e3t NAME'), (dict(e3t='e3t', e3Rule='anomaly'), 'go together')):
        with pytest.raises(RuntimeError, match=words):
            cellThicknessSource(True, *files, **kw)
    with pytest.raises(RuntimeError, match='--ssh needs --cell-thickness'):
        cellThicknessSource(False, *files, ssh='zos', e3Static='m.nc')


def _packed_bundle(tmp_path, c, nt_static=False):
    """an .npz bundle whose ssh, statics and column depths are int16 with a scale_factor of 1/8 (every value of the lattice is
    exact) and a _FillValue of -32768: (path, the decoded arrays: masked values NaN)"""
    path = str(tmp_path / 'packed.npz')
    raw, want, attrs = {}, {}, {}
    for name, a in (('zos', c['ssh'][1] if nt_static else c['ssh']), ('e3u_0', c['e3u0']), ('e3v_0', c['e3v0']),
                    ('hu_0', c['hu0'])):
        a = numpy.asarray(a, numpy.float64)
        bad = ~numpy.isfinite(a) | (numpy.abs(a) > 4000)
        raw[name] = numpy.where(bad, -32768, numpy.where(bad, 0, a) * 8).astype(numpy.int16)
        want[name] = numpy.where(bad, numpy.nan, a).astype(numpy.float32)
        attrs['_scale_factor_' + name] = numpy.array(0.125, numpy.float32)
        attrs['_FillValue_' + name] = numpy.array(-32768, numpy.int16)
    numpy.savez(path, **raw, **attrs)
    return path, want


@pytest.mark.parametrize('static', [False, True])
def test_packed_file_variables_are_decoded_once(tmp_path, static):
    """a packed variable of fewer than four dimensions decodes whole whatever step is asked for: ssh and the planes become host
    arrays when the descriptor is made, a packed static stays one read_step(0) away from its (nz, ny, nx) array"""
    from nemoflux_amd.thickness import SshThickness
    c = ref.series('float32', (13, 9), 3, 4)
    path, want = _packed_bundle(tmp_path, c, static)
    st = SshThickness((path, 'zos'), (path, 'e3u_0'), (path, 'e3v_0'), hu0=(path, 'hu_0'), hv0=(path, 'hu_0'))
    assert isinstance(st.ssh, numpy.ndarray) and st.dtype == numpy.float32 and st.shape == want['zos'].shape
    assert ref.same_bits(st.ssh, want['zos']) and numpy.isnan(st.ssh).any() and st.markers == (None, None)
    assert st.depths[0].dtype == numpy.float64 and st.depths[0].shape == (9, 13)
    assert numpy.array_equal(st.depths[0], want['hu_0'].astype(numpy.float64), equal_nan=True)
    for a, name in zip(st.statics, ('e3u_0', 'e3v_0')):
        assert tuple(a.shape) == (4, 9, 13)
        whole = a.read_step(0) if hasattr(a, 'read_step') else numpy.asarray(a)
        assert ref.same_bits(numpy.asarray(whole, numpy.float32), want[name])
    assert st.static_markers == (None, None)


def test_fluxplot_refuses_one_static_name_and_checks_up_front():
    from nemoflux_amd import fluxplot
    with pytest.raises(RuntimeError, match='two names'):
        fluxplot.checkSshArgs(True, ssh='zos', e3Static='m.nc:e3u_0')
    with pytest.raises(RuntimeError, match='two names'):
        fluxplot.cellThicknessSource(True, 'T.npz', 'U.npz', 'V.npz', ssh='zos', e3Static='m.nc:e3u_0,')
    assert fluxplot.checkSshArgs(True, ssh='zos', e3Static='dir/m.nc') == ('dir/m.nc', ['e3u_0', 'e3v_0'], None)
    assert fluxplot.checkSshArgs(True, ssh='zos', e3Static='m.nc:a,b', e3Areas='x,y,z') == ('m.nc', ['a', 'b'], ['x', 'y', 'z'])
    assert fluxplot.checkSshArgs(False) is None
    # main refuses before it reads a file, whatever product is asked for
    for kw in (dict(ssh='zos'), dict(sshFile='x.nc'), dict(ssh='zos', e3Static='m.nc', e3t='e3t', cellThickness=True),
               dict(e3Areas='a,b,c', classes='1,2', tracer='thetao')):
        with pytest.raises(RuntimeError, match='--ssh'):
            fluxplot.main(tFile='none_T.npz', uFile='none_U.npz', vFile='none_V.npz', lonLatPoints='[(0,0),(1,1)]', **kw)


# ---- past one column chunk: what the wide inputs of the GPU tests can tell apart ----------------------------------------------
WIDE = ref.wide_cases()
WIDE_IDS = [ref.wide_id(c) for c in WIDE]


def test_wide_cases_are_the_wide_shapes_of_the_face_kernel():
    assert ref.WIDE_SHAPES is fref.WIDE_SHAPES and all(nx <= 73 for _, _, nx in ref.SHAPES)
    assert len(set(WIDE_IDS)) == len(WIDE) == 64
    assert 'float64-9x6x1026-areas-wrap-computed-vec2x3+vec1x5' in WIDE_IDS
    assert 'float32-2x5x1027-plain-nowrap-supplied-vec1x5' in WIDE_IDS
    # nz = 9 is a full group of the kernel's 8 levels and a last one of 1
    assert {nz for shapes in ref.WIDE_SHAPES.values() for nz, _, _ in shapes} == {2, 9}


def _two_rows(kw):
    kw = dict(kw)
    for k in ('hu0', 'hv0'):
        kw[k] = None if kw[k] is None else numpy.ascontiguousarray(kw[k][:2])
    kw['areas'] = None if kw['areas'] is None else tuple(numpy.ascontiguousarray(a[:2]) for a in kw['areas'])
    return kw


@pytest.mark.parametrize('case', WIDE, ids=WIDE_IDS)
def test_wide_restatement_equals_the_scalar_loop_on_two_rows(case):
    """the first level and two rows of every wide case: the wide expected values rest on the definition of the narrow ones"""
    ssh, e3u0, e3v0, kw = ref.case_inputs(case)
    ssh, e3u0, e3v0 = (numpy.ascontiguousarray(a) for a in (ssh[:2], e3u0[:1, :2], e3v0[:1, :2]))
    kw = _two_rows(kw)
    u, v = ref.ssh_thickness(ssh, e3u0, e3v0, **kw)
    lu, lv = ref.ssh_thickness_loop(ssh, e3u0, e3v0, **kw)
    assert u.shape == (1, 2, case[3]) and u.dtype == numpy.dtype(case[0]) and ref.same_bits(u, lu) and ref.same_bits(v, lv)
    for s in (e3u0, e3v0):
        assert ref.same_bits(ref.column_depth(s, SM), ref.column_depth_loop(s, SM))


def _with_column(ssh, kw, col, source):
    """the cell inputs (ssh, area_t) with column col overwritten by column source; what belongs to the faces as it is"""
    ssh, kw = ssh.copy(), dict(kw)
    ssh[..., col] = ssh[..., source]
    if kw['areas'] is not None:
        at = kw['areas'][0].copy()
        at[..., col] = at[..., source]
        kw['areas'] = (at,) + tuple(kw['areas'][1:])
    return ssh, kw


@pytest.mark.parametrize('case', WIDE, ids=WIDE_IDS)
def test_wide_inputs_tell_a_wrong_east_neighbour_at_every_chunk_boundary(case):
    """a kernel that took column 0 for the east neighbour of a chunk's last column, in either lane form, would give other bits
    in that column; so would one that wrapped without wrapX, or did not wrap with it"""
    real, nz, ny, nx, areas, wrap, supplied = case
    ssh, e3u0, e3v0, kw = ref.case_inputs(case)
    true = ref.ssh_thickness(ssh, e3u0, e3v0, **kw)[0]
    cols = ref.boundary_columns(nx, numpy.dtype(real).itemsize)
    assert cols[-1] == nx - 1 and len(cols) >= 2
    for b in cols[:-1]:
        s, k = _with_column(ssh, kw, b + 1, 0)
        wrong = ref.ssh_thickness(s, e3u0, e3v0, **k)[0]
        assert not ref.same_bits(wrong[..., b], true[..., b]), b
    other = ref.ssh_thickness(ssh, e3u0, e3v0, **dict(kw, wrap=not wrap))[0]
    assert not ref.same_bits(other[..., -1], true[..., -1]) and ref.same_bits(other[..., :-1], true[..., :-1])
    if not wrap:      # without wrapX column 0 is nothing to the last column
        s, k = _with_column(ssh, kw, 0, nx // 2)
        assert not ref.same_bits(s[..., 0], ssh[..., 0])
        moved = ref.ssh_thickness(s, e3u0, e3v0, **k)[0]
        assert ref.same_bits(moved[..., -1], true[..., -1]) and not ref.same_bits(moved[..., 0], true[..., 0])


@pytest.mark.parametrize('areas', [False, True], ids=['plain', 'areas'])
@pytest.mark.parametrize('real', ['float64', 'float32'])
def test_wide_boundary_columns_take_both_present_and_absent_branches(real, areas):
    taken = set()
    for case in WIDE:
        if case[0] == real and case[4] == areas:
            ssh, e3u0, e3v0, kw = ref.case_inputs(case)
            bu = ref.ssh_thickness(ssh, e3u0, e3v0, with_branches=True, **kw)[2]
            cols = ref.boundary_columns(case[3], numpy.dtype(real).itemsize)
            taken |= {b for b, m in bu.items() if m[..., cols].any()}
    assert set(ref.branches_of((real, 0, 0, 0, areas, False, False))) <= taken, taken
