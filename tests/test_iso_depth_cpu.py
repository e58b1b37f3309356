"""Isosurface and mixed-layer depths (nf_iso_depth, nemoflux_amd.surfaces, fluxplot --iso-depth / --mixed-layer), the part that
needs no GPU: the numpy restatement of tests/iso_depth_reference.py pinned bit for bit to a scalar Python loop on every input
set of the GPU tests, against closed forms, and through every fallback of the definition one by one; the branches that the GPU
tests' inputs take; the symbol exported, declared and bound; every argument error the library decides before it needs a device;
the Python and fluxplot refusals.

Branch coverage.  The definition has the outcomes dry, sea bed, outcrop (k* = 0), interpolated and exactly on a level (tau_k*
== theta); each that a case's setting has is taken in 1 % to 60 % of the columns for every one of the m values, in every case,
the launches of 5 columns included (made by hand: one column in five per branch).  Two settings lack branches by the
definition itself: with one level there is no level above k*, so only dry, sea bed and outcrop exist; with relative = 1 the
search starts at kref + 1 >= 1, so there is no outcrop (and with one level kref = kb: only dry and sea bed).  The sixth
outcome, "at zref" (R at kref, relative = 1 only), needs tau_kref and tau_{kref+1} both past tau_ref + delta while tau_ref lies
between them, which only an offset <= 0 allows: the shared value sets hold offsets > 0 only and take it in the few columns with +inf at level kref alone, and a case of its
own (ref.atzref_case, also run on the GPU) holds offsets <= 0 and is asserted to take it."""
import ctypes
import os
import re
import subprocess
import sys

import numpy
import pytest

from conftest import ROOT
import iso_depth_reference as ref

NF_ERR_ARG = 1
NF_F64, NF_F32 = 0, 1
EPS = numpy.finfo(numpy.float64).eps
MARKS = dict(tau_markers=(ref.TFILL, ref.TMISSING), e3t_markers=(ref.EFILL, ref.EMISSING))
CASES = ref.raw_cases()


@pytest.mark.parametrize('case', CASES, ids=[ref.case_id(c) for c in CASES])
def test_restatement_is_the_scalar_loop_bit_for_bit_on_the_gpu_tests_inputs(case):
    real, nz, ny, nx, m, sense, relative, form = case
    tau, thk, e3t, values = ref.make_case(*case)
    kw = dict(thickness=thk, e3t=e3t, top=0.0, relative=relative, zref=ref.ZREF, fill_out=-5.0, **MARKS)
    got = ref.iso_depth(tau, values, sense, **kw)
    want = ref.iso_depth_scalar(tau, values, sense, **kw)
    assert got.shape == (m, ny, nx) and got.dtype == numpy.dtype(real)
    assert ref.same_bits(got, want)


@pytest.mark.parametrize('case', CASES, ids=[ref.case_id(c) for c in CASES])
def test_the_gpu_tests_inputs_take_every_branch(case):
    """every branch that the case's setting has, in 1 % to 60 % of the columns, for every one of the m values"""
    real, nz, ny, nx, m, sense, relative, form = case
    out, br = ref.case_reference(*case, with_branches=True)
    share = numpy.array([[(br[j] == b).mean() for b in range(6)] for j in range(m)])      # (value, branch)
    print(ref.case_id(case), numpy.round(100 * share, 1).tolist())
    if nz == 1:
        exist = [ref.DRY, ref.BED] if relative else [ref.DRY, ref.BED, ref.OUTCROP]
    elif relative:
        exist = [ref.DRY, ref.BED, ref.INTERP, ref.EXACT]
    else:
        exist = [ref.DRY, ref.BED, ref.OUTCROP, ref.INTERP, ref.EXACT]
    s = share[:, exist]
    assert ((s >= 0.01) & (s <= 0.60)).all()
    # what the setting lacks is never taken -- but for 'at zref' in relative mode, which a +inf at level kref reaches with any
    # offset: the few columns with +-inf in the tracer, under 1 %
    absent = [b for b in range(6) if b not in exist and not (relative and nz > 1 and b == ref.ATZREF)]
    assert (share[:, absent] == 0).all() and (share[:, ref.ATZREF] < 0.01).all()


@pytest.mark.parametrize('sense', [1, -1])
@pytest.mark.parametrize('real', ['float64', 'float32'])
def test_the_at_zref_case_takes_its_branch(real, sense):
    """offsets <= 0 in relative mode, the one setting in which level kref itself can have passed the threshold: 'at zref' in at
    least 1 % of the columns for each of them, next to interpolated columns; for the offset > 0 only where +inf sits at level kref"""
    tau, e3t, values = ref.atzref_case(real, 37, 73, sense)
    kw = dict(e3t=e3t, relative=True, zref=ref.ZREF, **MARKS)
    out, br = ref.iso_depth(tau, values, sense, with_branches=True, **kw)
    assert ref.same_bits(out, ref.iso_depth_scalar(tau, values, sense, **kw))
    share = numpy.array([[(br[j] == b).mean() for b in range(6)] for j in range(3)])
    print(numpy.round(100 * share, 1).tolist())
    assert (share[:2, ref.ATZREF] >= 0.01).all() and share[2, ref.ATZREF] < 0.01
    assert (share[:, ref.INTERP] >= 0.01).all() and (share[:, ref.OUTCROP] == 0).all()


def _lattice_columns(n, nz, seed):
    """thicknesses on the lattice of multiples of 1/8 and the exactly representable profile tau = 2 c + 1"""
    rng = numpy.random.default_rng(seed)
    h = rng.integers(1, 80, (nz, n)) / 8.0
    D = numpy.concatenate([numpy.zeros((1, n)), numpy.cumsum(h, axis=0)])
    c = 0.5 * (D[:-1] + D[1:])
    return h, D, c, 2.0 * c + 1.0


@pytest.mark.parametrize('real', ['float64', 'float32'])
def test_closed_form_of_a_linear_profile(real):
    """tau = 2 c + 1: the surface of theta lies at (theta - 1) / 2 wherever that is between c_0 and c_kb, to 4 eps x the column
    depth: the quotient, the product and the sum of the interpolation round once each, each to half an eps of a number that is
    at most the column depth -- three roundings, 1.5 eps, and the margin to 4 is for the rounding of the quotient being scaled
    by c_k - c_a.  At float32 the result is rounded once more, to float32, which alone is half a float32 eps of the depth: the
    bar there is one float32 eps x the column depth, the 4 float64 eps being far inside it"""
    nz, n = 9, 500
    h, D, c, tau = _lattice_columns(n, nz, 5)
    assert (tau.astype(real) == tau).all() and (h.astype(real) == h).all()
    theta = [7.3, 41.0, 70.5, 90.77]
    for form in ('levels', 'e3t'):
        if form == 'levels':        # one column, its thicknesses as the level vector
            DD, cc, tt = D[:, :1], c[:, :1], tau[:, :1]
            thick = dict(thickness=h[:, 0])
        else:
            DD, cc, tt = D, c, tau
            thick = dict(e3t=h.astype(real))
        got = ref.iso_depth(tt.astype(real), theta, +1, **thick)
        for j, th in enumerate(theta):
            z = (th - 1.0) / 2.0
            inside = (z > cc[0]) & (z <= cc[-1])
            assert inside.sum() > (20 if form == 'e3t' else 0) or form == 'levels'
            tol = 4 * EPS * DD[-1] if real == 'float64' else numpy.finfo(numpy.float32).eps * DD[-1]
            assert (numpy.abs(got[j].astype(numpy.float64) - z)[inside] <= tol[inside]).all(), (form, th)
            assert (got[j][z <= cc[0]] == 0.0).all() and (got[j][z > cc[-1]] == DD[-1][z > cc[-1]].astype(real)).all()
        # a falling tracer: the mirror image
        got2 = ref.iso_depth((-tt).astype(real), [-x for x in theta], -1, **thick)
        assert ref.same_bits(got, got2)


def test_closed_form_in_relative_mode():
    """the same profile with thresholds relative to the value at zref: tau_ref = 2 zref + 1 (up to rounding), so the surface of
    delta lies at zref + delta / 2, to the same bar, 4 eps x the column depth"""
    nz, n = 9, 500
    h, D, c, tau = _lattice_columns(n, nz, 6)
    for zref in (10.0, 33.3):
        for delta in (0.5, 3.0, 17.25):
            got = ref.iso_depth(tau, [delta], +1, e3t=h, relative=True, zref=zref)[0]
            z = zref + delta / 2.0
            inside = (zref > c[0]) & (z <= c[-1])
            assert inside.sum() > 50
            assert (numpy.abs(got - z)[inside] <= (4 * EPS * D[-1])[inside]).all(), (zref, delta)


def _one(tau, values, sense=+1, **kw):
    """one column through both restatements"""
    tau = numpy.asarray(tau, numpy.float64).reshape(-1, 1, 1)
    if 'e3t' in kw:
        kw['e3t'] = numpy.asarray(kw['e3t'], numpy.float64).reshape(-1, 1, 1)
    a = ref.iso_depth(tau, values, sense, **kw)
    b = ref.iso_depth_scalar(tau, values, sense, **kw)
    assert ref.same_bits(a, b)
    return [float(x) for x in a[:, 0, 0]]


def test_every_fallback_one_by_one():
    nan, inf = numpy.nan, numpy.inf
    h = [4.0, 12.0, 8.0, 8.0]                        # D = 0 4 16 24 32, c = 2 10 20 28
    tau = [1.0, 3.0, 5.0, 9.0]
    lev = dict(thickness=h, top=0.0)
    # interpolated, both senses; top moves everything
    assert _one(tau, [4.0], **lev) == [15.0]
    assert _one([-x for x in tau], [-4.0], -1, **lev) == [15.0]
    assert _one(tau, [4.0], thickness=h, top=100.0) == [115.0]
    # a dry column: the fill, for every value
    for first in (nan, -999.0, 1.e20):
        assert _one([first, 3.0, 5.0, 9.0], [4.0, 0.5], tau_markers=(-999.0, 1.e20), fill_out=-1.0, **lev) == [-1.0, -1.0]
    assert numpy.isnan(_one([nan] * 4, [4.0], **lev)[0])
    assert _one(tau, [4.0], e3t=[0.0, 12.0, 8.0, 8.0], fill_out=-2.0) == [-2.0]
    # the column ends at a marker, at a NaN, at a zero, negative, missing, NaN or infinite e3t: what lies below is not seen
    for bad in (-999.0, 1.e20, nan):
        assert _one([1.0, 3.0, bad, 9.0], [4.0, 2.0], tau_markers=(-999.0, 1.e20), **lev) == [16.0, 6.0]
    for bad in (0.0, -8.0, -999.0, 5.e15, nan, inf):
        assert _one(tau, [4.0, 2.0], e3t=[4.0, 12.0, bad, 8.0], e3t_markers=(-999.0, 5.e15)) == [16.0, 6.0]
    # nz = 1: outcrop or sea bed
    assert _one([5.0], [4.0, 5.0, 6.0], thickness=[7.0]) == [0.0, 0.0, 7.0]
    assert _one([5.0], [1.0], thickness=[7.0], relative=True, zref=2.0) == [7.0]
    # an outcrop; the value never reached; tau_k == theta exactly (R_k true by equality, the fraction is exactly 1)
    assert _one(tau, [1.0, 0.5], **lev) == [0.0, 0.0]
    assert _one(tau, [9.5], **lev) == [32.0]
    assert _one(tau, [5.0, 9.0], **lev) == [20.0, 28.0]
    # what lies below k* does not matter
    assert _one([1.0, 3.0, 5.0, -7.0], [4.0], **lev) == [15.0]
    # relative mode.  zref = 10 = c_1: kref = 1, tau_ref = tau_1 + (tau_2 - tau_1) * 0 = 3; delta = 1: theta = 4 at 15
    assert _one(tau, [1.0], relative=True, zref=10.0, **lev) == [15.0]
    # zref between c_1 and c_2: tau_ref = 3 + 2 * (5 / 10) = 4, theta = 4.5 between levels 1 and 2 at 10 + 10 * 0.75
    assert _one(tau, [0.5], relative=True, zref=15.0, **lev) == [17.5]
    # a delta <= 0 on a rising profile: theta = 3.5 and 4 lie between levels 1 and 2 above zref, R at kref is false
    assert _one(tau, [-0.5, 0.0], relative=True, zref=15.0, **lev) == [12.5, 15.0]
    # R at kref: a uniform layer around zref, tau_ref = 3; with delta <= 0 level kref has reached theta already: zref itself
    assert _one([1.0, 3.0, 3.0, 9.0], [0.0, -0.5], relative=True, zref=15.0, **lev) == [15.0, 15.0]
    # zref above c_0: kref = 0, tau_ref = tau_0, the search starts at level 1
    assert _one(tau, [1.0], relative=True, zref=1.0, **lev) == [2.0 + 8.0 * 0.5]
    assert _one(tau, [0.0], relative=True, zref=2.0, **lev) == [2.0]          # zref == c_0, R_0 by equality: zref
    # zref below c_kb: kref = kb, nothing left to search: the sea bed
    assert _one(tau, [0.5], relative=True, zref=30.0, **lev) == [32.0]
    assert _one([1.0, 3.0, nan, 9.0], [0.5], relative=True, zref=15.0, **lev) == [16.0]
    # +-inf in the tracer: stored as it comes
    assert _one([1.0, inf, 5.0, 9.0], [4.0], **lev) == [2.0]                  # 2 + 8 * (3 / inf)
    assert numpy.isnan(_one([-inf, inf, 5.0, 9.0], [4.0], **lev)[0])          # (4 + inf) / (inf + inf)
    assert _one([inf, 3.0, 5.0, 9.0], [4.0], **lev) == [0.0]                  # +inf has reached every value: outcrop
    assert numpy.isnan(_one([1.0, 3.0, -inf, 9.0], [4.0], **lev)[0])          # level 3 reaches: (4 + inf) / (9 + inf)


# ---- ABI ---------------------------------------------------------------------------------------------------------------------
ARGS = ('void *out_dev, const void *tau_dev, const double *thickness_host, const void *e3t_dev, long nz, long ny, long nx, '
        'int dtype, double tau_fill, double tau_missing, double e3t_fill, double e3t_missing, double top, const double *values, '
        'int m, int sense, int relative, double zref, double fill_out, void *hip_stream')
C_TYPES = [('void *', ctypes.c_void_p), ('const void *', ctypes.c_void_p), ('const double *', ctypes.POINTER(ctypes.c_double)),
           ('long ', ctypes.c_long), ('int ', ctypes.c_int), ('double ', ctypes.c_double)]


def test_symbol_is_exported_declared_and_bound_with_one_argument_list():
    from nemoflux_amd import _lib
    with open(os.path.join(ROOT, 'include', 'nemoflux_amd.h')) as fh:
        header = re.sub(r'/\*.*?\*/', '', fh.read(), flags=re.S)
    out = subprocess.run(['nm', '-D', '--defined-only', _lib._SO], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stderr
    assert 'nf_iso_depth' in {ln.split()[-1] for ln in out.stdout.splitlines() if ln.split()}
    m = re.search(r'\bint\s+nf_iso_depth\s*\(([^)]*)\)\s*;', header)
    assert m, 'nf_iso_depth is not declared in include/nemoflux_amd.h'
    declared = ' '.join(m.group(1).split())
    assert declared == ARGS, declared
    want = [next(v for k, v in C_TYPES if a.strip().startswith(k)) for a in declared.split(',')]
    fn = _lib.lib.nf_iso_depth
    assert fn.restype is ctypes.c_int and list(fn.argtypes) == want, fn.argtypes
    with open(os.path.join(ROOT, 'nemoflux_amd', 'csrc', 'nf_isodepth.hip')) as fh:
        src = fh.read()
    m = re.search(r'extern "C" int nf_iso_depth\s*\(([^)]*)\)', src)
    assert m and ' '.join(m.group(1).split()) == ARGS
    assert 'k_iso_depth' in src and '__shared__' not in src and 'atomic' not in src.lower().replace('no atomics', '')
    with open(os.path.join(ROOT, 'nemoflux_amd', 'csrc', 'Makefile')) as fh:
        assert re.search(r'^SRCS = .*\bnf_isodepth\.hip\b', fh.read(), flags=re.M)


def test_argument_errors_are_decided_without_a_device():
    """every error listed in the header; the device pointers are never dereferenced (they are not device memory)"""
    from nemoflux_amd import _lib
    lib = _lib.lib
    O, T, E = 1 << 24, 2 << 24, 3 << 24            # stand-ins for device addresses, 16 MiB apart
    nan, inf = numpy.nan, numpy.inf
    NZ, NY, NX = 7, 10, 20                          # tau: 11200 bytes at float64; out with m = 3: 4800 bytes
    dp = ctypes.POINTER(ctypes.c_double)

    def call(out=O, tau=T, h=tuple([2.0] * NZ), e3t=None, nz=NZ, ny=NY, nx=NX, dtype=NF_F64, top=0.0, values=(1.0, 2.0, 3.0),
             m=None, sense=1, relative=0, zref=10.0):
        hp = None if h is None else (ctypes.c_double * len(h))(*h)
        vp = None if values is None else (ctypes.c_double * max(len(values), 1))(*values)
        return lib.nf_iso_depth(out, tau, ctypes.cast(hp, dp) if hp is not None else None, e3t, nz, ny, nx, dtype, nan, nan, nan,
                                nan, top, ctypes.cast(vp, dp) if vp is not None else None, len(values or ()) if m is None else m,
                                sense, relative, zref, nan, None)

    nine = tuple(float(x) for x in range(9))
    for kw, word in ((dict(out=None), b'null'), (dict(tau=None), b'null'), (dict(values=None, m=3), b'null'),
                     (dict(e3t=E), b'exactly one'), (dict(h=None), b'exactly one'),
                     (dict(values=(), m=0), b'm must be'), (dict(values=nine), b'm must be'), (dict(m=-1), b'm must be'),
                     (dict(dtype=2), b'dtype'), (dict(dtype=-1), b'dtype'),
                     (dict(sense=0), b'sense'), (dict(sense=2), b'sense'), (dict(sense=-2), b'sense'),
                     (dict(relative=2), b'relative'),
                     (dict(top=nan), b'top'), (dict(top=inf), b'top'), (dict(zref=nan), b'zref'), (dict(zref=-inf), b'zref'),
                     (dict(values=(1.0, nan)), b'value'), (dict(values=(inf,)), b'value'),
                     (dict(nz=0, h=()), b'nz, ny and nx'), (dict(ny=0), b'nz, ny and nx'), (dict(nx=-3), b'nz, ny and nx'),
                     (dict(h=tuple([1.0] * 257), nz=257), b'256 levels'),
                     (dict(h=(2.0, 0.0, 2.0, 2.0, 2.0, 2.0, 2.0)), b'thickness'), (dict(h=tuple([nan] * NZ)), b'thickness'),
                     (dict(h=tuple([-1.0] * NZ)), b'thickness'),
                     (dict(out=T), b'overlaps'), (dict(out=T + 11192), b'overlaps'), (dict(out=T - 4792), b'overlaps'),
                     (dict(out=E + 8, h=None, e3t=E), b'overlaps'), (dict(out=T + 5596, dtype=NF_F32), b'overlaps'),
                     (dict(out=T - 2396, dtype=NF_F32), b'overlaps')):
        assert call(**kw) == NF_ERR_ARG, kw
        err = lib.nf_last_error()
        assert word in err and err.startswith(b'nf_iso_depth:'), (kw, err)
    if _lib.device_count() == 0:
        # what is NOT an error goes on to need a device: ranges that only touch, either thickness form, both senses and modes
        for kw in (dict(), dict(out=T + 11200), dict(out=T - 4800), dict(h=None, e3t=E), dict(sense=-1, relative=1),
                   dict(dtype=NF_F32, out=T + 5600), dict(values=nine[1:]), dict(nz=1, ny=1, nx=1, h=(3.0,))):
            assert call(**kw) == 4, kw
            assert b'no usable AMD GPU' in lib.nf_last_error()


# ---- Python ------------------------------------------------------------------------------------------------------------------
def test_iso_depth_objects_describe_derived_surfaces_and_refuse_what_they_cannot_be():
    from nemoflux_amd.eos import Sigma
    from nemoflux_amd.surfaces import IsoDepth, MixedLayerDepth, iso_depth
    th, so = numpy.zeros((2, 3, 4, 5), numpy.float32), numpy.ones((2, 3, 4, 5), numpy.float32)
    a = IsoDepth(th, [20.0, 18.0], -1, fill_value=1.e20)
    assert a.m == 2 and a.values == [20.0, 18.0] and a.sense == -1 and not a.relative and a.zref == 10.0
    assert a.shape == (2, 3, 4, 5) and a.dtype == numpy.float32 and a.markers == (1.e20, None) and a.e3t is None
    assert IsoDepth(th, 4.0, 'rising').values == [4.0] and IsoDepth(th, [4.0], 'falling').sense == -1
    b = MixedLayerDepth(th, so, zref=5.0, so_missing_value=-1.0, e3t=th[0], e3t_fill_value=0.5)
    assert isinstance(b.tracer, Sigma) and b.tracer.pref == 0.0 and b.tracer.markers == ((None, None), (None, -1.0))
    assert b.values == [0.03] and b.sense == 1 and b.relative and b.zref == 5.0 and b.e3t_markers == (0.5, None)
    assert MixedLayerDepth(th, so, delta=[0.01, 0.03, 0.125], pref=2000.).m == 3
    for bad in ([1.0, numpy.nan], [numpy.inf], [], list(range(9)), 'deep'):
        with pytest.raises(RuntimeError, match='values'):
            IsoDepth(th, bad, 1)
    for bad in (0, 2, -1.5, 'up', None):
        with pytest.raises(RuntimeError, match='sense must be'):
            IsoDepth(th, [1.0], bad)
    with pytest.raises(RuntimeError, match='zref'):
        IsoDepth(th, [1.0], 1, relative=True, zref=numpy.nan)
    with pytest.raises(RuntimeError, match='carries the markers'):
        IsoDepth(Sigma(th, so), [27.0], 1, fill_value=1.e20)
    with pytest.raises(RuntimeError, match='CUDA tensors or DeviceArrays'):
        iso_depth(th[0], [1.0], 1, thickness=[1.0, 1.0, 1.0])
    with pytest.raises(RuntimeError, match='exactly one of thickness'):
        iso_depth(th[0], [1.0], 1)


def _bare_field(nt=2, nz=3, ny=4, nx=5, real='float32'):
    """a Field with sizes and dtype only: the refusals of setDepthSurfaces come before anything touches the engine"""
    from nemoflux_amd.field import Field
    f = Field.__new__(Field)
    f.nt, f.nz, f.ny, f.nx = nt, nz, ny, nx
    f._uv_code = NF_F32 if real == 'float32' else NF_F64
    f._h = ctypes.c_void_p()
    f.thickness = numpy.ones(nz)
    return f


def test_set_depth_surfaces_refuses_derived_items_that_do_not_fit():
    from nemoflux_amd.eos import Sigma
    from nemoflux_amd.surfaces import IsoDepth, MixedLayerDepth
    f = _bare_field()
    th = numpy.zeros((2, 3, 4, 5), numpy.float32)
    for bad, words in ((IsoDepth(th[:, :2], [1.0], 1), 'surface 0: the tracer of the IsoDepth has shape'),
                       (IsoDepth(th[:1], [1.0], 1), 'surface 0: the tracer of the IsoDepth has shape'),
                       (IsoDepth(th.astype(numpy.float64), [1.0], 1), 'the tracer of the IsoDepth is float64, uo/vo are float32'),
                       (IsoDepth(th, [1.0], 1, e3t=th[:, :, :3]), 'the e3t of the IsoDepth has shape'),
                       (IsoDepth(th, [1.0], 1, e3t=th[0].astype(numpy.float64)), 'the e3t of the IsoDepth is float64'),
                       (MixedLayerDepth(th[:, :, :2], th[:, :, :2]), 'thetao and so of the Sigma of surface 0 have shape'),
                       (IsoDepth(Sigma(th.astype(numpy.float64), th.astype(numpy.float64)), [27.0], 1),
                        'thetao and so of the Sigma of surface 0 are float64')):
        with pytest.raises(RuntimeError, match=words):
            f.setDepthSurfaces([bad])
    deep = _bare_field(nz=300)
    with pytest.raises(RuntimeError, match='surface 0: an IsoDepth without e3t .* at most 256 levels; this Field has 300: give e3t='):
        deep.setDepthSurfaces([IsoDepth(numpy.zeros((2, 300, 4, 5), numpy.float32), [1.0], 1)])
    with pytest.raises(RuntimeError, match='1 to 8 surfaces, got 9'):
        f.setDepthSurfaces([IsoDepth(th, list(range(1, 9)), 1), numpy.zeros((2, 4, 5), numpy.float32)])
    with pytest.raises(RuntimeError, match='1 to 8 surfaces, got 10'):
        f.setDepthSurfaces([IsoDepth(th, [1.0] * 5, 1), IsoDepth(th, [1.0] * 5, 1)])
    with pytest.raises(RuntimeError, match='call setDepthSurfaces first'):
        f.getDepthSurfaces(0)


# ---- the command line --------------------------------------------------------------------------------------------------------
def test_fluxplot_iso_depth_options_are_checked_before_any_file_is_opened():
    from nemoflux_amd.fluxplot import main, parseIsoValues, parseMixedLayer, checkIsoDepthArgs
    assert parseIsoValues('20') == [20.0] and parseIsoValues(' 27.5, 27.7 ,27.9') == [27.5, 27.7, 27.9]
    assert parseMixedLayer('thetao,so') == ('thetao', 'so', 0.03, 10.0)
    assert parseMixedLayer(' thetao , so , 0.125, 5 ') == ('thetao', 'so', 0.125, 5.0)
    for bad in ('', 'a', '1,,2', '1,nan', 'inf', ','.join('1' * 9)):
        with pytest.raises(RuntimeError, match='--iso-depth'):
            parseIsoValues(bad)
    for bad in ('thetao', 'thetao,,0.03', 'thetao,so,x', 'thetao,so,0.03,deep', 'thetao,so,nan', 'a,b,1,2,3'):
        with pytest.raises(RuntimeError, match='--mixed-layer'):
            parseMixedLayer(bad)
    assert checkIsoDepthArgs() is None
    spec = checkIsoDepthArgs('20,18', 'thetao')
    assert spec['sense'] == -1 and spec['labels'] == ['thetao=20', 'thetao=18'] and not spec['relative']
    spec = checkIsoDepthArgs('27.7', sigma='thetao,so,2000', isoE3t='e3t')
    assert spec['sense'] == 1 and spec['sigma'] == ('thetao', 'so', 2000.0) and spec['labels'] == ['sigma2=27.7']
    spec = checkIsoDepthArgs('-0.2', 'thetao', isoRelative='10')
    assert spec['relative'] and spec['zref'] == 10.0 and spec['labels'] == ['thetao@10-0.2']
    spec = checkIsoDepthArgs(mixedLayer='thetao,so,0.125')
    assert spec['values'] == [0.125] and spec['relative'] and spec['sense'] == 1 and spec['sigma'] == ('thetao', 'so', 0.0)
    files = dict(tFile='/nonexistent/T.nc', uFile='/nonexistent/U.nc', vFile='/nonexistent/V.nc', lonLatPoints='(0,0),(1,1)')
    for kw, words in ((dict(isoOf='thetao'), '--iso-of needs --iso-depth'),
                      (dict(isoSense='rising'), '--iso-sense needs --iso-depth'),
                      (dict(isoRelative='10'), '--iso-relative needs --iso-depth'),
                      (dict(isoE3t='e3t'), '--iso-e3t needs --iso-depth'),
                      (dict(isoDepth='20'), 'exactly one of --iso-of NAME'),
                      (dict(isoDepth='20', isoOf='thetao', sigma='thetao,so'), 'exactly one of --iso-of NAME'),
                      (dict(isoDepth='20', isoOf='thetao', depthSurfaces='mld'), '--iso-depth and --depth-surfaces cannot be'),
                      (dict(mixedLayer='thetao,so', depthSurfaces='mld'), '--mixed-layer and --depth-surfaces cannot be'),
                      (dict(isoDepth='20', isoOf='thetao', mixedLayer='thetao,so'), '--iso-depth and --mixed-layer cannot be'),
                      (dict(isoDepth='20', isoOf='thetao', classes='1,2'), '--iso-depth and --classes cannot be combined'),
                      (dict(isoDepth='20', isoOf='thetao', depthBins='1,2'), '--iso-depth and --depth-bins cannot be combined'),
                      (dict(isoDepth='20', isoOf='thetao', levels=True), '--iso-depth and --levels cannot be combined'),
                      (dict(mixedLayer='thetao,so', eddy=True, tracer='thetao'), '--mixed-layer and --eddy cannot be combined'),
                      (dict(mixedLayer='thetao,so', sigma='thetao,so'), '--mixed-layer and --sigma cannot be combined'),
                      (dict(mixedLayer='thetao,so', isoOf='thetao'), '--mixed-layer and --iso-of cannot be combined'),
                      (dict(isoDepth='20', isoOf='thetao', isoSense='up'), "--iso-sense must be 'rising'"),
                      (dict(isoDepth='20', isoOf='thetao', isoRelative='deep'), '--iso-relative must be ZREF'),
                      (dict(isoDepth='20,x', isoOf='thetao'), '--iso-depth must be'),
                      (dict(isoDepth='20', isoOf='thetao', depthTop=numpy.inf), '--depth-top must be a finite number'),
                      (dict(isoDepth='20', isoOf='thetao', tracerRef=1.0), '--tracer-ref / --tracer-scale need --tracer'),
                      (dict(isoDepth='20', isoOf='thetao', e3u='e3u_0'), 'need --cell-thickness')):
        with pytest.raises(RuntimeError, match=words):
            main(**kw, **files)
    for kw in (dict(isoDepth='20', isoOf='thetao', surfaceFile='/nonexistent/S.nc', depthTop=5.0, tracer='so', cellThickness=True),
               dict(isoDepth='27.7,27.9', sigma='thetao,so', isoRelative='10', isoE3t='e3t', sverdrup=True),
               dict(mixedLayer='thetao,so,0.01,5', isoE3t='e3t')):
        with pytest.raises(RuntimeError, match='no such file'):      # an accepted combination goes on to open the files
            main(**kw, **files)


def test_fluxplot_command_line_lists_the_new_options():
    out = subprocess.run([sys.executable, '-m', 'nemoflux_amd.fluxplot', '--help'], cwd=ROOT, capture_output=True, text=True,
                         timeout=120)
    assert out.returncode == 0, out.stderr
    for opt in ('--iso-depth', '--iso-of', '--iso-sense', '--iso-relative', '--iso-e3t', '--mixed-layer'):
        assert opt in out.stdout
