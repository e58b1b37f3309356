"""Transport in joint classes of two tracers, the parts that need no GPU: tests/joint_class_reference.py pinned to a naive
per-entry loop with math.fsum on synthetic entries and to the 1-D class rows of resolved_reference; the three entry points'
argument, edge and call-order checks before a device is touched; fluxplot's --classes2 options; Field.jointClassStreamfunction."""
import bisect
import ctypes
import math
import os
import re

import numpy
import pytest

from joint_class_reference import JointClassReference
from resolved_reference import ResolvedReference, array_values

NF_ERR_ARG, NF_ERR_STATE = 1, 2
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CALLS = ('nf_field_set_joint_class_edges', 'nf_field_compute_joint_class_transport',
         'nf_field_compute_joint_class_transport_async')
EPS = numpy.finfo(numpy.float64).eps
FILL, MISSING = 1.e20, -999.                 # markers of uo / vo
AFILL, AMISSING = 9999., -7777.              # markers of A
BFILL, BMISSING = -32768., 12345.            # markers of B
REF = 3.25
EA = numpy.array([5., 8., 10., 12., 15.])
EB = numpy.array([-1., 0.5, 2.])
NX, NY, NZ, NT = 7, 5, 3, 2
TR_OFF = numpy.array([0, 3, 5])


def _entries(seed):
    """synthetic (cell * 4 + slot, weight, segment): random ones, every slot of the four corner cells (row 0's south slots,
    the last column's east slots, column 0's west slots, the last row's north slots) and of the cells around the planted
    +-inf pair"""
    rng = numpy.random.default_rng(seed)
    n = 160
    ce = rng.integers(0, NX * NY, n) * 4 + rng.integers(0, 4, n)
    special = [c * 4 + s for c in (0, NX - 1, (NY - 1) * NX, NX * NY - 1, 2 * NX + 2, 2 * NX + 3, 2 * NX + 4, 3 * NX + 3, 3 * NX + 5)
               for s in range(4)]
    ce = numpy.concatenate([ce, special])
    rng.shuffle(ce)
    return ce, rng.standard_normal(ce.size), rng.integers(0, TR_OFF[-1], ce.size)


def _arrays(real, seed, inf_a=True):
    """inf_a: +-inf in A too (its NaN faces have no class of A) -- for the volume form only: carried, they make the terms
    themselves infinite"""
    rng = numpy.random.default_rng(seed)
    dt = numpy.dtype(real).type
    shape = (NT, NZ, NY, NX)

    def plant(a, values, share):
        flat = a.reshape(-1)
        for m in values:
            flat[rng.choice(a.size, max(1, a.size // share), replace=False)] = dt(m)
        return a

    uo = plant(rng.standard_normal(shape).astype(dt), (FILL, MISSING, numpy.nan), 10)
    vo = plant(rng.standard_normal(shape).astype(dt), (FILL, MISSING, numpy.nan), 10)
    A = (10. + 4. * rng.standard_normal(shape)).astype(dt)
    A.reshape(-1)[rng.choice(A.size, A.size // 3, replace=False)] = rng.choice([8., 12.], A.size // 3)   # faces on an edge
    plant(A, (AFILL, AMISSING, numpy.nan, BFILL), 9)                 # B's marker is a value of A
    B = (0.5 + 1.5 * rng.standard_normal(shape)).astype(dt)
    B.reshape(-1)[rng.choice(B.size, B.size // 3, replace=False)] = rng.choice([-1., 2.], B.size // 3)
    plant(B, (BFILL, BMISSING, numpy.nan, AFILL), 9)
    if inf_a:
        A[:, :, 2, 2:5] = (numpy.inf, -numpy.inf, numpy.inf)         # east faces whose mean is NaN: no class of A
    B[:, :, 2:4, 3] = numpy.array([-numpy.inf, numpy.inf])[None, None, :]   # a north face without a class of B
    A[:, 0, 4, 0:2] = dt(AFILL)                                      # A missing on both sides where B is present
    B[:, 0, 4, 0:2] = dt(1.)
    A[:, 1, 0, 5:7] = dt(9.)                                         # ... and the reverse
    B[:, 1, 0, 5:7] = dt(BMISSING)
    A[:, 2, 3, 5:7] = dt(AMISSING)                                   # neither has a value, and water flows
    B[:, 2, 3, 5:7] = dt(BFILL)
    uo[:, 2, 3, 5] = dt(1.5)
    return dict(uo=uo, vo=vo, tracer=A, **{'class': B})


def _naive(ce, w, sg, arc, th, a, t, wrap, sverdrup, names=('volume', 'tracer')):
    """every joint value as math.fsum of its terms, one (entry, level) at a time from the full arrays"""
    dt = a['uo'].dtype.type
    nseg, ntr = int(TR_OFF[-1]), len(TR_OFF) - 1
    tr_of = [p for p in range(ntr) for _ in range(TR_OFF[p], TR_OFF[p + 1])]
    nrow = (len(EA) + 2) * (len(EB) + 2)

    def present(x, marks):
        return not math.isnan(x) and all(x != dt(m) for m in marks)

    def face(arr, z, ca, cb, marks):
        flat = arr[t, z].reshape(-1)
        pa = present(flat[ca], marks)
        pb = cb is not None and present(flat[cb], marks)
        if pa and pb:
            return True, 0.5 * (float(flat[ca]) + float(flat[cb]))
        if pa:
            return True, float(flat[ca])
        if pb:
            return True, float(flat[cb])
        return False, 0.0

    def row_of(has, x, edges):
        return bisect.bisect_right(list(edges), x) if has and not math.isnan(x) else len(edges) + 1

    terms = {nm: {} for nm in names}
    seen = dict(south0=0, a_only=0, b_only=0, nan_a=0, nan_b=0, on_edge=0, no_east=0)
    for e in range(len(ce)):
        c, slot, s = int(ce[e]) // 4, int(ce[e]) % 4, int(sg[e])
        j, i = divmod(c, NX)
        if slot == 0:
            if j == 0:
                seen['south0'] += 1
                continue
            ca, cb = c - NX, c
        elif slot == 1:
            ca, cb = c, (c + 1 if i < NX - 1 else (c + 1 - NX if wrap else None))
            seen['no_east'] += cb is None
        elif slot == 2:
            ca, cb = c, (c + NX if j < NY - 1 else None)
        else:
            ca = c - 1 if i > 0 else c - 1 + NX
            cb = c if (i > 0 or wrap) else None
        for z in range(NZ):
            x = (a['uo'] if slot in (1, 3) else a['vo'])[t, z].reshape(-1)[ca]
            vel = float(x) if present(x, (FILL, MISSING)) else 0.0
            has_a, xa = face(a['tracer'], z, ca, cb, (AFILL, AMISSING))
            has_b, xb = face(a['class'], z, ca, cb, (BFILL, BMISSING))
            tf = xa - REF if has_a else 0.0
            al = float(arc[ca, 1]) if slot in (1, 3) else -float(arc[ca, 2])
            dv, dtau = (float(th[z]) * vel) * al, (float(th[z]) * (vel * tf)) * al
            if sverdrup:
                dv, dtau = dv * (6371000.0 / 1.e6), dtau * (6371000.0 / 1.e6)
            row = row_of(has_a, xa, EA) * (len(EB) + 2) + row_of(has_b, xb, EB)
            seen['a_only'] += has_a and not has_b
            seen['b_only'] += has_b and not has_a
            seen['nan_a'] += has_a and math.isnan(xa)
            seen['nan_b'] += has_b and math.isnan(xb)
            seen['on_edge'] += (has_a and xa in EA) or (has_b and xb in EB)
            for col in (s, nseg + tr_of[s]):
                for nm, x in (('volume', dv), ('tracer', dtau)):
                    if nm in terms:
                        terms[nm].setdefault((row, col), []).append(float(w[e]) * x)
    out = {}
    for nm in terms:
        want, mag = numpy.zeros((nrow, nseg + ntr)), numpy.zeros((nrow, nseg + ntr))
        for idx, xs in terms[nm].items():
            want[idx], mag[idx] = math.fsum(xs), math.fsum(abs(x) for x in xs)
        out[nm] = (want, mag)
    return out, seen


def _reference(cls, ce, w, sg, arc, th, wrap, sverdrup, class_markers=(BFILL, BMISSING)):
    return cls(ce, w, sg, arc, th, TR_OFF, NX, NY, uv_markers=(FILL, MISSING), tracer_markers=(AFILL, AMISSING),
               class_markers=class_markers, reference=REF, wrap=wrap, sverdrup=sverdrup)


@pytest.mark.parametrize('wrap', [True, False], ids=['wrap', 'nowrap'])
@pytest.mark.parametrize('real', ['float64', 'float32'])
def test_restatement_is_the_naive_loop(real, wrap):
    ce, w, sg = _entries(seed=11 + wrap)
    rng = numpy.random.default_rng(5)
    arc = 0.5 + rng.random((NX * NY, 4))
    th = numpy.array([0.5, 0.25, 2.0])
    sverdrup = not wrap
    ref = _reference(JointClassReference, ce, w, sg, arc, th, wrap, sverdrup)
    for inf_a, names in ((True, ('volume',)), (False, ('volume', 'tracer'))):
        a = _arrays(real, seed=3 + wrap, inf_a=inf_a)
        for t in range(NT):
            got = ref.joint(array_values(a, t), EA, EB)
            want, seen = _naive(ce, w, sg, arc, th, a, t, wrap, sverdrup, names)
            assert all(seen[k] > 0 for k in ('south0', 'a_only', 'b_only', 'nan_b', 'on_edge')), seen
            assert (seen['nan_a'] > 0) == inf_a and (seen['no_east'] > 0) == (not wrap), seen
            for nm in names:
                (g_, gm_), (w_, m_) = got[nm], want[nm]
                assert g_.shape == w_.shape == gm_.shape == ((len(EA) + 2) * (len(EB) + 2), TR_OFF[-1] + 2)
                assert (m_ > 0).mean() > 0.25, nm
                assert numpy.all(numpy.abs(g_ - w_) <= 4 * EPS * m_), (nm, t, (numpy.abs(g_ - w_) / numpy.maximum(m_, 1e-300)).max())
                assert numpy.all(numpy.abs(gm_ - m_) <= 4 * EPS * m_), (nm, t)
            # the rows without a class of A, of B, and of both carry flux
            m3 = want['volume'][1].reshape(len(EA) + 2, len(EB) + 2, -1)
            assert m3[-1, :-1].max() > 0 and m3[:-1, -1].max() > 0 and m3[-1, -1].max() > 0


@pytest.mark.parametrize('wrap', [True, False], ids=['wrap', 'nowrap'])
def test_marginals_are_the_one_dimensional_class_rows(wrap):
    ce, w, sg = _entries(seed=21)
    arc = 0.5 + numpy.random.default_rng(6).random((NX * NY, 4))
    th = numpy.array([0.5, 0.25, 2.0])
    a = _arrays('float64', seed=8, inf_a=False)
    joint = _reference(JointClassReference, ce, w, sg, arc, th, wrap, False).joint(array_values(a, 1), EA, EB)
    by_b = _reference(ResolvedReference, ce, w, sg, arc, th, wrap, False).step(array_values(a, 1), [EB])
    a_as_class = dict(a, **{'class': a['tracer']})
    by_a = _reference(ResolvedReference, ce, w, sg, arc, th, wrap, False, class_markers=(AFILL, AMISSING)).step(
        array_values(a_as_class, 1), [EA])
    for nm, one in (('volume', 'volume_classes'), ('tracer', 'tracer_classes')):
        want, mag = (x.reshape(len(EA) + 2, len(EB) + 2, -1) for x in joint[nm])
        for axis, ref in ((1, by_a), (0, by_b)):
            w1, m1 = ref[one, 0]
            assert m1.max() > 0
            assert numpy.all(numpy.abs(want.sum(axis=axis) - w1) <= 8 * EPS * m1), (nm, axis)
            assert numpy.all(numpy.abs(mag.sum(axis=axis) - m1) <= 8 * EPS * m1), (nm, axis)


# ---- the C ABI without a device ---------------------------------------------------------------------------------------------
def test_header_declares_and_library_exports_the_joint_calls():
    from nemoflux_amd import _lib
    with open(os.path.join(ROOT, 'include', 'nemoflux_amd.h')) as fh:
        header = fh.read()
    for name in CALLS:
        assert re.search(r'\bint\s+' + name + r'\s*\(\s*nf_field\s*\*\*\s*self', header), name
        assert hasattr(_lib.lib, name), name


def _new():
    from nemoflux_amd import _lib
    h = ctypes.c_void_p()
    assert _lib.lib.nf_field_new(ctypes.byref(h)) == 0
    return h


def _set_edges(h, ea, eb, na=None, nb=None):
    from nemoflux_amd import _lib
    ea = numpy.ascontiguousarray(ea, dtype=numpy.float64)
    eb = numpy.ascontiguousarray(eb, dtype=numpy.float64)
    return _lib.lib.nf_field_set_joint_class_edges(ctypes.byref(h) if h is not None else None, _lib.dptr(ea),
                                                   len(ea) if na is None else na, _lib.dptr(eb), len(eb) if nb is None else nb)


def test_edges_are_checked_without_a_gpu():
    from nemoflux_amd import _lib
    lib = _lib.lib
    ok = [0., 1.]
    assert _set_edges(None, ok, ok) == NF_ERR_ARG
    assert b'null' in lib.nf_last_error()
    h = _new()
    try:
        e = numpy.array(ok)
        assert lib.nf_field_set_joint_class_edges(ctypes.byref(h), None, 2, _lib.dptr(e), 2) == NF_ERR_ARG
        assert b'null' in lib.nf_last_error()
        assert lib.nf_field_set_joint_class_edges(ctypes.byref(h), _lib.dptr(e), 2, None, 2) == NF_ERR_ARG
        assert b'null' in lib.nf_last_error()
        for axis, put in ((b'axis A', lambda bad, n=None: _set_edges(h, bad, ok, na=n)),
                          (b'axis B', lambda bad, n=None: _set_edges(h, ok, bad, nb=n))):
            for bad in ([0.], numpy.arange(1026.)):
                assert put(bad) == NF_ERR_ARG, len(bad)
                assert b'nedges' in lib.nf_last_error() and axis in lib.nf_last_error()
            assert put(ok, -3) == NF_ERR_ARG and put(ok, 0) == NF_ERR_ARG
            for bad in ([0., 0.], [1., 0.], [0., 1., 1.], [0., 2., 1.]):
                assert put(bad) == NF_ERR_ARG, bad
                assert b'strictly increasing' in lib.nf_last_error() and axis in lib.nf_last_error()
            for bad in ([0., numpy.nan], [-numpy.inf, 0.], [0., numpy.inf], [numpy.nan, numpy.nan]):
                assert put(bad) == NF_ERR_ARG, bad
                assert b'finite' in lib.nf_last_error() and axis in lib.nf_last_error()
        # the row cap: (na + 2) * (nb + 2) <= 16384, the count is named
        assert _set_edges(h, numpy.arange(126.), numpy.arange(126.)) == 0            # 128 * 128 = 16384
        assert _set_edges(h, numpy.arange(127.), numpy.arange(126.)) == NF_ERR_ARG   # 129 * 128 = 16512
        assert b'16512' in lib.nf_last_error() and b'16384' in lib.nf_last_error()
        assert _set_edges(h, numpy.arange(1025.), numpy.arange(1025.)) == NF_ERR_ARG
        assert b'1054729' in lib.nf_last_error()
        assert _set_edges(h, numpy.arange(1025.), numpy.arange(14.)) == NF_ERR_ARG   # 1027 * 16 = 16432
        assert _set_edges(h, numpy.arange(1022.), numpy.arange(14.)) == 0            # 1024 * 16 = 16384
        assert _set_edges(h, [-1e300, 1e300], [-1e300, -0.5, 0.5, 1e300]) == 0
        assert lib.nf_field_set_joint_class_edges(ctypes.byref(h), None, 0, None, 0) == 0   # two NULLs clear the edges
    finally:
        assert lib.nf_field_del(ctypes.byref(h)) == 0


def _both(h, t=0, carry=0, rows=numpy.zeros(64)):
    from nemoflux_amd import _lib
    lib = _lib.lib
    hp = ctypes.byref(h) if h is not None else None
    a = lib.nf_field_compute_joint_class_transport(hp, t, carry, _lib.dptr(rows) if rows is not None else None)
    msg_a = lib.nf_last_error()
    b = lib.nf_field_compute_joint_class_transport_async(hp, t, carry, ctypes.c_void_p(rows.ctypes.data) if rows is not None else None)
    return (a, msg_a), (b, lib.nf_last_error())


def test_null_arguments_and_carry_are_refused():
    for rc, msg in _both(None):
        assert rc == NF_ERR_ARG and b'null' in msg
    h = _new()
    try:
        for rc, msg in _both(h, rows=None):
            assert rc == NF_ERR_ARG and b'null' in msg
        for carry in (2, -1):
            for rc, msg in _both(h, carry=carry):
                assert rc == NF_ERR_ARG and b'carry must be 0 or 1' in msg
    finally:
        from nemoflux_amd import _lib
        assert _lib.lib.nf_field_del(ctypes.byref(h)) == 0


def test_call_order_is_a_state_error():
    from nemoflux_amd import _lib
    lib = _lib.lib
    uv = numpy.zeros(16)
    h = _new()
    try:
        for carry in (0, 1):
            for rc, msg in _both(h, carry=carry):         # nothing set
                assert rc == NF_ERR_STATE and b'set_tracer first' in msg
        assert _set_edges(h, [0., 1.], [0., 1., 2.]) == 0
        for rc, msg in _both(h):                          # edges, no tracer
            assert rc == NF_ERR_STATE and b'set_tracer first' in msg
        assert lib.nf_field_set_uv(ctypes.byref(h), uv.ctypes.data, uv.ctypes.data, 3, 0, 0, numpy.nan) == 0
        assert lib.nf_field_set_tracer(ctypes.byref(h), uv.ctypes.data, 3, 0, 0, numpy.nan) == 0
        for rc, msg in _both(h):                          # no class tracer
            assert rc == NF_ERR_STATE and b'set_class_tracer first' in msg
        assert lib.nf_field_set_class_tracer(ctypes.byref(h), uv.ctypes.data, 3, 0, 0, numpy.nan) == 0
        for rc, msg in _both(h):                          # everything but the grid
            assert rc == NF_ERR_STATE and b'set_bounds' in msg
        assert lib.nf_field_set_joint_class_edges(ctypes.byref(h), None, 0, None, 0) == 0
        for rc, msg in _both(h):                          # cleared edges
            assert rc == NF_ERR_STATE and b'set_joint_class_edges first' in msg
        # the 1-D edges are another state: they do not serve the joint call, and the joint edges do not serve the 1-D call
        e = numpy.array([0., 1.])
        assert lib.nf_field_set_class_edges(ctypes.byref(h), _lib.dptr(e), 2) == 0
        for rc, msg in _both(h):
            assert rc == NF_ERR_STATE and b'set_joint_class_edges first' in msg
    finally:
        assert lib.nf_field_del(ctypes.byref(h)) == 0
    h = _new()
    try:
        assert lib.nf_field_set_uv(ctypes.byref(h), uv.ctypes.data, uv.ctypes.data, 3, 0, 0, numpy.nan) == 0
        assert lib.nf_field_set_tracer(ctypes.byref(h), uv.ctypes.data, 3, 0, 0, numpy.nan) == 0
        assert _set_edges(h, [0., 1.], [0., 1.]) == 0
        rows = numpy.zeros(64)
        assert lib.nf_field_compute_class_transport(ctypes.byref(h), 0, _lib.dptr(rows)) == NF_ERR_STATE
        assert b'set_class_edges first' in lib.nf_last_error()
    finally:
        assert lib.nf_field_del(ctypes.byref(h)) == 0


def test_tuning_knobs_are_range_checked():
    from nemoflux_amd import _lib
    lib = _lib.lib
    for bad in (0, 33, -1):
        assert lib.nf_tuning_set(b'joint_window', bad) != 0
    for bad in (2, -1):
        assert lib.nf_tuning_set(b'joint_skip', bad) != 0
    for name, values in ((b'joint_window', (1, 5, 32)), (b'joint_skip', (0, 1))):
        for v in values:
            assert lib.nf_tuning_set(name, v) == 0


# ---- Python -----------------------------------------------------------------------------------------------------------------
def test_joint_class_streamfunction_on_a_hand_made_array():
    from nemoflux_amd.field import Field
    na, nb = 3, 2
    rows = numpy.arange((na + 2) * (nb + 2) * 2, dtype=numpy.float64).reshape(na + 2, nb + 2, 2) ** 1.5
    psi = Field.jointClassStreamfunction(rows)
    assert psi.shape == (na, nb + 2, 2)
    assert numpy.array_equal(psi[0], rows[0])
    assert numpy.array_equal(psi[1], rows[0] + rows[1])
    assert numpy.array_equal(psi[2], (rows[0] + rows[1]) + rows[2])
    psi = Field.jointClassStreamfunction(rows, axis=1)
    assert psi.shape == (na + 2, nb, 2)
    assert numpy.array_equal(psi[:, 0], rows[:, 0])
    assert numpy.array_equal(psi[:, 1], rows[:, 0] + rows[:, 1])
    # a 2-D array of class pairs works too; along one axis it is classStreamfunction of every column
    flat = rows[..., 0]
    assert numpy.array_equal(Field.jointClassStreamfunction(flat, axis=0), Field.classStreamfunction(flat))
    with pytest.raises(ValueError, match='axis'):
        Field.jointClassStreamfunction(rows, axis=2)
    for bad in (numpy.zeros((3, 4)), numpy.zeros((4, 3, 2)), numpy.zeros(6)):
        with pytest.raises(ValueError, match='computeJointClassTransport'):
            Field.jointClassStreamfunction(bad)


def test_fluxplot_joint_class_options_are_checked():
    from nemoflux_amd.fluxplot import checkJointClassArgs, main
    checkJointClassArgs()
    good = dict(classes2='34,35,36', tracer2='so', tracer='thetao', classes='0,10,20')
    checkJointClassArgs(**good)
    checkJointClassArgs(tracer2File='S.nc', **good)
    for missing in ('tracer2', 'tracer', 'classes'):
        with pytest.raises(RuntimeError, match='--classes2 needs --tracer2'):
            checkJointClassArgs(**dict(good, **{missing: ''}))
    for kw in (dict(tracer2='so'), dict(tracer2File='S.nc')):
        with pytest.raises(RuntimeError, match='need --classes2'):
            checkJointClassArgs(**kw)
    for opt, kw in (('--carry', dict(carry='thetao')), ('--levels', dict(levels=True)), ('--zrange', dict(zrange='0,10')),
                    ('--show', dict(show=True)), ('--eddy', dict(eddy=True)), ('--decompose', dict(decompose=True))):
        with pytest.raises(RuntimeError, match='--classes2 and ' + opt):
            checkJointClassArgs(**dict(good, **kw))
    for bad in ('34', '35,34', '34,nan', 'a,b'):
        with pytest.raises(RuntimeError, match='--classes2'):
            checkJointClassArgs(**dict(good, classes2=bad))
    with pytest.raises(RuntimeError, match='16384'):
        checkJointClassArgs(**dict(good, classes=','.join(str(k) for k in range(200)), classes2=','.join(str(k) for k in range(200))))
    # refused before any file is opened
    for kw in (dict(tracer2=''), dict(carry='thetao'), dict(levels=True), dict(zrange='0,10'), dict(show=True), dict(eddy=True),
               dict(decompose=True)):
        with pytest.raises(RuntimeError, match='--classes2'):
            main(tFile='no_such_T.nc', uFile='no_such_U.nc', vFile='no_such_V.nc', lonLatPoints='[(0,0),(1,1)]',
                 **dict(good, **kw))


def test_fluxplot_command_line_has_the_joint_class_options():
    import subprocess
    import sys
    out = subprocess.run([sys.executable, '-m', 'nemoflux_amd.fluxplot', '--help'], cwd=ROOT, capture_output=True, text=True,
                         timeout=120)
    assert out.returncode == 0, out.stderr
    for opt in ('--tracer2 NAME', '--tracer2-file FILE', '--classes2 F0,F1,...,FM'):
        assert opt in out.stdout, opt
    bad = subprocess.run([sys.executable, '-m', 'nemoflux_amd.fluxplot', '-t', 'no_T.nc', '-u', 'no_U.nc', '-v', 'no_V.nc',
                          '-l', '[(0,0),(1,1)]', '--classes2', '34,35'], cwd=ROOT, capture_output=True, text=True, timeout=120)
    assert bad.returncode != 0 and '--classes2 needs --tracer2' in bad.stderr
