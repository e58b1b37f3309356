"""Volume transport in tracer classes, the parts that need no GPU: the header declares the three entry points and the library
exports them; the calls check their handle, edges and call order before touching a device; Field.classStreamfunction;
fluxplot's --classes option."""
import ctypes
import os
import re

import numpy
import pytest

NF_ERR_ARG, NF_ERR_STATE = 1, 2
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CALLS = ('nf_field_set_class_edges', 'nf_field_compute_class_transport', 'nf_field_compute_class_transport_async')


def test_header_declares_and_library_exports_the_class_calls():
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


def _set_edges(h, edges, n=None):
    from nemoflux_amd import _lib
    e = numpy.ascontiguousarray(edges, dtype=numpy.float64)
    return _lib.lib.nf_field_set_class_edges(ctypes.byref(h) if h is not None else None, _lib.dptr(e),
                                             len(e) if n is None else n)


def test_edges_are_checked_without_a_gpu():
    from nemoflux_amd import _lib
    lib = _lib.lib
    assert _set_edges(None, [0., 1.]) == NF_ERR_ARG
    assert b'null' in lib.nf_last_error()
    h = _new()
    try:
        assert lib.nf_field_set_class_edges(ctypes.byref(h), None, 2) == NF_ERR_ARG
        for bad in ([0.], [], numpy.arange(1026.)):
            assert _set_edges(h, bad if len(bad) else [0.], len(bad)) == NF_ERR_ARG, len(bad)
            assert b'nedges' in lib.nf_last_error()
        assert _set_edges(h, [0., 1.], -3) == NF_ERR_ARG
        for bad in ([0., 0.], [1., 0.], [0., 1., 1.], [0., 2., 1.]):
            assert _set_edges(h, bad) == NF_ERR_ARG, bad
            assert b'strictly increasing' in lib.nf_last_error()
        for bad in ([0., numpy.nan], [-numpy.inf, 0.], [0., numpy.inf], [numpy.nan, numpy.nan]):
            assert _set_edges(h, bad) == NF_ERR_ARG, bad
            assert b'finite' in lib.nf_last_error()
        assert _set_edges(h, [0., 1.]) == 0
        assert _set_edges(h, numpy.arange(1025.)) == 0
        assert _set_edges(h, [-1e300, -0.5, 0.5, 1e300]) == 0
    finally:
        assert lib.nf_field_del(ctypes.byref(h)) == 0


def test_null_handles_and_arguments_are_refused():
    from nemoflux_amd import _lib
    lib = _lib.lib
    rows = numpy.zeros(64)
    assert lib.nf_field_compute_class_transport(None, 0, _lib.dptr(rows)) == NF_ERR_ARG
    assert lib.nf_field_compute_class_transport_async(None, 0, ctypes.c_void_p(rows.ctypes.data)) == NF_ERR_ARG
    h = _new()
    try:
        assert lib.nf_field_compute_class_transport(ctypes.byref(h), 0, None) == NF_ERR_ARG
        assert b'null' in lib.nf_last_error()
        assert lib.nf_field_compute_class_transport_async(ctypes.byref(h), 0, None) == NF_ERR_ARG
        assert b'null' in lib.nf_last_error()
    finally:
        assert lib.nf_field_del(ctypes.byref(h)) == 0


def test_compute_before_set_tracer_or_set_class_edges_is_a_state_error():
    from nemoflux_amd import _lib
    lib = _lib.lib
    rows = numpy.zeros(64)
    uv = numpy.zeros(16)

    def both(h):
        a = lib.nf_field_compute_class_transport(ctypes.byref(h), 0, _lib.dptr(rows))
        msg_a = lib.nf_last_error()
        b = lib.nf_field_compute_class_transport_async(ctypes.byref(h), 0, ctypes.c_void_p(rows.ctypes.data))
        return (a, msg_a), (b, lib.nf_last_error())

    h = _new()
    try:
        for rc, msg in both(h):             # nothing set
            assert rc == NF_ERR_STATE and b'set_tracer first' in msg
        assert _set_edges(h, [0., 1.]) == 0
        for rc, msg in both(h):             # edges, no tracer
            assert rc == NF_ERR_STATE and b'set_tracer first' in msg
    finally:
        assert lib.nf_field_del(ctypes.byref(h)) == 0
    h = _new()
    try:
        assert lib.nf_field_set_uv(ctypes.byref(h), uv.ctypes.data, uv.ctypes.data, 3, 0, 0, numpy.nan) == 0
        assert lib.nf_field_set_tracer(ctypes.byref(h), uv.ctypes.data, 3, 0, 0, numpy.nan) == 0
        for rc, msg in both(h):             # tracer, no edges
            assert rc == NF_ERR_STATE and b'set_class_edges first' in msg
        assert _set_edges(h, [0., 1., 2.]) == 0
        for rc, msg in both(h):             # both, but no grid yet
            assert rc == NF_ERR_STATE and b'set_bounds' in msg
    finally:
        assert lib.nf_field_del(ctypes.byref(h)) == 0


def test_class_streamfunction_on_synthetic_rows():
    from nemoflux_amd.field import Field
    rng = numpy.random.default_rng(3)
    nedges = 5
    rows = rng.standard_normal((nedges + 2, 4))
    psi = Field.classStreamfunction(rows)
    assert psi.shape == (nedges, 4)
    want = numpy.zeros(4)
    for k in range(nedges):
        want = want + rows[k]
        assert numpy.array_equal(psi[k], want), k
    # the no-value row and the top class are not part of psi; psi[-1] + the top class = the transport of every classed face
    assert numpy.allclose(psi[-1] + rows[nedges], rows[:nedges + 1].sum(axis=0), rtol=1e-14, atol=1e-14)
    # segments or totals, with trailing axes of any shape; a 1-D column of class values works too
    assert Field.classStreamfunction(rows.reshape(nedges + 2, 2, 2)).shape == (nedges, 2, 2)
    assert numpy.array_equal(Field.classStreamfunction(numpy.arange(6.)), [0., 1., 3., 6.])
    with pytest.raises(ValueError, match='nedges'):
        Field.classStreamfunction(numpy.zeros((3, 2)))


def test_fluxplot_class_options_are_checked():
    from nemoflux_amd.fluxplot import checkClassArgs, parseClasses, main
    checkClassArgs()
    checkClassArgs('26,27,28', 'sigma0')
    assert parseClasses('26, 27.5,28') == [26., 27.5, 28.]
    with pytest.raises(RuntimeError, match='needs --tracer'):
        checkClassArgs('26,27')
    with pytest.raises(RuntimeError, match='--zrange'):
        checkClassArgs('26,27', 'sigma0', zrange='0,1000')
    with pytest.raises(RuntimeError, match='--tracer-ref'):
        checkClassArgs('26,27', 'sigma0', tracerRef=1.0)
    with pytest.raises(RuntimeError, match='--tracer-scale'):
        checkClassArgs('26,27', 'sigma0', tracerScale=2.0)
    with pytest.raises(RuntimeError, match='--show'):
        checkClassArgs('26,27', 'sigma0', show=True)
    for bad in ('26', '27,26', '26,26', '26,nan', '26,inf', 'a,b', ''):
        with pytest.raises(RuntimeError, match='--classes'):
            parseClasses(bad)
    # refused before any file is opened
    for kw in (dict(zrange='0,10'), dict(show=True), dict(tracerRef=2.0), dict(tracer='')):
        args = dict(tracer='sigma0', classes='26,27')
        args.update(kw)
        with pytest.raises(RuntimeError, match='--'):
            main(tFile='no_such_T.nc', uFile='no_such_U.nc', vFile='no_such_V.nc', lonLatPoints='[(0,0),(1,1)]', **args)


def test_fluxplot_command_line_has_the_class_option():
    import subprocess
    import sys
    out = subprocess.run([sys.executable, '-m', 'nemoflux_amd.fluxplot', '--help'], cwd=ROOT, capture_output=True, text=True,
                         timeout=120)
    assert out.returncode == 0, out.stderr
    assert '--classes E0,E1,...,EN' in out.stdout
    bad = subprocess.run([sys.executable, '-m', 'nemoflux_amd.fluxplot', '-t', 'no_T.nc', '-u', 'no_U.nc', '-v', 'no_V.nc',
                          '-l', '[(0,0),(1,1)]', '--classes', '26,27'], cwd=ROOT, capture_output=True, text=True, timeout=120)
    assert bad.returncode != 0 and '--classes needs --tracer' in bad.stderr
