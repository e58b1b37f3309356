"""The interleaved inner steps of a per-step pass ("pass_inner_interleaved"): the steps of a pair that no caller can read --
the first of every pair, the second of every pair but the pass's last -- are stored by K1 as one (eU, eV) stream and
gathered by the pair form of K3 from it.  Nothing about the results may change: every comparison here is bit for bit
(uint64 views), against the knob at 0, against per-step nf_field_compute_flux and against a lone step on a fresh handle.

Shapes: 37 x 36 x 3 (odd rows: lanes straddle row ends, 1332 cells leave a partial last tile at both dtypes) with 2, 3 and 5
steps (one pair on the resident planes; an odd count with its leading single step; two pairs, the first one interleaved in
both operands), and 64 x 8 x 2 with 4 steps (rows a multiple of the lane width).  The interleaved form belongs to K1's
two-field kernel, which a launch this small takes only with "field_split" at 0 (what the big grids run by themselves); with
the knob at its default the pass must stay on the path it had, so both settings are run."""
import contextlib
import ctypes

import numpy
import pytest

from gpu_helpers import _field, _resident, _same_bits

pytestmark = pytest.mark.gpu

SHAPES = [(37, 36, 3, 2), (37, 36, 3, 3), (37, 36, 3, 5), (64, 8, 2, 4)]
YMIN, YMAX = -72., 72.
FILL = 1.e20
_CASES = {}


def _transects(nx, ny):
    """Polylines that need every neighbour rule: inside column 0 (the west slot wraps to column nx - 1), across the seam
    into column 0 from the east, along row 0 (no south slot), along the top row, a closed one, and a long open one."""
    dx, dy = 360. / nx, (YMAX - YMIN) / ny
    ym = 0.5 * (YMIN + YMAX)
    lines = [
        [(-180. + 0.3 * dx, YMIN + 1.2 * dy), (-180. + 0.7 * dx, YMAX - 1.4 * dy)],
        [(180. - 2.4 * dx, ym - 2.3 * dy), (180. + 1.6 * dx, ym + 1.7 * dy), (180. + 0.4 * dx, ym + 2.6 * dy)],
        [(-180. + 1.5 * dx, YMIN + 0.3 * dy), (180. - 1.5 * dx, YMIN + 0.7 * dy)],
        [(-180. + 2.5 * dx, YMAX - 0.6 * dy), (180. - 2.5 * dx, YMAX - 0.2 * dy)],
        [(-100., YMIN + 1.1 * dy), (100., YMIN + 1.3 * dy), (3., YMAX - 1.2 * dy), (-100., YMIN + 1.1 * dy)],
        [(-170., ym - 1.9 * dy), (-20., ym + 2.2 * dy), (60., YMIN + 0.4 * dy), (175., YMAX - 0.5 * dy)],
    ]
    out = []
    for pts in lines:
        xyz = numpy.zeros((len(pts), 3))
        xyz[:, :2] = pts
        out.append(xyz)
    return out


def _case(shape, real):
    """Arguments of Field.fromArrays, made once per (shape, dtype) and left unchanged: random velocities that grow with the
    step, land blocks of NaN and of the fill value (one against column 0 and row 0), and one large value in the last step so
    that the running max of a whole pass is also the max of its last step alone."""
    key = (shape, real)
    if key not in _CASES:
        import torch
        from nemoflux_amd.datagen import DataGen
        nx, ny, nz, nt = shape
        dg = DataGen(real=real)
        dg.setSizes(nx, ny, nz, nt)
        dg.setBoundingBox(-180., 180., YMIN, YMAX, 0., 1.)
        dg.build()
        rng = numpy.random.default_rng(1000 * nx + nt)
        scale = (1. + numpy.arange(nt))[:, None, None, None]
        u = (rng.standard_normal((nt, nz, ny, nx)) * scale).astype(real)
        v = (rng.standard_normal((nt, nz, ny, nx)) * scale).astype(real)
        u[nt - 1, :, ny // 2, nx // 3] = 1000.
        j0, j1 = ny // 2, min(ny, ny // 2 + 3)
        u[:, :, j0:j1, 10:20] = numpy.nan
        v[:, :, j0:j1, 10:20] = FILL
        u[:, :, 0:2, 0:3] = FILL
        v[:, :, 0:2, 0:3] = numpy.nan
        u[:, nz - 1, ny - 1, nx - 2:] = numpy.nan
        _CASES[key] = (dg.bounds_lon, dg.bounds_lat, dg.deptht_bounds, torch.from_numpy(u).cuda(), torch.from_numpy(v).cuda(),
                       _transects(nx, ny))
    return _CASES[key]


@contextlib.contextmanager
def _knobs(interleaved, field_split):
    """batch_steps = 0: the per-step pass (a grid this small would take all steps in one launch)"""
    from nemoflux_amd._lib import lib, check
    try:
        check(lib.nf_tuning_set(b'batch_steps', 0))
        check(lib.nf_tuning_set(b'field_split', field_split))
        check(lib.nf_tuning_set(b'pass_inner_interleaved', interleaved))
        yield
    finally:
        check(lib.nf_tuning_set(b'pass_inner_interleaved', DEFAULT))
        check(lib.nf_tuning_set(b'field_split', -1))
        check(lib.nf_tuning_set(b'batch_steps', 1))


DEFAULT = -1   # the library's default of "pass_inner_interleaved": by the dtype of uo / vo


def _make(args, **kw):
    return _field(*args, fill_value=FILL, readback=False, **kw)


def _run_pass(f, nt, out=None):
    """rows (nt, rowlen) of one nf_field_compute_all_async"""
    import torch
    from nemoflux_amd._lib import lib, check
    if out is None:
        out = torch.full((nt, f._rowlen), numpy.nan, dtype=torch.float64, device='cuda')
        torch.cuda.synchronize()
    check(lib.nf_field_compute_all_async(ctypes.byref(f._h), ctypes.c_void_p(out.data_ptr())))
    check(lib.nf_synchronize())
    return out.cpu().numpy()


def _planes(f):
    """the six resident planes as they lie in HBM (nf_field_device_ptr), and read_step's view of them with the running max"""
    from nemoflux_amd._lib import lib, check
    n = f.ny * f.nx
    iv, ab = numpy.empty(4 * n), numpy.empty(2 * n)
    for which, host in ((0, iv), (1, ab)):
        p = ctypes.c_void_p()
        check(lib.nf_field_device_ptr(ctypes.byref(f._h), which, ctypes.byref(p)))
        check(lib.nf_synchronize())
        check(lib.nf_memcpy_d2h(host.ctypes.data, p, host.nbytes))
    return (iv, ab) + _resident(f)


def _step_rows(f, steps, rowlen):
    from nemoflux_amd import _lib
    from nemoflux_amd._lib import lib, check
    rows = numpy.zeros((len(steps), rowlen))
    for k, t in enumerate(steps):
        check(lib.nf_field_compute_flux(ctypes.byref(f._h), int(t), _lib.dptr(rows[k])))
    return rows


def _assert_same(got, want, what):
    assert len(got) == len(want)
    for k, (a, b) in enumerate(zip(got, want)):
        assert _same_bits(numpy.atleast_1d(a), numpy.atleast_1d(b)), (what, k)


def _param_id(v):
    return 'x'.join(map(str, v)) if isinstance(v, tuple) else str(v)


@pytest.mark.parametrize('field_split', [0, -1], ids=_param_id)
@pytest.mark.parametrize('real', ['float64', 'float32'])
@pytest.mark.parametrize('shape', SHAPES, ids=_param_id)
def test_interleaved_pass_bit_identical(shape, real, field_split):
    """Rows, resident planes, |.| planes and running max of a pass: knob 1 = knob 0 = per-step compute_flux = (planes) a lone
    compute_flux of the last step; a second pass on the same handle with timing on (direct launches)."""
    nt = shape[3]
    args = _case(shape, real)
    with _knobs(0, field_split):
        f0 = _make(args)
        rows0 = _run_pass(f0, nt)
        res0 = _planes(f0)
    with _knobs(1, field_split):
        f1 = _make(args)
        rows1 = _run_pass(f1, nt)
        res1 = _planes(f1)
        assert _same_bits(rows1, rows0), 'rows: knob 1 against knob 0'
        _assert_same(res1, res0, 'resident state: knob 1 against knob 0')
        # per-step rows on one handle: its running max is that of all the steps, its planes those of the last
        fs = _make(args)
        assert _same_bits(rows1, _step_rows(fs, range(nt), f1._rowlen)), 'rows against per-step compute_flux'
        _assert_same(res1, _planes(fs), 'resident state against per-step compute_flux')
        # a lone compute_flux of the last step on a fresh handle (the large value of the last step is the max of both)
        fl = _make(args)
        _step_rows(fl, [nt - 1], f1._rowlen)
        _assert_same(res1, _planes(fl), 'resident state against a lone compute_flux of the last step')
        # a second pass on the same handle, with per-launch timing (never a graph)
        f1.enableKernelTiming(True)
        assert _same_bits(_run_pass(f1, nt), rows0), 'second pass, timing on'
        n, ms = f1.readKernelTiming()
        f1.enableKernelTiming(False)
        assert n == nt
        _assert_same(_planes(f1), res0, 'resident state after the second pass')


@pytest.mark.parametrize('real', ['float64', 'float32'])
def test_interleaved_pass_default_knob(real):
    """The library's own setting (by dtype) against the knob at 0, and a value the knob does not take."""
    from nemoflux_amd._lib import lib
    shape = SHAPES[2]
    args = _case(shape, real)
    with _knobs(0, 0):
        f0 = _make(args)
        rows0 = _run_pass(f0, shape[3])
        res0 = _planes(f0)
    with _knobs(DEFAULT, 0):
        f1 = _make(args)
        assert _same_bits(_run_pass(f1, shape[3]), rows0)
        _assert_same(_planes(f1), res0, 'resident state: default against knob 0')
    assert lib.nf_tuning_set(b'pass_inner_interleaved', 2) != 0


@pytest.mark.parametrize('real', ['float64', 'float32'])
@pytest.mark.parametrize('shape', SHAPES, ids=_param_id)
def test_interleaved_pass_captured_and_replayed(shape, real):
    """Timing off on a real stream: the pass is captured, then replayed twice; every run gives the rows and the resident
    state of direct launches with the knob at 0."""
    import torch
    nt = shape[3]
    args = _case(shape, real)
    with _knobs(0, 0):
        f0 = _make(args)
        rows0 = _run_pass(f0, nt)
        res0 = _planes(f0)
    st = torch.cuda.Stream()
    torch.cuda.synchronize()
    with torch.cuda.stream(st), _knobs(1, 0):
        g = _make(args, stream=st.cuda_stream)
        out = torch.zeros((nt, g._rowlen), dtype=torch.float64, device='cuda')
        for rep in range(3):
            out.fill_(numpy.nan)
            st.synchronize()
            assert _same_bits(_run_pass(g, nt, out), rows0), ('captured pass', rep)
            _assert_same(_planes(g), res0, ('resident state of the captured pass', rep))
    torch.cuda.synchronize()


@pytest.mark.parametrize('real', ['float64', 'float32'])
@pytest.mark.parametrize('shape', SHAPES, ids=_param_id)
def test_interleaved_pass_sharded_range(shape, real):
    """A slab range that cuts inside the first and the last step it touches: the partial steps stay on their own path, the
    whole steps between them pair up as in a full pass."""
    nx, ny, nz, nt = shape
    args = _case(shape, real)
    sr = (1, nt * nz - 1)
    with _knobs(0, 0):
        f0 = _make(args, slab_range=sr)
        rows0 = _run_pass(f0, nt)
        res0 = _planes(f0)
    with _knobs(1, 0):
        f1 = _make(args, slab_range=sr)
        assert _same_bits(_run_pass(f1, nt), rows0), 'rows: knob 1 against knob 0'
        _assert_same(_planes(f1), res0, 'resident state: knob 1 against knob 0')
        fs = _make(args, slab_range=sr)
        assert _same_bits(_step_rows(fs, range(nt), f1._rowlen), rows0), 'rows against per-step compute_flux'
        _assert_same(_planes(fs), res0, 'resident state against per-step compute_flux')
        assert _same_bits(_run_pass(f1, nt), rows0), 'second pass'
        _assert_same(_planes(f1), res0, 'resident state after the second pass')
