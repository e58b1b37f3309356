"""Re-use of one nf_field handle around the transports in depth bins (nf_field_compute_depth_transport): class -> depth ->
joint -> depth on one handle, a cell thickness set and cleared in between, then another dtype, more levels and other depth
edges.  The depth rows share the run sums of the class forms and have edges of their own: every depth result has the bits of a
fresh handle that makes that call alone, and the class, joint, gross and crossings results and the resident planes are the same
bytes with and without the depth calls in between."""
import ctypes

import numpy
import pytest

from gpu_helpers import _same_bits
from depth_remap_reference import depth_thickness
from gross_reference import THFILL, THMISSING, gross_velocities
from test_gpu_reuse import TRANSECTS
from test_gpu_reuse_products import ProductHandle

pytestmark = pytest.mark.gpu

FILL = 1.e20
NY, NX, NT = 24, 40, 2
dp = ctypes.POINTER(ctypes.c_double)
lin = numpy.linspace


def _state(nz, dtype, seed, ea, eb, ec, ed, top, e3_on_device):
    shape = (NT, nz, NY, NX)
    u, v = gross_velocities(dtype, shape, seed=seed)
    rng = numpy.random.default_rng(seed + 1)
    A = (5. + 2. * rng.standard_normal(shape)).astype(dtype)
    B = (rng.integers(0, 2048, shape) / 512. + numpy.arange(nz)[None, :, None, None]).astype(dtype)
    A[:, :, 3:6, 5:9] = numpy.nan
    B[:, :, 10:12, 20:30] = numpy.nan
    e3u, e3v = depth_thickness(dtype, (NT if e3_on_device else 1, nz, NY, NX), seed=seed + 2)
    return dict(nz=nz, u=u, v=v, A=A, B=B, ea=ea, eb=eb, ec=ec, ed=ed, top=top, e3=(e3u, e3v), e3_on_device=e3_on_device)


def _apply(h, s, first):
    if first:
        h.set_bounds(NY, NX, numpy.float64, True)
    h.set_cell_thickness(None, None, False, None)
    h.set_thickness(numpy.linspace(0.25, 2., s['nz']))
    h.set_uv(s['u'], s['v'], True, FILL)
    h.set_tracer(s['A'], True, None)
    h.set_class_tracer(s['B'], True, None)
    if first:
        for line in TRANSECTS[:3]:
            h.add_transect(line)
        h.call('build_weights', 128, 360.)
    h.call('set_joint_class_edges', s['ea'].ctypes.data_as(dp), s['ea'].size, s['eb'].ctypes.data_as(dp), s['eb'].size)
    h.set_class_edges(s['ec'])
    h.call('set_depth_edges', s['ed'].ctypes.data_as(dp), s['ed'].size, s['top'])


def _cell(h, s, on):
    if on:
        h.set_cell_thickness(s['e3'][0], s['e3'][1], s['e3_on_device'], THFILL)
        h.call('set_cell_thickness_missing_value', THMISSING)
    else:
        h.set_cell_thickness(None, None, False, None)


def _both(h, name, nrows):
    """the volume and the carried form of a call that takes a carry flag"""
    out = []
    for carry in (0, 1):
        r = numpy.full((nrows, h.rowlen()), numpy.nan)
        h.call(name, 1, carry, r.ctypes.data_as(dp))
        out.append(r)
    return numpy.array(out)


def _depth(h, s):
    return _both(h, 'compute_depth_transport', s['ed'].size + 2)


def _class(h, s):
    out = []
    for name in ('compute_class_transport', 'compute_class_tracer_transport'):
        r = numpy.full((s['ec'].size + 2, h.rowlen()), numpy.nan)
        h.call(name, 1, r.ctypes.data_as(dp))
        out.append(r)
    return numpy.array(out)


def _joint(h, s):
    return _both(h, 'compute_joint_class_transport', (s['ea'].size + 2) * (s['eb'].size + 2))


def _crossings(h, s):
    n = ctypes.c_size_t()
    h.call('num_crossings', ctypes.byref(n))
    out = numpy.full((4, s['nz'], n.value), numpy.nan)
    h.call('compute_crossings', 1, 1, out.ctypes.data_as(dp))
    return out


def _planes(h, kind):
    return numpy.concatenate([numpy.ravel(x) for x in h.compute(kind, 1, NY * NX) if x is not None])


def _run(h, s, with_depth):
    """the sequence of one state; the depth calls are made only `with_depth`"""
    out, depth = {}, {}

    def d(key):
        if with_depth:
            depth[key] = _depth(h, s)

    out['class'] = _class(h, s)
    d('scalar 1')
    out['joint'] = _joint(h, s)
    d('scalar 2')
    out['flux'] = _planes(h, 'flux')
    d('scalar 3')
    out['planes'] = _planes(h, 'read')
    _cell(h, s, True)
    d('cell 1')
    out['gross'] = _both(h, 'compute_gross_profile', 2 * s['nz'])
    out['crossings'] = _crossings(h, s)
    d('cell 2')
    out['planes under the cell thickness'] = _planes(h, 'read')
    _cell(h, s, False)
    d('scalar 4')
    out['class again'] = _class(h, s)
    return out, depth


def test_class_depth_joint_depth_on_one_handle_equal_fresh_handles():
    states = [_state(3, numpy.float64, 71, lin(3., 7., 2), lin(1., 5., 3), lin(0., 6., 5), lin(0.5, 5., 4), 0.0, False),
              # another dtype, more levels, more rows than a window, a time-varying thickness in HBM
              _state(7, numpy.float32, 73, lin(1., 9., 33), lin(1., 9., 9), lin(0., 10., 1025), numpy.arange(80) / 4., -1.5, True),
              # fewer levels, other edges
              _state(5, numpy.float64, 79, lin(2., 8., 4), lin(2., 6., 2), lin(0., 8., 40), lin(1., 9., 33), 0.25, False)]
    h, plain = ProductHandle(), ProductHandle()
    for k, s in enumerate(states):
        _apply(h, s, k == 0)
        _apply(plain, s, k == 0)
        got, depth = _run(h, s, True)
        want, none = _run(plain, s, False)
        assert not none and sorted(got) == sorted(want)
        for key in want:
            assert numpy.isfinite(want[key]).all() and numpy.abs(want[key]).max() > 0, (k, key)
            assert _same_bits(got[key], want[key]), (k, key)
        fresh = {}
        for cell in (False, True):
            f = ProductHandle()
            _apply(f, s, True)
            _cell(f, s, cell)
            fresh[cell] = _depth(f, s)
            assert numpy.isfinite(fresh[cell]).all() and (numpy.abs(fresh[cell]).max(axis=(0, 2)) > 0).sum() >= 3, (k, cell)
            assert not fresh[cell][:, -1].view(numpy.uint64).any()
        assert not numpy.array_equal(fresh[False], fresh[True])
        for key, rows in depth.items():
            assert _same_bits(rows, fresh[key.startswith('cell')]), (k, key)
        # other depth edges on the same handle, and back: the rows follow the latest set
        other = numpy.array([1., 2.5])
        h.call('set_depth_edges', other.ctypes.data_as(dp), other.size, 0.0)
        two = _both(h, 'compute_depth_transport', 4)
        assert numpy.abs(two).max() > 0 and two.shape[1] == 4
        h.call('set_depth_edges', s['ed'].ctypes.data_as(dp), s['ed'].size, s['top'])
        assert _same_bits(_depth(h, s), fresh[False]), k
        assert _same_bits(_class(h, s), want['class']), k
