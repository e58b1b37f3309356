"""Re-use of one nf_field handle around the transports between surfaces (nf_field_compute_surface_transport): depth -> surface
-> class -> surface on one handle, a cell thickness set and cleared in between, then another dtype, more levels, another m and a
larger grid, then back.  The surface rows share the run sums of the class forms and have a state of their own: every surface
result has the bits of a fresh handle that makes that call alone, and the depth, class, joint, gross and crossings results and
the resident planes are the same bytes with and without the surface calls in between.  A static host set belongs to the grid of
its upload: after a set_bounds of another shape every compute is refused until the surfaces are set again or cleared."""
import ctypes

import numpy
import pytest

from gpu_helpers import _same_bits
from depth_remap_reference import depth_thickness
from gross_reference import gross_velocities
from surface_transport_reference import SFILL
from test_gpu_reuse import TRANSECTS
from test_gpu_reuse_depth import _both, _cell, _class, _crossings, _depth, _joint
from test_gpu_reuse_products import ProductHandle

pytestmark = pytest.mark.gpu

FILL = 1.e20
NT = 2
NF_F64, NF_F32 = 0, 1
dp = ctypes.POINTER(ctypes.c_double)
lin = numpy.linspace


def _surfaces(dtype, nt_s, m, ny, nx, seed):
    """m surfaces (nt_s, ny, nx) inside the columns of linspace(0.25, 2, nz): multiples of 1/8, NaN and a marker scattered"""
    rng = numpy.random.default_rng(seed)
    out = []
    for k in range(m):
        a = (numpy.floor(8. * 4.5 * k / m) / 8. + rng.integers(0, 20, (nt_s, ny, nx)) / 8.).astype(dtype)
        a[rng.random(a.shape) < 0.02] = numpy.nan
        a[rng.random(a.shape) < 0.02] = SFILL
        a[rng.random(a.shape) < 0.02] = numpy.inf          # one infinite cell leaves its faces without an edge set
        out.append(a)
    return out


def _state(ny, nx, nz, dtype, seed, m, nt_s, on_device, top, ec, ed):
    shape = (NT, nz, ny, nx)
    u, v = gross_velocities(dtype, shape, seed=seed)
    rng = numpy.random.default_rng(seed + 1)
    A = (5. + 2. * rng.standard_normal(shape)).astype(dtype)
    B = (rng.integers(0, 2048, shape) / 512. + numpy.arange(nz)[None, :, None, None]).astype(dtype)
    A[:, :, 3:6, 5:9] = numpy.nan
    e3u, e3v = depth_thickness(dtype, (1, nz, ny, nx), seed=seed + 2)
    return dict(ny=ny, nx=nx, nz=nz, u=u, v=v, A=A, B=B, ea=lin(3., 7., 2), eb=lin(1., 5., 3), ec=ec, ed=ed, top=top,
                e3=(e3u, e3v), e3_on_device=True, surf=_surfaces(dtype, nt_s, m, ny, nx, seed + 3), nt_s=nt_s, m=m,
                surf_on_device=on_device)


def _set_surfaces(h, s):
    ptrs = (ctypes.c_void_p * s['m'])(*[h.lend(a, s['surf_on_device']) for a in s['surf']])
    h.call('set_depth_surfaces', ptrs, s['m'], s['nt_s'], NF_F32 if s['u'].dtype == numpy.float32 else NF_F64,
           int(s['surf_on_device']), SFILL, s['top'])
    h.call('set_depth_surfaces_missing_value', float('nan'))
    h.call('set_depth_surfaces_wrap', 1)


def _apply(h, s, first, surfaces=True, between=None):
    h.set_cell_thickness(None, None, False, None)
    h.set_bounds(s['ny'], s['nx'], numpy.float64, True)
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
    if between:
        between()
    if surfaces:
        _set_surfaces(h, s)


def _surface(h, s):
    return _both(h, 'compute_surface_transport', s['m'] + 2)


def _planes(h, s, kind):
    return numpy.concatenate([numpy.ravel(x) for x in h.compute(kind, 1, s['ny'] * s['nx']) if x is not None])


def _run(h, s, with_surface):
    """the sequence of one state; the surface calls are made only `with_surface`"""
    out, surf = {}, {}

    def d(key):
        if with_surface:
            surf[key] = _surface(h, s)

    out['depth'] = _depth(h, s)
    d('scalar 1')
    out['class'] = _class(h, s)
    d('scalar 2')
    out['joint'] = _joint(h, s)
    out['flux'] = _planes(h, s, 'flux')
    d('scalar 3')
    out['planes'] = _planes(h, s, 'read')
    _cell(h, s, True)
    d('cell 1')
    out['gross'] = _both(h, 'compute_gross_profile', 2 * s['nz'])
    out['depth under the cell thickness'] = _depth(h, s)
    out['crossings'] = _crossings(h, s)
    d('cell 2')
    out['planes under the cell thickness'] = _planes(h, s, 'read')
    _cell(h, s, False)
    d('scalar 4')
    out['class again'] = _class(h, s)
    out['depth again'] = _depth(h, s)
    return out, surf


def test_depth_surface_class_surface_on_one_handle_equal_fresh_handles():
    states = [_state(24, 40, 3, numpy.float64, 171, 2, 1, False, 0.0, lin(0., 6., 5), lin(0.5, 5., 4)),
              # another dtype, more levels, another m, a larger grid, time-varying surfaces in HBM
              _state(30, 48, 7, numpy.float32, 173, 8, NT, True, -1.5, lin(0., 10., 1025), numpy.arange(80) / 4.),
              # back to the first grid: fewer levels, a time-varying host set
              _state(24, 40, 5, numpy.float64, 179, 3, NT, False, 0.25, lin(0., 8., 40), lin(1., 9., 33))]
    h, plain = ProductHandle(), ProductHandle()
    rows = numpy.zeros(4096)
    for k, s in enumerate(states):
        def stale():
            # state 0 left a static host set uploaded for 24 x 40: on the larger grid every compute is refused until it is set again
            if k == 1:
                for name, args in (('compute_flux', (1, rows.ctypes.data_as(dp))),
                                   ('compute_depth_transport', (1, 0, rows.ctypes.data_as(dp))),
                                   ('compute_surface_transport', (1, 0, rows.ctypes.data_as(dp)))):
                    assert h.raw(name, *args) == 2, name
                    words = h.lib.nf_last_error().decode()
                    assert 'nf_field_set_depth_surfaces' in words and '(24, 40)' in words and '(30, 48)' in words, words
                assert not rows.any()
        _apply(h, s, k == 0, between=stale)
        _apply(plain, s, k == 0, surfaces=False)
        got, surf = _run(h, s, True)
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
            fresh[cell] = _surface(f, s)
            assert numpy.isfinite(fresh[cell]).all() and (numpy.abs(fresh[cell]).max(axis=(0, 2)) > 0).sum() >= 3, (k, cell)
            assert numpy.abs(fresh[cell][:, -1]).max() > 0                       # faces without an edge set
        assert not numpy.array_equal(fresh[False], fresh[True])
        for key, r in surf.items():
            assert _same_bits(r, fresh[key.startswith('cell')]), (k, key)
        # cleared and set again on the same handle: refused in between, then the rows of the fresh handle
        h.call('set_depth_surfaces', None, 0, 0, NF_F64, 0, float('nan'), 0.0)
        assert h.raw('compute_surface_transport', 1, 0, rows.ctypes.data_as(dp)) == 2
        assert 'set_depth_surfaces first' in h.lib.nf_last_error().decode()
        assert _same_bits(_depth(h, s), want['depth']), k
        _set_surfaces(h, s)
        assert _same_bits(_surface(h, s), fresh[False]), k
        assert _same_bits(_class(h, s), want['class']), k
