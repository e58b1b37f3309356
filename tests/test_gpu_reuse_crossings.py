"""One nf_field handle of the C ABI driven through the joint classes, the crossings, the gross class transport and the crossings
again -- then with another dtype, more levels, a cell thickness set and cleared, and other transects: every crossings result
equals, bit for bit, that of a fresh handle given the state of the moment alone, and the resident planes and the row of the
last nf_field_compute_flux are the same bytes before and after every crossings call.  The crossings share no buffer with the
term table of the joint / gross class calls, and their own buffer follows the weights and the number of levels."""
import ctypes

import numpy
import pytest

from gross_reference import FILL, THFILL, gross_thickness, gross_velocities
from test_gpu_reuse import TRANSECTS, same_bits
from test_gpu_reuse_products import ProductHandle

pytestmark = pytest.mark.gpu

dp = ctypes.POINTER(ctypes.c_double)
NY, NX, NT = 24, 40, 2


def _state(dtype, nz, seed):
    shape = (NT, nz, NY, NX)
    u, v = gross_velocities(dtype, shape, seed=seed)
    rng = numpy.random.default_rng(seed + 1)
    tau, sig = (4. + rng.standard_normal(shape)).astype(dtype), (30. + 3. * rng.standard_normal(shape)).astype(dtype)
    return dict(u=u, v=v, tau=tau, sig=sig, thick=numpy.linspace(0.25, 1.0, nz), nz=nz, e3=None, lines=TRANSECTS[:2])


def _apply(h, s, on_device, build=True):
    """the state s on handle h; build=False: the fields and the levels alone, the grid and the weights stay"""
    if build:
        h.set_bounds(NY, NX, numpy.float64, False)
    h.set_thickness(s['thick'])
    h.set_uv(s['u'], s['v'], on_device, FILL)
    h.set_tracer(s['tau'], on_device, None)
    h.set_class_tracer(s['sig'], on_device, None)
    if s['e3'] is not None:
        h.set_cell_thickness(s['e3'][0], s['e3'][1], on_device, THFILL)
    if build:
        for ln in s['lines']:
            h.add_transect(ln)
        h.call('build_weights', 16, 360.)


def _ncross(h):
    n = ctypes.c_size_t()
    h.call('num_crossings', ctypes.byref(n))
    return n.value


def _crossings(h, s, t, carry, form):
    import torch
    shape = (4 if carry else 2, s['nz'], _ncross(h))
    if form == 'sync':
        out = numpy.full(shape, numpy.nan)
        h.call('compute_crossings', t, carry, out.ctypes.data_as(dp))
        return out
    dev = torch.full(shape, float('nan'), dtype=torch.float64, device='cuda')
    h.call('compute_crossings_async', t, carry, ctypes.c_void_p(dev.data_ptr()))
    torch.cuda.synchronize()
    return dev.cpu().numpy()


def _flux_row(h, t):
    row = numpy.full(max(h.rowlen(), 1), numpy.nan)
    h.call('compute_flux', t, row.ctypes.data_as(dp))
    return row


def _checked_crossings(h, s, on_device, t=1):
    """both forms, both ways of calling, against a fresh handle; the resident planes and a flux row recomputed after the
    calls are what they were before them"""
    ncell = NY * NX
    row = _flux_row(h, t)
    before = h.planes(ncell)
    fresh = ProductHandle()
    _apply(fresh, s, on_device)
    assert _ncross(fresh) == _ncross(h) > 0
    out = {}
    for carry in (0, 1):
        for form in ('sync', 'async'):
            got = _crossings(h, s, t, carry, form)
            assert numpy.abs(got).max() > 0 and not numpy.isnan(got).any()
            assert same_bits(got, _crossings(fresh, s, t, carry, form)), (carry, form)
            for b, a in zip(before, h.planes(ncell)):
                assert same_bits(b, a), ('the resident planes changed', carry, form)
            out[carry] = got
    assert same_bits(out[0][0], out[1][0])
    for b, a in zip(before, h.planes(ncell)):
        assert same_bits(b, a)
    assert same_bits(_flux_row(h, t), row)
    return out


@pytest.mark.parametrize('on_device', [True, False], ids=['hbm', 'host'])
def test_crossings_between_the_class_products_on_one_handle(on_device):
    s = _state('float64', 5, seed=41)
    h = ProductHandle()
    _apply(h, s, on_device)
    ea, eb = numpy.array([3., 4., 5.]), numpy.array([27., 30., 33.])
    h.call('set_joint_class_edges', ea.ctypes.data_as(dp), ea.size, eb.ctypes.data_as(dp), eb.size)
    h.set_class_edges(numpy.array([28., 30., 32.]))
    rowlen = h.rowlen()
    # 1. joint, 2. crossings, 3. gross class, 4. crossings
    joint = numpy.full(((ea.size + 2) * (eb.size + 2), rowlen), numpy.nan)
    h.call('compute_joint_class_transport', 1, 1, joint.ctypes.data_as(dp))
    first = _checked_crossings(h, s, on_device)
    gross = numpy.full((2, 5, rowlen), numpy.nan)
    h.call('compute_gross_class_transport', 1, 0, gross.ctypes.data_as(dp))
    again = _checked_crossings(h, s, on_device)
    for carry in (0, 1):
        assert same_bits(first[carry], again[carry])
    joint2 = numpy.full(joint.shape, numpy.nan)
    h.call('compute_joint_class_transport', 1, 1, joint2.ctypes.data_as(dp))
    assert same_bits(joint, joint2) and numpy.abs(joint).max() > 0            # the crossings left the term table's users alone
    # another dtype and more levels
    s2 = _state('float32', 7, seed=43)
    _apply(h, s2, on_device, build=False)
    wide = _checked_crossings(h, s2, on_device)
    assert wide[1].shape[1] == 7
    # a cell thickness set, then cleared
    s2['e3'] = gross_thickness('float32', (NT, 7, NY, NX), seed=47)
    h.set_cell_thickness(s2['e3'][0], s2['e3'][1], on_device, THFILL)
    thick = _checked_crossings(h, s2, on_device)
    assert not numpy.array_equal(thick[0], wide[0])
    s2['e3'] = None
    h.set_cell_thickness(None, None, on_device, None)
    cleared = _checked_crossings(h, s2, on_device)
    for carry in (0, 1):
        assert same_bits(cleared[carry], wide[carry])
    # other transects: one more, and the weights built again
    n_before = _ncross(h)
    h.add_transect(TRANSECTS[3])
    n = ctypes.c_size_t()
    assert h.raw('num_crossings', ctypes.byref(n)) == 2 and b'build_weights' in h.lib.nf_last_error()
    out = numpy.full((2, 7, max(n_before, 1)), numpy.nan)
    assert h.raw('compute_crossings', 1, 0, out.ctypes.data_as(dp)) == 2 and b'build_weights' in h.lib.nf_last_error()
    h.call('build_weights', 16, 360.)
    s2['lines'] = TRANSECTS[:2] + [TRANSECTS[3]]
    assert _ncross(h) > n_before
    more = _checked_crossings(h, s2, on_device)
    assert same_bits(more[0][:, :, :n_before], cleared[0])                     # the first two transects' crossings come first
