"""Depth-resolved transect fluxes, the parts that need no GPU: the two C entry points exist and check their arguments and
the call order before touching a device, and Field.depthBandFlux turns a profile into the flux of a depth band."""
import ctypes

import numpy
import pytest

NF_ERR_ARG, NF_ERR_STATE = 1, 2


def test_library_exports_the_profile_calls():
    from nemoflux_amd import _lib
    for name in ('nf_field_compute_profile', 'nf_field_compute_profile_async'):
        assert hasattr(_lib.lib, name), name


def test_profile_calls_check_handle_and_state_without_a_gpu():
    from nemoflux_amd import _lib
    lib = _lib.lib
    out = numpy.zeros(16)
    assert lib.nf_field_compute_profile(None, 0, _lib.dptr(out)) == NF_ERR_ARG
    assert b'null' in lib.nf_last_error()
    assert lib.nf_field_compute_profile_async(None, 0, ctypes.c_void_p(out.ctypes.data)) == NF_ERR_ARG
    h = ctypes.c_void_p()
    assert lib.nf_field_new(ctypes.byref(h)) == 0
    try:
        assert lib.nf_field_compute_profile(ctypes.byref(h), 0, None) == NF_ERR_ARG
        assert lib.nf_field_compute_profile_async(ctypes.byref(h), 0, None) == NF_ERR_ARG
        # an unset handle: nothing to compute from
        assert lib.nf_field_compute_profile(ctypes.byref(h), 0, _lib.dptr(out)) == NF_ERR_STATE
        assert b'set_bounds, set_thickness and set_uv first' in lib.nf_last_error()
        assert lib.nf_field_compute_profile_async(ctypes.byref(h), 0, ctypes.c_void_p(out.ctypes.data)) == NF_ERR_STATE
    finally:
        assert lib.nf_field_del(ctypes.byref(h)) == 0


def _field_with_layers(bounds):
    """A Field shell with only what depthBandFlux reads (the band rule needs no device)."""
    from nemoflux_amd.field import Field
    f = Field.__new__(Field)
    f.bounds_depth = numpy.asarray(bounds, dtype=numpy.float64)
    f.nz = f.bounds_depth.shape[0]
    return f


BOUNDS = [(0., 10.), (10., 30.), (30., 30.), (30., 70.), (70., 150.)]   # layer 2 has zero thickness


def _profile(seed, shape):
    rng = numpy.random.default_rng(seed)
    return rng.standard_normal((len(BOUNDS),) + shape) * 10. ** rng.integers(-3, 4, size=(len(BOUNDS),) + shape)


@pytest.mark.parametrize('shape', [(3,), (4, 2)])
def test_band_at_layer_boundaries_is_the_plain_sum(shape):
    f = _field_with_layers(BOUNDS)
    P = _profile(1, shape)
    for ztop, zbot, levels in ((0., 150., [0, 1, 3, 4]), (10., 70., [1, 3]), (0., 10., [0]), (30., 150., [3, 4]),
                               (10., 30., [1])):
        want = numpy.zeros(shape)
        for z in levels:
            want = want + P[z]
        assert numpy.array_equal(f.depthBandFlux(P, ztop, zbot), want), (ztop, zbot)


def test_half_a_layer_is_half_its_row():
    f = _field_with_layers(BOUNDS)
    P = _profile(2, (5,))
    assert numpy.array_equal(f.depthBandFlux(P, 10., 20.), P[1] * 0.5)
    assert numpy.array_equal(f.depthBandFlux(P, 110., 150.), P[4] * 0.5)
    # a band that cuts two layers: a quarter of layer 3 and the first half of layer 4
    assert numpy.allclose(f.depthBandFlux(P, 60., 110.), P[3] * 0.25 + P[4] * 0.5, rtol=1e-15, atol=0)


def test_band_outside_the_column_is_zero():
    f = _field_with_layers(BOUNDS)
    P = _profile(3, (4,))
    for ztop, zbot in ((150., 400.), (-50., 0.), (200., 300.), (30., 30.)):
        assert numpy.array_equal(f.depthBandFlux(P, ztop, zbot), numpy.zeros(4)), (ztop, zbot)


def test_band_arguments_are_checked():
    f = _field_with_layers(BOUNDS)
    with pytest.raises(ValueError, match='ztop <= zbot'):
        f.depthBandFlux(numpy.zeros((5, 2)), 20., 10.)
    with pytest.raises(ValueError, match='levels first'):
        f.depthBandFlux(numpy.zeros((4, 2)), 0., 10.)


def test_zrange_option_is_parsed():
    from nemoflux_amd.fluxplot import parseZRange
    assert parseZRange('0,1000') == (0., 1000.)
    assert parseZRange(' 1000.5 , 4000') == (1000.5, 4000.)
    for bad in ('1000', '1,2,3', 'a,b', '100,10'):
        with pytest.raises(RuntimeError, match='--zrange'):
            parseZRange(bad)
