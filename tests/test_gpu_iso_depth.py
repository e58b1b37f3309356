"""Isosurface and mixed-layer depths on the GPU, the raw ABI: nf_iso_depth against the numpy restatement of
tests/iso_depth_reference.py bit for bit -- every operation of the definition is one correctly rounded IEEE float64 operation
in a fixed order, and the device's float64 division is correctly rounded (tests/test_gpu_eos.py) -- on the inputs whose branch
coverage tests/test_iso_depth_cpu.py asserts: (ny, nx) = (36, 72) and (37, 73), nz = 1, 7 and 75, a launch of 5 columns, m = 1,
3 and 8, both dtypes, both senses, absolute and relative mode, the level vector and e3t, both markers and NaN in the tracer and
in e3t, guard words around out, the input pointers moved by one element.  Then the exact identities: what lies below a
column's last k* does not matter, a wave is not left early, m values at once are m calls of one, a broadcast level vector is
the level-vector form."""
import ctypes

import numpy
import pytest

import iso_depth_reference as ref

pytestmark = pytest.mark.gpu

NF_F64, NF_F32 = 0, 1
GUARD = -7.0
CASES = ref.raw_cases()
_DP = ctypes.POINTER(ctypes.c_double)


def _device(a, shift):
    """a host array on the device behind `shift` leading elements: (tensor that owns it, address of a's first element)"""
    import torch
    host = numpy.full(a.size + shift + 4, 3.25, a.dtype)
    host[shift:shift + a.size] = a.reshape(-1)
    t = torch.from_numpy(host).cuda()
    return t, t.data_ptr() + shift * a.dtype.itemsize


def _call(tau, values, sense, thickness=None, e3t=None, top=0.0, relative=False, zref=ref.ZREF, fill_out=numpy.nan, shift=0,
          markers=True):
    """nf_iso_depth on host inputs: the (m, ny, nx) result, with the guard words around out checked"""
    import torch
    from nemoflux_amd._lib import lib
    nz, ny, nx = tau.shape
    m = len(values)
    real = tau.dtype
    pad = 16
    keep_t, tp = _device(tau, shift)
    keep_e, ep = _device(e3t, shift) if e3t is not None else (None, None)
    out = torch.full((m * ny * nx + 2 * pad,), GUARD, dtype=keep_t.dtype, device='cuda')
    hp = None
    if thickness is not None:
        h = numpy.ascontiguousarray(thickness, numpy.float64)
        hp = h.ctypes.data_as(_DP)
    v = (ctypes.c_double * m)(*[float(x) for x in values])
    tm = (ref.TFILL, ref.TMISSING) if markers else (numpy.nan, numpy.nan)
    em = (ref.EFILL, ref.EMISSING) if markers else (numpy.nan, numpy.nan)
    rc = lib.nf_iso_depth(out.data_ptr() + pad * real.itemsize, tp, hp, ep, nz, ny, nx, NF_F32 if real == numpy.float32 else NF_F64,
                          tm[0], tm[1], em[0], em[1], top, ctypes.cast(v, _DP), m, sense, 1 if relative else 0, zref, fill_out,
                          None)
    assert rc == 0, lib.nf_last_error()
    assert lib.nf_synchronize() == 0
    got = out.cpu().numpy()
    assert (got[:pad] == GUARD).all() and (got[pad + m * ny * nx:] == GUARD).all(), 'out was written outside its m planes'
    for keep, a in ((keep_t, tau), (keep_e, e3t)):        # the inputs are only read
        if keep is not None:
            assert ref.same_bits(keep.cpu().numpy()[shift:shift + a.size], a.reshape(-1))
    return got[pad:pad + m * ny * nx].reshape(m, ny, nx)


def _report(got, want, label):
    bad = ~((got == want) | (numpy.isnan(got) & numpy.isnan(want)))
    if bad.any():
        j, y, x = (int(i[0]) for i in numpy.nonzero(bad))
        print(f'{label}: {int(bad.sum())} of {got.size} values differ; first: value {j} column ({y}, {x}) got {got[j, y, x]!r} '
              f'want {want[j, y, x]!r}')
    return not bad.any()


@pytest.mark.parametrize('case', CASES, ids=[ref.case_id(c) for c in CASES])
def test_raw_abi_is_the_restatement_bit_for_bit(case):
    """the bases as the allocator gives them, then moved by one element (4 or 8 bytes: no 16-byte alignment)"""
    real, nz, ny, nx, m, sense, relative, form = case
    tau, thk, e3t, values = ref.make_case(*case)
    kw = dict(thickness=thk, e3t=e3t, relative=relative)
    want = ref.iso_depth(tau, values, sense, top=0.0, zref=ref.ZREF, tau_markers=(ref.TFILL, ref.TMISSING),
                         e3t_markers=(ref.EFILL, ref.EMISSING), **kw)
    for shift in (0, 1):
        got = _call(tau, values, sense, shift=shift, **kw)
        assert _report(got, want, f'{ref.case_id(case)} shift={shift}')
        assert ref.same_bits(got, want)


@pytest.mark.parametrize('sense', [1, -1])
@pytest.mark.parametrize('real', ['float64', 'float32'])
def test_offsets_that_are_not_positive_find_level_kref_past_the_threshold(real, sense):
    """relative mode with offsets <= 0: the 'at zref' outcome, whose share tests/test_iso_depth_cpu.py asserts"""
    tau, e3t, values = ref.atzref_case(real, 37, 73, sense)
    want, branch = ref.iso_depth(tau, values, sense, e3t=e3t, relative=True, zref=ref.ZREF, tau_markers=(ref.TFILL, ref.TMISSING),
                                 e3t_markers=(ref.EFILL, ref.EMISSING), with_branches=True)
    assert (branch[:2] == ref.ATZREF).mean() > 0.01
    got = _call(tau, values, sense, e3t=e3t, relative=True)
    assert _report(got, want, f'at zref {real} {sense}') and ref.same_bits(got, want)


@pytest.mark.parametrize('real', ['float64', 'float32'])
def test_top_fill_out_markers_off_and_the_python_call(real):
    import torch
    from nemoflux_amd._lib import DeviceArray
    from nemoflux_amd.surfaces import iso_depth
    case = (real, 7, 37, 73, 3, -1, True, 'e3t')
    tau, _, e3t, values = ref.make_case(*case)
    marks = dict(tau_markers=(ref.TFILL, ref.TMISSING), e3t_markers=(ref.EFILL, ref.EMISSING))
    want = ref.iso_depth(tau, values, -1, e3t=e3t, top=-3.5, relative=True, zref=7.25, fill_out=1.e20, **marks)
    assert (want == numpy.dtype(real).type(1.e20)).mean() > 0.05
    assert ref.same_bits(_call(tau, values, -1, e3t=e3t, top=-3.5, relative=True, zref=7.25, fill_out=1.e20), want)
    # without markers the marker values are data (and a marker thickness that is negative still ends the column)
    want = ref.iso_depth(tau, values, -1, e3t=e3t, relative=True, zref=ref.ZREF)
    assert ref.same_bits(_call(tau, values, -1, e3t=e3t, relative=True, markers=False), want)
    # the Python call: tensors with a new out, DeviceArrays with out=, the level vector
    d_tau, d_e3t = torch.from_numpy(tau).cuda(), torch.from_numpy(e3t).cuda()
    got = iso_depth(d_tau, values, 'falling', e3t=d_e3t, relative=True, zref=ref.ZREF, **marks)
    torch.cuda.synchronize()
    assert ref.same_bits(got.cpu().numpy(), ref.iso_depth(tau, values, -1, e3t=e3t, relative=True, zref=ref.ZREF, **marks))
    h = ref.level_thickness(7)
    out = torch.empty((3, 37, 73), dtype=d_tau.dtype, device='cuda')
    arrs = [DeviceArray(x.data_ptr(), x.shape, real, keepalive=x) for x in (d_tau, out)]
    assert iso_depth(arrs[0], [12.0, 14.5, 18.0], -1, thickness=h, out=arrs[1], tau_markers=(ref.TFILL, None), top=2.0) is arrs[1]
    torch.cuda.synchronize()
    assert ref.same_bits(out.cpu().numpy(), ref.iso_depth(tau, [12.0, 14.5, 18.0], -1, thickness=h, top=2.0,
                                                          tau_markers=(ref.TFILL,)))
    with pytest.raises(RuntimeError, match='needs out='):
        iso_depth(arrs[0], [1.0], 1, thickness=h)
    with pytest.raises(RuntimeError, match='e3t is'):
        iso_depth(d_tau, [1.0], 1, e3t=d_e3t[:-1])
    with pytest.raises(RuntimeError, match='thickness has 6 numbers'):
        iso_depth(d_tau, [1.0], 1, thickness=h[:-1])


@pytest.mark.parametrize('relative', [False, True])
@pytest.mark.parametrize('real', ['float64', 'float32'])
def test_what_lies_below_the_last_crossing_does_not_matter(real, relative):
    """every level below the last k* of a column (over its m values) overwritten with other wet values: the same bits, where
    every value of the column was found"""
    case = (real, 75, 37, 73, 3, 1, relative, 'levels')
    tau, thk, _, values = ref.make_case(*case)
    marks = dict(tau_markers=(ref.TFILL, ref.TMISSING))
    want, kstar = ref.iso_depth(tau, values, 1, thickness=thk, relative=relative, zref=ref.ZREF, with_kstar=True, **marks)
    got = _call(tau, values, 1, thickness=thk, relative=relative)
    assert ref.same_bits(got, want)
    nwet = numpy.cumprod(ref.present(tau, marks['tau_markers']), axis=0).sum(axis=0)
    last = kstar.max(axis=0)
    done = last < nwet                       # every value has a k* inside the column
    assert 0.3 < done.mean() < 0.95
    lev = numpy.arange(75).reshape(75, 1, 1)
    below = (lev > last) & done
    assert below.mean() > 0.2
    rng = numpy.random.default_rng(3)
    other = tau.copy()
    other[below] = rng.uniform(-50.0, 50.0, int(below.sum())).astype(real)
    got2 = _call(other, values, 1, thickness=thk, relative=relative)
    assert ref.same_bits(got2[:, done], got[:, done])        # NaN by position: +-inf in the tracer gives some
    assert not numpy.array_equal(other, tau)


@pytest.mark.parametrize('real', ['float64', 'float32'])
def test_a_wave_is_not_left_before_its_last_lane_is_done(real):
    """a block of 64 x 4 columns that all outcrop and one column that runs to the bed -- in the middle of a wave, at the end of
    one, and alone behind the block: the restatement's bits"""
    nz = 75
    h = ref.level_thickness(nz)
    values = [10.0, 20.0, 1000.0]
    for deep in (37, 63, 255, 256):
        tau = numpy.full((nz, 1, 257), 2000.0, real)                   # level 0 has reached every value
        tau[:, 0, deep] = numpy.linspace(0.0, 30.0, nz).astype(real)   # 10 and 20 are crossed, 1000 is never: the bed
        want, branch = ref.iso_depth(tau, values, 1, thickness=h, with_branches=True)
        assert (numpy.delete(branch, deep, axis=2) == ref.OUTCROP).all()
        assert list(branch[:, 0, deep]) == [ref.INTERP, ref.INTERP, ref.BED]
        got = _call(tau, values, 1, thickness=h)
        assert numpy.array_equal(got, want), deep
        assert got[2, 0, deep] == numpy.dtype(real).type(h.sum()) and 0 < got[0, 0, deep] < got[1, 0, deep] < got[2, 0, deep]


@pytest.mark.parametrize('case', [('float64', 7, 37, 73, 8, 1, False, 'e3t'), ('float32', 75, 36, 72, 8, -1, True, 'levels'),
                                  ('float32', 7, 37, 73, 8, 1, True, 'e3t')], ids=ref.case_id)
def test_m_values_in_one_call_are_m_calls_of_one_value(case):
    real, nz, ny, nx, m, sense, relative, form = case
    tau, thk, e3t, values = ref.make_case(*case)
    kw = dict(thickness=thk, e3t=e3t, relative=relative)
    together = _call(tau, values, sense, **kw)
    for j, v in enumerate(values):
        assert numpy.array_equal(_call(tau, [v], sense, **kw)[0], together[j], equal_nan=True), j
    assert numpy.array_equal(_call(tau, values[::-1], sense, **kw), together[::-1], equal_nan=True)


@pytest.mark.parametrize('relative', [False, True])
@pytest.mark.parametrize('real', ['float64', 'float32'])
def test_a_broadcast_level_vector_is_the_level_vector_form(real, relative):
    case = (real, 7, 37, 73, 3, -1, relative, 'levels')
    tau, thk, _, values = ref.make_case(*case)
    e3t = numpy.ascontiguousarray(numpy.broadcast_to(thk.astype(real).reshape(7, 1, 1), tau.shape))
    assert (e3t.astype(numpy.float64) == thk.reshape(7, 1, 1)).all()
    a = _call(tau, values, -1, thickness=thk, relative=relative)
    b = _call(tau, values, -1, e3t=e3t, relative=relative)
    assert numpy.isfinite(a).mean() > 0.5 and numpy.array_equal(a, b, equal_nan=True)
