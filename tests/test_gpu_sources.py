"""nemoflux_amd._sources on the GPU: StepSource over every home an input of a Field can have -- the bytes at the address it
returns for the steps 0, 2, 2, 1, the address itself where the array is read in place, and what it reports about its staging
buffer (a step that is already staged is neither read nor uploaded again) -- and each producer (SigmaProducer,
ThicknessProducer, IsoDepthProducer) run into two different output addresses from host inputs against the raw C call on the
uploaded step, bit for bit: what _DerivedThickness.compute_step and Field.getDepthSurfaces rely on.

nt = 3, nz = 2, ny = 3, nx = 5; float32 and float64."""
import ctypes

import numpy
import pytest

pytestmark = pytest.mark.gpu

NT, NZ, NY, NX = 3, 2, 3, 5
ORDER = (0, 2, 2, 1)
DIMS = (NZ, NY, NX)
NAN = numpy.nan
FILL = -999.


def _other(real):
    return 'float32' if real == 'float64' else 'float64'


def _pinned(shape, dtype):
    from nemoflux_amd.field import Field
    return Field._host_array(None, shape, dtype)


def _values(real, shape, seed=0):
    """distinct numbers that both dtypes hold exactly"""
    return (numpy.arange(int(numpy.prod(shape)), dtype=numpy.float64).reshape(shape) * 0.25 + seed).astype(real)


def _download(ptr, shape, dtype):
    from nemoflux_amd._lib import lib
    out = numpy.empty(shape, dtype)
    assert lib.nf_synchronize() == 0
    assert lib.nf_memcpy_d2h(out.ctypes.data, ptr, out.nbytes) == 0
    return out


def _upload(a):
    from nemoflux_amd import _lib
    a = numpy.ascontiguousarray(a)
    return _lib.DeviceBuffer(a.nbytes).upload(a)


class _Variable(object):
    """the least a file variable is: shape, dtype and read_step(t, out=None) along its first axis; counts its reads"""

    def __init__(self, a):
        self.a, self.shape, self.dtype, self.reads = a, a.shape, a.dtype, 0

    def read_step(self, t, out=None):
        self.reads += 1
        if out is None:
            return self.a[t].copy()
        out[...] = self.a[t]
        return out


# home -> (the array-like, its number of steps, the shape of a step, once, what it holds as (steps, *step shape), the device
# address it is read in place at or None, the stand-in or None, reads of the stand-in per staged step)
def _home(home, real):
    import torch
    from nemoflux_amd import _lib
    series, planes, static = _values(real, (NT,) + DIMS, 1), _values(real, (NT, NY, NX), 2), _values(real, DIMS, 3)
    if home == 'torch':
        t = torch.from_numpy(series).cuda()
        return t, NT, DIMS, False, series, t.data_ptr(), None, 0
    if home == 'devicearray':
        buf = _upload(series)
        return _lib.DeviceArray(buf.ptr, series.shape, series.dtype, keepalive=buf), NT, DIMS, False, series, buf.ptr, None, 0
    if home == 'static-torch':
        t = torch.from_numpy(static).cuda()
        return t, 1, DIMS, False, static[None], t.data_ptr(), None, 0
    if home == 'host':
        return series, NT, DIMS, False, series, None, None, 0
    if home == 'swapped':
        return series.astype(series.dtype.newbyteorder('S')), NT, DIMS, False, series, None, None, 0
    if home == 'planes':
        return planes, NT, (NY, NX), False, planes, None, None, 0
    if home in ('static3', 'static3-once'):
        return static, 1, DIMS, home.endswith('once'), static[None], None, None, 0
    if home in ('static4', 'static4-once'):
        return static[None], 1, DIMS, home.endswith('once'), static[None], None, None, 0
    if home == 'cast-once':
        a = _values(_other(real), DIMS, 4) + 1.e-9        # not a float32 number: the cast rounds
        return a, 1, DIMS, True, a.astype(real)[None], None, None, 0
    if home == 'file4':
        var = _Variable(series)
        return var, NT, DIMS, False, series, None, var, 1
    if home == 'file3-static':        # no time axis: read_step walks the levels
        var = _Variable(static)
        return var, 1, DIMS, False, static[None], None, var, NZ
    if home == 'file4-static-once':
        var = _Variable(static[None])
        return var, 1, DIMS, True, static[None], None, var, 1
    raise AssertionError(home)


HOMES = ('torch', 'devicearray', 'static-torch', 'host', 'swapped', 'planes', 'static3', 'static4', 'static3-once', 'static4-once',
         'cast-once', 'file4', 'file3-static', 'file4-static-once')


@pytest.mark.parametrize('home', HOMES)
@pytest.mark.parametrize('real', ['float64', 'float32'])
def test_step_source_returns_the_step_from_every_home(real, home):
    from nemoflux_amd._sources import StepSource
    src, nt, dims, once, want, base, var, reads_per_step = _home(home, real)
    source = StepSource(src, nt, dims, real, _pinned, once=once)
    nbytes = int(numpy.prod(dims)) * numpy.dtype(real).itemsize
    assert source.nbytes == nbytes
    in_place = base is not None or once
    if once and base is None:       # uploaded when it was built, and never again
        base = source.ptr
        assert var is None or var.reads == 1
    staged, reads = None, 0 if var is None else var.reads
    for t in ORDER:
        ptr, wrote = source.step(t)
        held = t if nt > 1 else 0
        got = _download(ptr, dims, real)
        assert got.dtype == want.dtype and got.tobytes() == want[held].tobytes(), (home, t)
        if in_place:
            assert ptr == base + held * nbytes and wrote is False, (home, t)
        else:
            assert wrote is (held != staged), (home, t, staged)     # a step that is staged already is not staged again
            if var is not None:
                reads += reads_per_step if wrote else 0
            staged = held
        assert var is None or var.reads == reads, (home, t, var.reads, reads)
    if not in_place:
        assert ptr == source.dev.ptr and source.pinned.shape == tuple(dims) and source.pinned.dtype == numpy.dtype(real)


# ---- the producers ---------------------------------------------------------------------------------------------------------
def _layout(real):
    from nemoflux_amd._lib import NF_F32, NF_F64
    from nemoflux_amd._sources import Layout
    return Layout(NT, NZ, NY, NX, numpy.dtype(real), NF_F32 if real == 'float32' else NF_F64, None, _pinned)


def _two_outputs(run, raw, shape, real):
    """run(t, ptr) into two addresses: t = 1 into A, t = 1 into B (its inputs are staged already), t = 2 into A; A and B
    against raw(t), the C call on the uploaded step"""
    from nemoflux_amd import _lib
    nbytes = int(numpy.prod(shape)) * numpy.dtype(real).itemsize
    A, B = _lib.DeviceBuffer(nbytes), _lib.DeviceBuffer(nbytes)
    for buf in (A, B):
        assert _lib.lib.nf_memset(buf.ptr, 0x55, nbytes) == 0
    run(1, A)
    a1 = _download(A.ptr, shape, real)
    run(1, B)
    run(2, A)
    a2, b1 = _download(A.ptr, shape, real), _download(B.ptr, shape, real)
    want1, want2 = raw(1), raw(2)
    assert not numpy.array_equal(want1, want2, equal_nan=True)
    assert a1.tobytes() == want1.tobytes() and b1.tobytes() == want1.tobytes() and a2.tobytes() == want2.tobytes()


@pytest.mark.parametrize('real', ['float64', 'float32'])
def test_sigma_producer_is_the_raw_call_whatever_the_output_address(real):
    from nemoflux_amd._lib import lib
    from nemoflux_amd._sources import SigmaProducer
    from nemoflux_amd.eos import Sigma
    g = _layout(real)
    rng = numpy.random.default_rng(11)
    theta = rng.uniform(-2., 30., (NT,) + DIMS).astype(real)
    salt = rng.uniform(30., 38., (NT,) + DIMS).astype(real)
    theta[:, 0, 1, 2], salt[1, 1, 0, 0] = FILL, NAN
    producer = SigmaProducer(g, Sigma(theta, salt, 2000., fill_value=FILL))
    assert len(producer.sources) == 2 and all(s.ptr is None for s in producer.sources) and producer.out.nbytes == producer.nbytes

    def raw(t):
        th, sa, out = _upload(theta[t]), _upload(salt[t]), _upload(numpy.zeros(DIMS, real))
        assert lib.nf_sigma_eos80(out.ptr, th.ptr, sa.ptr, NZ * NY * NX, g.code, 2000., FILL, NAN, NAN, NAN, NAN, None) == 0
        return _download(out.ptr, DIMS, real)

    _two_outputs(lambda t, buf: producer.run(t, buf.ptr), raw, DIMS, real)


@pytest.mark.parametrize('kind', ['face', 'ssh'])
@pytest.mark.parametrize('real', ['float64', 'float32'])
def test_thickness_producer_is_the_raw_call_whatever_the_output_addresses(real, kind):
    from nemoflux_amd import _lib
    from nemoflux_amd._lib import lib
    from nemoflux_amd._sources import ThicknessProducer
    from nemoflux_amd.thickness import FaceThickness, SshThickness
    g = _layout(real)
    rng = numpy.random.default_rng(12)
    e3t = rng.uniform(0.5, 20., (NT,) + DIMS).astype(real)
    e3t[:, 1, 2, 4], e3t[2, 0, 0, 0] = FILL, NAN
    ssh = rng.uniform(-1., 1., (NT, NY, NX)).astype(real)
    e3u0, e3v0 = rng.uniform(0.5, 20., DIMS).astype(real), rng.uniform(0.5, 20., DIMS).astype(real)
    if kind == 'face':
        producer = ThicknessProducer.face(g, FaceThickness(e3t, 'min', fill_value=FILL), NT)
    else:
        producer = ThicknessProducer.ssh(g, SshThickness(ssh, e3u0, e3v0), NT)
    assert producer.src.ptr is None and len(producer.out) == 2

    def raw(t):
        u, v = _upload(numpy.zeros(DIMS, real)), _upload(numpy.zeros(DIMS, real))
        if kind == 'face':
            src = _upload(e3t[t])
            assert lib.nf_face_thickness(u.ptr, v.ptr, src.ptr, None, None, None, NZ, NY, NX, g.code, _lib.NF_E3_MIN, 1, FILL, NAN,
                                         NAN, NAN, None) == 0
        else:
            src, su, sv = _upload(ssh[t]), _upload(e3u0), _upload(e3v0)
            hu, hv = _upload(numpy.zeros((NY, NX))), _upload(numpy.zeros((NY, NX)))
            for h, s in ((hu, su), (hv, sv)):
                assert lib.nf_column_depth(h.ptr, s.ptr, NZ, NY, NX, g.code, NAN, NAN, None) == 0
            assert lib.nf_ssh_thickness(u.ptr, v.ptr, src.ptr, su.ptr, sv.ptr, hu.ptr, hv.ptr, None, None, None, NZ, NY, NX,
                                        g.code, 1, NAN, NAN, NAN, NAN, None) == 0
        return numpy.stack([_download(u.ptr, DIMS, real), _download(v.ptr, DIMS, real)])

    def run(t, buf):        # e3u and e3v side by side in one buffer
        producer.run(t, buf.ptr, buf.ptr + producer.nbytes)

    _two_outputs(run, raw, (2,) + DIMS, real)


@pytest.mark.parametrize('tracer', ['array', 'sigma'])
@pytest.mark.parametrize('real', ['float64', 'float32'])
def test_iso_depth_producer_is_the_raw_call_whatever_the_output_address(real, tracer):
    from nemoflux_amd._lib import lib
    from nemoflux_amd._sources import IsoDepthProducer
    from nemoflux_amd.eos import Sigma
    from nemoflux_amd.surfaces import IsoDepth
    g = _layout(real)
    rng = numpy.random.default_rng(13)
    theta = (20. - 8. * numpy.arange(NZ)[None, :, None, None] + rng.uniform(-3., 3., (NT,) + DIMS)).astype(real)
    salt = rng.uniform(34., 36., (NT,) + DIMS).astype(real)
    e3t = rng.uniform(5., 15., (NT,) + DIMS).astype(real)
    theta[:, :, 0, 3] = NAN
    top = -1.5
    if tracer == 'array':
        values, sense = [17.5, 12.0], -1
        iso = IsoDepth(theta, values, sense, e3t=e3t)
    else:
        values, sense = [25.5, 27.0], 1
        iso = IsoDepth(Sigma(theta, salt, 0.), values, sense, e3t=e3t)
    producer = IsoDepthProducer(g, iso, NT, None, top)
    shape = (len(values), NY, NX)
    assert producer.out.nbytes == int(numpy.prod(shape)) * numpy.dtype(real).itemsize and producer.thickness is None

    def raw(t):
        tau, thk, out = _upload(theta[t]), _upload(e3t[t]), _upload(numpy.zeros(shape, real))
        if tracer == 'sigma':
            sa = _upload(salt[t])
            assert lib.nf_sigma_eos80(tau.ptr, tau.ptr, sa.ptr, NZ * NY * NX, g.code, 0., NAN, NAN, NAN, NAN, NAN, None) == 0
        v = (ctypes.c_double * len(values))(*values)
        assert lib.nf_iso_depth(out.ptr, tau.ptr, None, thk.ptr, NZ, NY, NX, g.code, NAN, NAN, NAN, NAN, top, v, len(values), sense,
                                0, iso.zref, NAN, None) == 0
        return _download(out.ptr, shape, real)

    _two_outputs(lambda t, buf: producer.run(t, buf.ptr), raw, shape, real)
