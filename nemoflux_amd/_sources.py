"""The inputs a Field computes from one time step at a time: where step t of an array lives (StepSource) and the three derived
products built on it -- potential density (SigmaProducer), the e3u / e3v pair of a FaceThickness or an SshThickness
(ThicknessProducer) and the planes of an IsoDepth (IsoDepthProducer).  Each producer owns its sources and its output buffers
and has one call, run(t, *out_ptrs), that issues its C calls on the Field's stream and drains the stream if and only if a
staging buffer was written (it is written again by the next step).  The checks of shapes and dtypes, with their words, are
the Field's: nothing here is built before they passed."""
import collections
import ctypes

import numpy

from . import _lib
from ._lib import lib, check

# what a producer needs to know of its Field: the sizes, the dtype of uo / vo as numpy has it and as the C ABI has it, the HIP
# stream and the allocator of pinned host arrays (Field._host_array)
Layout = collections.namedtuple('Layout', 'nt nz ny nx dtype code stream host_array')


def _native(a):
    """C-contiguous host array in native byte order (files may be big-endian: NetCDF classic, some HDF5)."""
    a = numpy.ascontiguousarray(a)
    return a if a.dtype.isnative else a.astype(a.dtype.newbyteorder('='))


def _nan_if_none(seq):
    """markers as the C ABI takes them: NaN stands for 'none'"""
    return tuple(numpy.nan if m is None else m for m in seq)


class StepSource(object):
    """nt (1: static, read at t = 0 whatever step is asked for) steps of an array, a step of which is shaped dims and must be
    of dtype on the device.  step(t) -> (the device address of step t, whether a staging buffer was written):
      * a torch CUDA tensor or a DeviceArray is read in place at ptr + t * nbytes;
      * a host array (any byte order) goes step by step through one pinned buffer into one device buffer;
      * a file variable does too, by read_step(t, out=pinned); one without a time axis (its rank is that of dims) is static and
        read_step walks its first axis, so it is read slice by slice;
      * once=True (static only): read (read_step(0) of a file variable), cast to dtype and uploaded here, once, without a
        pinned buffer, and read in place from then on.
    The step that is staged is remembered: asking for it again reads and writes nothing.  What is borrowed is kept alive; the
    pinned buffer and the device buffer are the object's own."""

    def __init__(self, src, nt, dims, dtype, host_array, once=False):
        self.nt, self.dims, self.dtype = int(nt), tuple(int(d) for d in dims), numpy.dtype(dtype)
        self.nbytes = int(numpy.prod(self.dims)) * self.dtype.itemsize
        self.keep = src      # a borrowed buffer must outlive the handle
        self.ptr = _lib.device_pointer(src)
        self.held = -1
        if self.ptr is not None:
            return
        if once:
            if hasattr(src, 'read_step'):
                src = src.read_step(0)       # a packed variable of fewer than 4 dimensions decodes whole
            self.keep = _lib.DeviceBuffer(self.nbytes)
            self.keep.upload(_native(numpy.asarray(src).astype(self.dtype, copy=False)).reshape(self.dims))
            self.ptr = self.keep.ptr
            return
        self.file = hasattr(src, 'read_step')
        self.sliced = self.file and len(src.shape) == len(self.dims)
        self.host = None if self.file else _native(src).reshape((self.nt,) + self.dims)
        self.pinned = host_array(self.dims, self.dtype)
        self.dev = _lib.DeviceBuffer(self.nbytes)

    def step(self, tIndex):
        t = tIndex if self.nt > 1 else 0
        if self.ptr is not None:
            return self.ptr + t * self.nbytes, False
        if self.held == t:
            return self.dev.ptr, False
        if not self.file:
            numpy.copyto(self.pinned, self.host[t])
        elif self.sliced:
            for z in range(self.dims[0]):
                numpy.copyto(self.pinned[z], self.keep.read_step(z))
        else:
            self.keep.read_step(t, out=self.pinned)
        check(lib.nf_memcpy_h2d(self.dev.ptr, self.pinned.ctypes.data, self.nbytes))
        self.held = t
        return self.dev.ptr, True


class SigmaProducer(object):
    """sigma_pref(thetao, so) of a nemoflux_amd.eos.Sigma, one (nz, ny, nx) step at a time by nf_sigma_eos80; `out` is the
    device buffer the Field's slots have it written to.  Missing inputs give NaN."""

    def __init__(self, g, sigma):
        dims = (g.nz, g.ny, g.nx)
        self.n, self.code, self.pref, self.stream = g.nz * g.ny * g.nx, g.code, sigma.pref, g.stream
        self.sources = [StepSource(src, g.nt, dims, g.dtype, g.host_array) for src in sigma.sources]
        self.marks = _nan_if_none(m for pair in sigma.markers for m in pair)
        self.nbytes = self.n * g.dtype.itemsize
        self.out = _lib.DeviceBuffer(self.nbytes)

    def run(self, tIndex, out_ptr):
        (theta, wrote_t), (salt, wrote_s) = [src.step(tIndex) for src in self.sources]
        check(lib.nf_sigma_eos80(out_ptr, theta, salt, self.n, self.code, self.pref, *self.marks, numpy.nan, self.stream))
        if wrote_t or wrote_s:
            check(lib.nf_synchronize())


class ThicknessProducer(object):
    """e3u and e3v of one time step derived from a per-step input -- e3t of a FaceThickness (face) or the sea surface height
    of an SshThickness (ssh) -- and statics that go to the device once, when the producer is built.  kernel(e3u_ptr, e3v_ptr,
    src_ptr) makes the C call; `out` is the pair of (nz, ny, nx) device buffers the Field's slot has it written to.  A static
    input is uploaded once too."""

    def __init__(self, g, kernel, src, nt_src, step_dims, keep):
        self.kernel, self.keep = kernel, keep
        self.nbytes = g.nz * g.ny * g.nx * g.dtype.itemsize
        self.out = (_lib.DeviceBuffer(self.nbytes), _lib.DeviceBuffer(self.nbytes))
        self.src = StepSource(src, nt_src, step_dims, g.dtype, g.host_array, once=nt_src == 1)

    def run(self, tIndex, e3u_ptr, e3v_ptr):
        src, wrote = self.src.step(tIndex)
        self.kernel(e3u_ptr, e3v_ptr, src)
        if wrote:
            check(lib.nf_synchronize())

    @classmethod
    def face(cls, g, ft, nt_src):
        """nf_face_thickness of a nemoflux_amd.thickness.FaceThickness whose e3t has nt_src steps"""
        dims = (g.nz, g.ny, g.nx)
        statics = [StepSource(a, 1, dims, g.dtype, g.host_array, once=True) for a in ft.statics]
        ptrs = [s.ptr for s in statics] + [None] * (3 - len(statics))
        marks = _nan_if_none(ft.markers + ft.static_markers)
        tail = dims + (g.code, ft.code, 1 if ft.wrapX else 0) + marks + (g.stream,)      # (not g: it leads back to the Field)

        def kernel(e3u_ptr, e3v_ptr, src):
            check(lib.nf_face_thickness(e3u_ptr, e3v_ptr, src, *ptrs, *tail))

        return cls(g, kernel, ft.e3t, nt_src, dims, [ft] + statics)

    @classmethod
    def ssh(cls, g, st, nt_src):
        """nf_ssh_thickness of a nemoflux_amd.thickness.SshThickness whose ssh has nt_src steps.  The static face thicknesses
        are given, or derived here from e3t0 by nf_face_thickness with NF_E3_MIN; the column depths are given, or
        nf_column_depth of the face statics over all levels, whatever levels this rank owns."""
        dims, cells, nan = (g.nz, g.ny, g.nx), (g.ny, g.nx), numpy.nan

        def once(a, shape, dtype):
            return StepSource(a, 1, shape, dtype, g.host_array, once=True)

        smarks = _nan_if_none(st.static_markers)
        keep = [st] + [once(a, dims, g.dtype) for a in st.statics]
        statics = [s.ptr for s in keep[1:]]
        if st.from_e3t0:
            # NEMO's partial-step rule for e3u_0 / e3v_0: the thinner of the two cells, 0 beside a cell without a thickness
            nbytes = g.nz * g.ny * g.nx * g.dtype.itemsize
            pair = (_lib.DeviceBuffer(nbytes), _lib.DeviceBuffer(nbytes))
            check(lib.nf_face_thickness(pair[0].ptr, pair[1].ptr, statics[0], None, None, None, g.nz, g.ny, g.nx, g.code,
                                        _lib.NF_E3_MIN, 1 if st.wrapX else 0, *smarks, nan, nan, g.stream))
            keep += list(pair)
            statics, smarks = [pair[0].ptr, pair[1].ptr], (nan, nan)
        depths = []
        for k in (0, 1):
            if st.depths is not None:
                owner = once(st.depths[k], cells, numpy.float64)
            else:
                owner = _lib.DeviceBuffer(g.ny * g.nx * 8)
                check(lib.nf_column_depth(owner.ptr, statics[k], g.nz, g.ny, g.nx, g.code, *smarks, g.stream))
            depths.append(owner.ptr)
            keep.append(owner)
        areas = [None, None, None]
        for k, a in enumerate(st.areas or ()):
            keep.append(once(a, cells, numpy.float64))
            areas[k] = keep[-1].ptr
        tail = dims + (g.code, 1 if st.wrapX else 0) + _nan_if_none(st.markers) + smarks + (g.stream,)     # (not g, as above)

        def kernel(e3u_ptr, e3v_ptr, src):
            check(lib.nf_ssh_thickness(e3u_ptr, e3v_ptr, src, *statics, *depths, *areas, *tail))

        return cls(g, kernel, st.ssh, nt_src, cells, keep)


class IsoDepthProducer(object):
    """The m planes of a nemoflux_amd.surfaces.IsoDepth of one time step by nf_iso_depth, from its tracer -- a StepSource, or a
    SigmaProducer when the tracer is a Sigma -- and its e3t of nt_e3t steps (None: no e3t, the per-level thicknesses
    `thickness` from the host instead), with depths measured from `top`.  `out` is the (m, ny, nx) device buffer the Field has
    them written to; `host` is the Field's note of which step of them it holds on the host."""

    def __init__(self, g, iso, nt_e3t, thickness, top):
        from .eos import Sigma
        dims, nan = (g.nz, g.ny, g.nx), numpy.nan
        self.iso, self.top, self.host = iso, top, None
        self.sizes, self.code, self.stream = dims, g.code, g.stream
        self.sigma = self.tracer = self.e3t = self.thickness = None
        if isinstance(iso.tracer, Sigma):
            self.sigma = SigmaProducer(g, iso.tracer)
        else:
            self.tracer = StepSource(iso.tracer, g.nt, dims, g.dtype, g.host_array)
        self.marks = (nan, nan) if self.sigma is not None else _nan_if_none(iso.markers)
        self.emarks = (nan, nan) if nt_e3t is None else _nan_if_none(iso.e3t_markers)
        if nt_e3t is None:
            self.thickness = numpy.ascontiguousarray(thickness, dtype=numpy.float64)
        else:
            self.e3t = StepSource(iso.e3t, nt_e3t, dims, g.dtype, g.host_array)
        self.values = (ctypes.c_double * iso.m)(*iso.values)
        self.out = _lib.DeviceBuffer(iso.m * g.ny * g.nx * g.dtype.itemsize)

    def run(self, tIndex, out_ptr):
        iso, wrote, e3t = self.iso, False, None
        if self.sigma is not None:
            self.sigma.run(tIndex, self.sigma.out.ptr)
            tau = self.sigma.out.ptr
        else:
            tau, wrote = self.tracer.step(tIndex)
        if self.e3t is not None:
            e3t, wrote_e = self.e3t.step(tIndex)
            wrote = wrote or wrote_e
        check(lib.nf_iso_depth(out_ptr, tau, None if self.thickness is None else _lib.dptr(self.thickness), e3t, *self.sizes,
                               self.code, *self.marks, *self.emarks, self.top, self.values, iso.m, iso.sense,
                               1 if iso.relative else 0, iso.zref, numpy.nan, self.stream))
        if wrote:
            check(lib.nf_synchronize())
        self.host = None
