"""Depth surfaces derived on the GPU (nf_iso_depth, csrc/nf_isodepth.hip): the depth at which a tracer first reaches a value,
column by column -- the depth of an isotherm or an isopycnal, the mixed-layer depth by a threshold criterion -- computed from
what NEMO writes instead of a 2-D field the user brings.

iso_depth is the raw call on device arrays; IsoDepth and MixedLayerDepth describe derived surfaces to
Field.setDepthSurfaces, which computes them one time step at a time into one (m, ny, nx) device buffer per item -- the full
series is never materialised, a step that is not visited is never read."""
import ctypes
import math

import numpy

from . import _lib
from ._lib import lib, check, NF_F64, NF_F32
from .eos import Sigma, _np_dtype, _marker

_NAN = float('nan')
MAX_SURFACES = 8


def _values(values, what='values'):
    try:
        v = [float(x) for x in numpy.atleast_1d(numpy.asarray(values, dtype=numpy.float64))]
    except (TypeError, ValueError):
        raise RuntimeError(f'ERROR: {what} must be a sequence of numbers, got {values!r}')
    if not 1 <= len(v) <= MAX_SURFACES:
        raise RuntimeError(f'ERROR: {what} must hold 1 to {MAX_SURFACES} numbers (one surface each), got {len(v)}')
    if not all(math.isfinite(x) for x in v):
        raise RuntimeError(f'ERROR: {what} must be finite, got {v}')
    return v


def _sense(sense):
    if sense in ('rising', 'falling'):
        return 1 if sense == 'rising' else -1
    try:
        ok = float(sense) in (1.0, -1.0)
    except (TypeError, ValueError):
        ok = False
    if not ok:
        raise RuntimeError(f'ERROR: sense must be +1 (the tracer rises downward, as density does) or -1 (it falls, as '
                           f'temperature does), got {sense!r}')
    return int(float(sense))


def _finite(x, what):
    x = float(x)
    if not math.isfinite(x):
        raise RuntimeError(f'ERROR: {what} must be a finite number, got {x!r}')
    return x


def _is_device(a):
    import torch
    return isinstance(a, _lib.DeviceArray) or (isinstance(a, torch.Tensor) and a.is_cuda)


def iso_depth(tau, values, sense, thickness=None, e3t=None, top=0.0, relative=False, zref=10.0, out=None,
              tau_markers=(_NAN, _NAN), e3t_markers=(_NAN, _NAN), fill_out=_NAN, stream=None):
    """The depths at which one time step of a tracer first reaches each of `values` going down its columns (nf_iso_depth; the
    definition is in include/nemoflux_amd.h).  tau: a torch CUDA tensor or DeviceArray of shape (nz, ny, nx), float64 or
    float32 (the arithmetic is float64).  values: 1 to 8 finite numbers.  sense: +1, the tracer rises downward (density), or
    -1, it falls (temperature).  The level thicknesses: either thickness, nz numbers (host), or e3t, a device array shaped and
    typed like tau -- exactly one of the two.  top: the depth of the upper interface of level 0.  relative: the values are
    offsets from the tracer's own value at depth zref (the mixed-layer criteria).  tau_markers / e3t_markers: the
    (fill, missing) pair of each array, NaN = none; NaN always counts as missing.  A column without a wet level gets fill_out.
    out: the (m, ny, nx) array that receives the result -- a new torch tensor when tau is a tensor and out is None.
    Asynchronous on `stream` (a HIP stream address; None: the null stream).  Returns out."""
    import torch
    values = _values(values)
    sense = _sense(sense)
    top, zref = _finite(top, 'top'), _finite(zref, 'zref')
    if (thickness is None) == (e3t is None):
        raise RuntimeError('ERROR: iso_depth needs exactly one of thickness (nz numbers) and e3t (a device array like tau)')
    for a, what in ((tau, 'tau'), (e3t, 'e3t'), (out, 'out')):
        if a is None:
            continue
        if not _is_device(a):
            raise RuntimeError(f'ERROR: iso_depth works on torch CUDA tensors or DeviceArrays; {what} is not one (IsoDepth '
                               f'takes host arrays and files)')
        if isinstance(a, torch.Tensor) and not a.is_contiguous():
            raise RuntimeError(f'ERROR: iso_depth needs contiguous tensors; {what} is not')
    shape, dt = tuple(int(x) for x in tau.shape), _np_dtype(tau)
    if len(shape) != 3 or min(shape) < 1:
        raise RuntimeError(f'ERROR: iso_depth: tau has shape {shape}; need (nz, ny, nx), each >= 1')
    if dt not in (numpy.float64, numpy.float32):
        raise RuntimeError(f'ERROR: unsupported dtype {dt} (need float64 or float32)')
    nz, ny, nx = shape
    m = len(values)
    if out is None:
        if not isinstance(tau, torch.Tensor):
            raise RuntimeError('ERROR: iso_depth needs out= when tau is a DeviceArray')
        out = torch.empty((m, ny, nx), dtype=tau.dtype, device=tau.device)
    for a, what, want in ((e3t, 'e3t', shape), (out, 'out', (m, ny, nx))):
        if a is not None and (tuple(int(x) for x in a.shape) != want or _np_dtype(a) != dt):
            raise RuntimeError(f'ERROR: iso_depth: {what} is {_np_dtype(a).name} {tuple(a.shape)}, need {dt.name} {want}')
    hp = None
    if thickness is not None:
        h = numpy.ascontiguousarray(thickness, dtype=numpy.float64).reshape(-1)
        if h.size != nz:
            raise RuntimeError(f'ERROR: iso_depth: thickness has {h.size} numbers, tau has {nz} levels')
        hp = _lib.dptr(h)
    v = (ctypes.c_double * m)(*values)
    check(lib.nf_iso_depth(_lib.device_pointer(out), _lib.device_pointer(tau), hp,
                           None if e3t is None else _lib.device_pointer(e3t), nz, ny, nx,
                           NF_F32 if dt == numpy.float32 else NF_F64, _marker(tau_markers[0]), _marker(tau_markers[1]),
                           _marker(e3t_markers[0]), _marker(e3t_markers[1]), top, v, m, sense, 1 if relative else 0, zref,
                           float(fill_out), stream))
    return out


def _open_source(src, fill, missing, what):
    """a (path, name) pair opened with its CF markers; anything else as it is"""
    if isinstance(src, tuple) and len(src) == 2 and isinstance(src[1], str):
        from .io import open_uvfile
        path, name = src
        src, _, d = open_uvfile(path, name, with_all=True)
        marks = list(d['_markers_' + name])
        if len(marks) > 2:
            raise RuntimeError(f'ERROR: {what} ({name}) carries {len(marks)} different _FillValue / missing_value markers '
                               f'({marks}); the engine masks at most two')
        if fill is None:
            fill = marks[0] if marks else None
        if missing is None:
            missing = marks[1] if len(marks) > 1 else None
    return src, (None if fill is None else float(fill), None if missing is None else float(missing))


class IsoDepth(object):
    """Derived depth surfaces for Field.setDepthSurfaces: the depths at which `tracer` first reaches each of `values` going
    down the column (nf_iso_depth), len(values) surfaces from one pass.  tracer: anything Field.setTracer takes -- a host
    array, a torch CUDA tensor or DeviceArray, or a (path, name) pair read one time step at a time with its CF markers -- of the
    shape (nt, nz, ny, nx) and dtype of uo / vo, or a nemoflux_amd.eos.Sigma(thetao, so, pref).  sense: +1 / 'rising' (the
    tracer rises downward, as density does) or -1 / 'falling' (as temperature does).  e3t: the cell thicknesses at T-points,
    the same kinds, static (nz, ny, nx) / (1, nz, ny, nx) or (nt, nz, ny, nx); None: the Field's own per-level thickness.
    relative=True: the values are offsets from the tracer's own value at depth zref.  fill_value / missing_value: the markers
    of the tracer (a Sigma carries its own); e3t_fill_value / e3t_missing_value: those of e3t; a file's when not given."""

    def __init__(self, tracer, values, sense, e3t=None, relative=False, zref=10.0, fill_value=None, missing_value=None,
                 e3t_fill_value=None, e3t_missing_value=None):
        self.values = _values(values, 'the values of an IsoDepth')
        self.sense = _sense(sense)
        self.relative = bool(relative)
        self.zref = _finite(zref, 'zref')
        if isinstance(tracer, Sigma):
            if fill_value is not None or missing_value is not None:
                raise RuntimeError('ERROR: a Sigma carries the markers of thetao and so itself; give them to Sigma(...)')
            self.tracer, self.markers = tracer, (None, None)
            self.shape, self.dtype = tracer.shape, tracer.dtype
        else:
            self.tracer, self.markers = _open_source(tracer, fill_value, missing_value, 'the tracer of an IsoDepth')
            self.shape, self.dtype = tuple(int(x) for x in self.tracer.shape), _np_dtype(self.tracer)
        self.e3t, self.e3t_markers = None, (None, None)
        if e3t is not None:
            self.e3t, self.e3t_markers = _open_source(e3t, e3t_fill_value, e3t_missing_value, 'the e3t of an IsoDepth')

    @property
    def m(self):
        return len(self.values)


def MixedLayerDepth(thetao, so, delta=0.03, zref=10.0, pref=0.0, e3t=None, fill_value=None, missing_value=None,
                    so_fill_value=None, so_missing_value=None, e3t_fill_value=None, e3t_missing_value=None):
    """The mixed-layer depth by the density criterion: the depth at which sigma_pref(thetao, so) first exceeds its own value
    at zref by delta kg m-3 -- IsoDepth(Sigma(thetao, so, pref), [delta], +1, relative=True, zref=zref).  delta may be a
    sequence (one surface each).  The markers are those of Sigma; e3t as in IsoDepth."""
    sigma = Sigma(thetao, so, pref, fill_value=fill_value, missing_value=missing_value, so_fill_value=so_fill_value,
                  so_missing_value=so_missing_value)
    return IsoDepth(sigma, numpy.atleast_1d(delta), +1, e3t=e3t, relative=True, zref=zref, e3t_fill_value=e3t_fill_value,
                    e3t_missing_value=e3t_missing_value)
