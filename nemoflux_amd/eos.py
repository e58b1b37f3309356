"""Potential density from potential temperature and practical salinity on the GPU (nf_sigma_eos80, csrc/nf_eos.hip): the class
field of the density-space products, computed from what NEMO writes -- thetao and so -- instead of a sigma0 the user brings.

UNESCO EOS-80 only: theta in degC referenced to the surface, practical salinity, the reference pressure in dbar (0: sigma0,
2000: sigma2, 4000: sigma4).  TEOS-10 (conservative temperature, absolute salinity) is not covered.

sigma_eos80 is the raw call on device arrays; Sigma describes the derived tracer to Field.setTracer / Field.setClassTracer, which
compute it one time step at a time into a single (nz, ny, nx) buffer -- the full series is never materialised."""
import math

import numpy

from . import _lib
from ._lib import lib, check, NF_F64, NF_F32

_NAN = float('nan')


def _pref(pref):
    p = float(pref)
    if not (p >= 0.0 and math.isfinite(p)):
        raise RuntimeError(f'ERROR: the reference pressure pref must be a finite number of dbar >= 0, got {pref!r}')
    return p


def _np_dtype(a):
    dt = a.dtype
    return dt.newbyteorder('=') if isinstance(dt, numpy.dtype) else numpy.dtype(str(dt).replace('torch.', ''))


def _marker(x):
    return _NAN if x is None else float(x)


def sigma_eos80(theta, salt, pref=0.0, out=None, theta_markers=(_NAN, _NAN), salt_markers=(_NAN, _NAN), fill_out=_NAN,
                stream=None):
    """sigma_pref(theta, S) = rho(S, T_pref, pref) - 1000 in kg m-3 (EOS-80) of two torch CUDA tensors or DeviceArrays of one
    shape and dtype (float64 or float32; the arithmetic is float64): theta in degC, S practical salinity, pref in dbar, uniform.
    theta_markers / salt_markers: the (fill, missing) pair of each input, NaN = none; NaN always counts as missing.  Where
    either input is missing the result is fill_out.  out: the array that receives the result -- a new torch tensor when both
    inputs are tensors and out is None; it may be theta or salt itself.  Asynchronous on `stream` (a HIP stream address; None:
    the null stream).  Returns out."""
    import torch
    pref = _pref(pref)
    for a in (theta, salt) + (() if out is None else (out,)):
        if not (isinstance(a, _lib.DeviceArray) or (isinstance(a, torch.Tensor) and a.is_cuda)):
            raise RuntimeError('ERROR: sigma_eos80 works on torch CUDA tensors or DeviceArrays (Sigma takes host arrays and files)')
        if isinstance(a, torch.Tensor) and not a.is_contiguous():
            raise RuntimeError('ERROR: sigma_eos80 needs contiguous tensors')
    if out is None:
        if not isinstance(theta, torch.Tensor):
            raise RuntimeError('ERROR: sigma_eos80 needs out= when the inputs are DeviceArrays')
        out = torch.empty_like(theta)
    shape, dt = tuple(int(x) for x in theta.shape), _np_dtype(theta)
    for a, what in ((salt, 'salt'), (out, 'out')):
        if tuple(int(x) for x in a.shape) != shape or _np_dtype(a) != dt:
            raise RuntimeError(f'ERROR: sigma_eos80: {what} is {_np_dtype(a).name} {tuple(a.shape)}, theta is {dt.name} {shape}')
    if dt not in (numpy.float64, numpy.float32):
        raise RuntimeError(f'ERROR: unsupported dtype {dt} (need float64 or float32)')
    n = int(numpy.prod(shape, dtype=numpy.int64)) if shape else 1
    check(lib.nf_sigma_eos80(_lib.device_pointer(out), _lib.device_pointer(theta), _lib.device_pointer(salt), n,
                             NF_F32 if dt == numpy.float32 else NF_F64, pref, _marker(theta_markers[0]),
                             _marker(theta_markers[1]), _marker(salt_markers[0]), _marker(salt_markers[1]), float(fill_out),
                             stream))
    return out


class Sigma(object):
    """The derived tracer sigma_pref(thetao, so) for Field.setTracer / Field.setClassTracer.  thetao, so: each anything setTracer
    takes -- a host array, a torch CUDA tensor or DeviceArray, or a (path, name) pair read with nemoflux_amd.io one time step at
    a time, its CF markers read from the file when not given -- of the shape and dtype of uo / vo.  fill_value / missing_value:
    the markers of thetao; so_fill_value / so_missing_value: those of so.  pref: the reference pressure in dbar."""

    def __init__(self, thetao, so, pref=0.0, fill_value=None, missing_value=None, so_fill_value=None, so_missing_value=None):
        self.pref = _pref(pref)
        given = ((fill_value, missing_value), (so_fill_value, so_missing_value))
        self.sources, self.markers = [], []
        for src, (fill, missing), what in zip((thetao, so), given, ('thetao', 'so')):
            if isinstance(src, tuple) and len(src) == 2 and isinstance(src[1], str):
                from .io import open_uvfile
                path, name = src
                src, _, d = open_uvfile(path, name, with_all=True)
                marks = list(d['_markers_' + name])
                if len(marks) > 2:
                    raise RuntimeError(f'ERROR: {what} ({name}) carries {len(marks)} different _FillValue / missing_value '
                                       f'markers ({marks}); the engine masks at most two')
                if fill is None:
                    fill = marks[0] if marks else None
                if missing is None:
                    missing = marks[1] if len(marks) > 1 else None
            self.sources.append(src)
            self.markers.append((None if fill is None else float(fill), None if missing is None else float(missing)))
        self.markers = tuple(self.markers)
        shapes = [tuple(int(x) for x in s.shape) for s in self.sources]
        if shapes[0] != shapes[1]:
            raise RuntimeError(f'ERROR: thetao and so have different shapes, {shapes[0]} and {shapes[1]}')
        dts = [_np_dtype(s) for s in self.sources]
        if dts[0] != dts[1]:
            raise RuntimeError(f'ERROR: thetao is {dts[0].name} and so {dts[1].name}: both must have the dtype of uo / vo')
        self.shape, self.dtype = shapes[0], dts[0]
