"""Layer thicknesses at the U and V faces derived on the GPU from the thickness at T-points (nf_face_thickness,
csrc/nf_facethick.hip): the e3u / e3v of Field.setCellThickness computed from what the model writes -- e3t in grid_T, thkcello of
CMIP6 -- where grid_U / grid_V carry none.

face_thickness is the raw call on device arrays; FaceThickness describes the derived pair to Field.setCellThickness, which
computes it one time step at a time into two (nz, ny, nx) device buffers -- the full series is never materialised, a step that
is not visited is never read.

Out of scope: thicknesses from ssh alone (e3_0 * (1 + ssh / H)), and NEMO's cell-area weights in the anomaly rule."""
import numpy

from . import _lib
from ._lib import lib, check, NF_F64, NF_F32
from .eos import _np_dtype, _marker
from .surfaces import _is_device, _open_source

_NAN = float('nan')
RULES = {'min': _lib.NF_E3_MIN, 'mean': _lib.NF_E3_MEAN, 'anomaly': _lib.NF_E3_ANOMALY}


def _rule(rule):
    if rule not in RULES:
        raise RuntimeError(f"ERROR: rule must be 'min' (partial steps: the thinner of the two cells), 'mean' or 'anomaly' "
                           f"(z*: the static face thickness plus the mean anomaly of the two cells), got {rule!r}")
    return RULES[rule]


def _statics(rule, e3t0, e3u0, e3v0, what):
    given = [x is not None for x in (e3t0, e3u0, e3v0)]
    if rule == 'anomaly' and not all(given):
        raise RuntimeError(f"ERROR: {what}: rule 'anomaly' needs the static thicknesses e3t0, e3u0 and e3v0")
    if rule != 'anomaly' and any(given):
        raise RuntimeError(f"ERROR: {what}: e3t0, e3u0 and e3v0 go with rule 'anomaly' only")


def face_thickness(e3t, rule='min', e3t0=None, e3u0=None, e3v0=None, wrapX=True, markers=(_NAN, _NAN),
                   static_markers=(_NAN, _NAN), out=None, stream=None):
    """(e3u, e3v), the layer thicknesses at the east and north faces of one time step of the T-grid thickness e3t
    (nf_face_thickness; the definition is in include/nemoflux_amd.h).  e3t: a torch CUDA tensor or DeviceArray of shape
    (nz, ny, nx), float64 or float32 (the arithmetic is float64).  rule: 'min', the thinner of the two cells (partial steps);
    'mean'; or 'anomaly', e3u0 + the mean of the two cells' e3t - e3t0 (z*), which needs the static e3t0, e3u0, e3v0, device
    arrays shaped and typed like e3t.  wrapX: the east face of the last column takes the first column as its neighbour.
    markers / static_markers: the (fill, missing) pair of e3t / of the statics, NaN = none; NaN always counts as missing.  A
    face beside a cell without a thickness gets 0 (the static face thickness under 'anomaly').  out: the pair of arrays that
    receives the result -- two new torch tensors when e3t is a tensor and out is None.  Asynchronous on `stream` (a HIP stream
    address; None: the null stream).  Returns out."""
    import torch
    code = _rule(rule)
    _statics(rule, e3t0, e3u0, e3v0, 'face_thickness')
    if out is not None and (not isinstance(out, (tuple, list)) or len(out) != 2):
        raise RuntimeError('ERROR: face_thickness: out must be the pair (e3u, e3v)')
    outs = (None, None) if out is None else tuple(out)
    named = ((e3t, 'e3t'), (e3t0, 'e3t0'), (e3u0, 'e3u0'), (e3v0, 'e3v0'), (outs[0], 'out[0]'), (outs[1], 'out[1]'))
    for a, what in named:
        if a is None:
            continue
        if not _is_device(a):
            raise RuntimeError(f'ERROR: face_thickness works on torch CUDA tensors or DeviceArrays; {what} is not one '
                               f'(FaceThickness takes host arrays and files)')
        if isinstance(a, torch.Tensor) and not a.is_contiguous():
            raise RuntimeError(f'ERROR: face_thickness needs contiguous tensors; {what} is not')
    shape, dt = tuple(int(x) for x in e3t.shape), _np_dtype(e3t)
    if len(shape) != 3 or min(shape) < 1:
        raise RuntimeError(f'ERROR: face_thickness: e3t has shape {shape}; need (nz, ny, nx), each >= 1')
    if dt not in (numpy.float64, numpy.float32):
        raise RuntimeError(f'ERROR: unsupported dtype {dt} (need float64 or float32)')
    if out is None:
        if not isinstance(e3t, torch.Tensor):
            raise RuntimeError('ERROR: face_thickness needs out= when e3t is a DeviceArray')
        outs = (torch.empty_like(e3t), torch.empty_like(e3t))
    for a, what in named[1:4] + ((outs[0], 'out[0]'), (outs[1], 'out[1]')):
        if a is not None and (tuple(int(x) for x in a.shape) != shape or _np_dtype(a) != dt):
            raise RuntimeError(f'ERROR: face_thickness: {what} is {_np_dtype(a).name} {tuple(a.shape)}, need {dt.name} {shape}')
    nz, ny, nx = shape
    check(lib.nf_face_thickness(_lib.device_pointer(outs[0]), _lib.device_pointer(outs[1]), _lib.device_pointer(e3t),
                                *[None if a is None else _lib.device_pointer(a) for a in (e3t0, e3u0, e3v0)], nz, ny, nx,
                                NF_F32 if dt == numpy.float32 else NF_F64, code, 1 if wrapX else 0, _marker(markers[0]),
                                _marker(markers[1]), _marker(static_markers[0]), _marker(static_markers[1]), stream))
    return outs


class FaceThickness(object):
    """The derived cell thickness for Field.setCellThickness(FaceThickness(...)): e3u and e3v computed from the thickness at
    T-points (nf_face_thickness).  e3t: anything Field.setTracer takes -- a host array, a torch CUDA tensor or DeviceArray, or a
    (path, name) pair read one time step at a time with its CF markers -- of the dtype of uo / vo, static (nz, ny, nx) /
    (1, nz, ny, nx) or (nt, nz, ny, nx).  rule: 'min' (partial steps), 'mean' or 'anomaly' (z*; needs e3t0, e3u0, e3v0).  The
    statics are static arrays of the same kinds or (path, name) pairs; a static host array of another float dtype is cast to
    the dtype of uo / vo, any other dtype mismatch raises.  wrapX: the east face of the last column takes the first column as
    its neighbour.  fill_value / missing_value: the markers of e3t; static_fill_value / static_missing_value: those of the
    three statics; a file's when not given."""

    def __init__(self, e3t, rule='min', e3t0=None, e3u0=None, e3v0=None, wrapX=True, fill_value=None, missing_value=None,
                 static_fill_value=None, static_missing_value=None):
        self.code = _rule(rule)
        self.rule = rule
        _statics(rule, e3t0, e3u0, e3v0, 'FaceThickness')
        self.wrapX = bool(wrapX)
        self.e3t, self.markers = _open_source(e3t, fill_value, missing_value, 'the e3t of a FaceThickness')
        self.shape, self.dtype = tuple(int(x) for x in self.e3t.shape), _np_dtype(self.e3t)
        self.statics, marks = [], []
        for src, what in ((e3t0, 'e3t0'), (e3u0, 'e3u0'), (e3v0, 'e3v0')):
            if src is None:
                continue
            src, m = _open_source(src, None, None, f'the {what} of a FaceThickness')
            self.statics.append(src)
            for x in m:
                if x is not None and x not in marks:
                    marks.append(x)
        if len(marks) > 2:
            raise RuntimeError(f'ERROR: e3t0 / e3u0 / e3v0 carry {len(marks)} different _FillValue / missing_value markers '
                               f'({marks}); the engine masks at most two')
        if static_fill_value is None:
            static_fill_value = marks[0] if marks else None
        if static_missing_value is None:
            static_missing_value = marks[1] if len(marks) > 1 else None
        self.static_markers = (None if static_fill_value is None else float(static_fill_value),
                               None if static_missing_value is None else float(static_missing_value))
