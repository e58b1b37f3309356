"""Layer thicknesses at the U and V faces derived on the GPU: the e3u / e3v of Field.setCellThickness computed from what the model
writes where grid_U / grid_V carry none -- from the thickness at T-points, e3t in grid_T or thkcello of CMIP6 (nf_face_thickness,
csrc/nf_facethick.hip), or, for z* output that holds no 3-D thickness at all, from the sea surface height and the static
mesh_mask thicknesses, e3_0 * (1 + ssh / H) with NEMO's cell-area weights when the areas are given (nf_ssh_thickness,
nf_column_depth, csrc/nf_sshthick.hip).

face_thickness / ssh_thickness / column_depth are the raw calls on device arrays; FaceThickness / SshThickness describe the
derived pair to Field.setCellThickness, which computes it one time step at a time into two (nz, ny, nx) device buffers -- the
full series is never materialised, a step that is not visited is never read.

Out of scope: e3t(t) at T-points from ssh (for an IsoDepth), the ln_vvl_ztilde / layer coordinates, whose thicknesses do not
follow from ssh, and NEMO's cell-area weights in the anomaly rule of face_thickness."""
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


# ---- z*: thicknesses from the sea surface height ---------------------------------------------------------------------------------
def _device_arrays(named, what, descriptor):
    import torch
    for a, name in named:
        if a is None:
            continue
        if not _is_device(a):
            raise RuntimeError(f'ERROR: {what} works on torch CUDA tensors or DeviceArrays; {name} is not one '
                               f'({descriptor} takes host arrays and files)')
        if isinstance(a, torch.Tensor) and not a.is_contiguous():
            raise RuntimeError(f'ERROR: {what} needs contiguous tensors; {name} is not')


def _shape(a):
    return tuple(int(x) for x in a.shape)


def column_depth(e3_0, markers=(_NAN, _NAN), out=None, stream=None):
    """The sum of a static thickness down every column (nf_column_depth; the definition is in include/nemoflux_amd.h): hu_0 /
    hv_0 of e3u_0 / e3v_0, the H of ssh_thickness.  e3_0: a torch CUDA tensor or DeviceArray of shape (nz, ny, nx), float64 or
    float32; the levels are added in ascending order in float64, a level that is NaN or one of `markers` (the (fill, missing)
    pair, NaN = none) is left out.  out: the float64 (ny, nx) device array that receives the result -- a new torch tensor when
    e3_0 is a tensor and out is None.  Asynchronous on `stream` (a HIP stream address; None: the null stream).  Returns out."""
    import torch
    _device_arrays(((e3_0, 'e3_0'), (out, 'out')), 'column_depth', 'SshThickness')
    shape, dt = _shape(e3_0), _np_dtype(e3_0)
    if len(shape) != 3 or min(shape) < 1:
        raise RuntimeError(f'ERROR: column_depth: e3_0 has shape {shape}; need (nz, ny, nx), each >= 1')
    if dt not in (numpy.float64, numpy.float32):
        raise RuntimeError(f'ERROR: unsupported dtype {dt} (need float64 or float32)')
    nz, ny, nx = shape
    if out is None:
        if not isinstance(e3_0, torch.Tensor):
            raise RuntimeError('ERROR: column_depth needs out= when e3_0 is a DeviceArray')
        out = torch.empty((ny, nx), dtype=torch.float64, device=e3_0.device)
    if _shape(out) != (ny, nx) or _np_dtype(out) != numpy.float64:
        raise RuntimeError(f'ERROR: column_depth: out is {_np_dtype(out).name} {_shape(out)}, need float64 {(ny, nx)}')
    check(lib.nf_column_depth(_lib.device_pointer(out), _lib.device_pointer(e3_0), nz, ny, nx,
                              NF_F32 if dt == numpy.float32 else NF_F64, _marker(markers[0]), _marker(markers[1]), stream))
    return out


def _areas(areas, what):
    if areas is None:
        return (None, None, None)
    if not isinstance(areas, (tuple, list)) or len(areas) != 3 or any(a is None for a in areas):
        raise RuntimeError(f'ERROR: {what}: areas must be None or the triple (e1e2t, e1e2u, e1e2v)')
    return tuple(areas)


def ssh_thickness(ssh, e3u0, e3v0, hu0=None, hv0=None, areas=None, wrapX=True, markers=(_NAN, _NAN),
                  static_markers=(_NAN, _NAN), out=None, stream=None):
    """(e3u, e3v), the z* layer thicknesses at the east and north faces of one time step of the sea surface height:
    e3u0 * (1 + ssh_u / hu0) (nf_ssh_thickness; the definition is in include/nemoflux_amd.h).  ssh: a torch CUDA tensor or
    DeviceArray of shape (ny, nx), float64 or float32 (the arithmetic is float64).  e3u0 / e3v0: the static thicknesses at the U
    and V points, device arrays of shape (nz, ny, nx) typed like ssh.  hu0 / hv0: the column depths at the U and V points,
    float64 (ny, nx) device arrays; None: column_depth of e3u0 / e3v0.  areas: None -- ssh at a face is the mean of the two
    cells -- or the triple (e1e2t, e1e2u, e1e2v) of float64 (ny, nx) device arrays: NEMO's area-weighted mean.  wrapX: the east
    face of the last column takes the first column as its neighbour.  markers / static_markers: the (fill, missing) pair of
    ssh / of the statics, NaN = none; NaN always counts as missing.  A face beside a cell without ssh keeps its static
    thickness.  out: the pair of arrays that receives the result -- two new torch tensors when e3u0 is a tensor and out is
    None.  Asynchronous on `stream` (a HIP stream address; None: the null stream); complete at return when hu0 / hv0 are
    computed here.  Returns out."""
    import torch
    if out is not None and (not isinstance(out, (tuple, list)) or len(out) != 2):
        raise RuntimeError('ERROR: ssh_thickness: out must be the pair (e3u, e3v)')
    if (hu0 is None) != (hv0 is None):
        raise RuntimeError('ERROR: ssh_thickness: hu0 and hv0 go together: both or neither')
    at, au, av = _areas(areas, 'ssh_thickness')
    outs = (None, None) if out is None else tuple(out)
    planes = ((hu0, 'hu0'), (hv0, 'hv0'), (at, 'areas[0]'), (au, 'areas[1]'), (av, 'areas[2]'))
    named = ((ssh, 'ssh'), (e3u0, 'e3u0'), (e3v0, 'e3v0')) + planes + ((outs[0], 'out[0]'), (outs[1], 'out[1]'))
    for a, what in named[:3]:
        if a is None:
            raise RuntimeError(f'ERROR: ssh_thickness needs {what}')
    _device_arrays(named, 'ssh_thickness', 'SshThickness')
    shape, dt = _shape(e3u0), _np_dtype(e3u0)
    if len(shape) != 3 or min(shape) < 1:
        raise RuntimeError(f'ERROR: ssh_thickness: e3u0 has shape {shape}; need (nz, ny, nx), each >= 1')
    if dt not in (numpy.float64, numpy.float32):
        raise RuntimeError(f'ERROR: unsupported dtype {dt} (need float64 or float32)')
    nz, ny, nx = shape
    if out is None:
        if not isinstance(e3u0, torch.Tensor):
            raise RuntimeError('ERROR: ssh_thickness needs out= when e3u0 is a DeviceArray')
        outs = (torch.empty_like(e3u0), torch.empty_like(e3u0))
    for a, what in ((e3v0, 'e3v0'), (outs[0], 'out[0]'), (outs[1], 'out[1]')):
        if _shape(a) != shape or _np_dtype(a) != dt:
            raise RuntimeError(f'ERROR: ssh_thickness: {what} is {_np_dtype(a).name} {_shape(a)}, need {dt.name} {shape}')
    if _shape(ssh) != (ny, nx) or _np_dtype(ssh) != dt:
        raise RuntimeError(f'ERROR: ssh_thickness: ssh is {_np_dtype(ssh).name} {_shape(ssh)}, need {dt.name} {(ny, nx)}')
    for a, what in planes:
        if a is not None and (_shape(a) != (ny, nx) or _np_dtype(a) != numpy.float64):
            raise RuntimeError(f'ERROR: ssh_thickness: {what} is {_np_dtype(a).name} {_shape(a)}, need float64 {(ny, nx)}')
    computed = hu0 is None
    if computed:
        if not isinstance(e3u0, torch.Tensor):
            raise RuntimeError('ERROR: ssh_thickness needs hu0= and hv0= when e3u0 is a DeviceArray')
        hu0 = column_depth(e3u0, static_markers, stream=stream)
        hv0 = column_depth(e3v0, static_markers, stream=stream)
    check(lib.nf_ssh_thickness(_lib.device_pointer(outs[0]), _lib.device_pointer(outs[1]), _lib.device_pointer(ssh),
                               _lib.device_pointer(e3u0), _lib.device_pointer(e3v0), _lib.device_pointer(hu0),
                               _lib.device_pointer(hv0), *[None if a is None else _lib.device_pointer(a) for a in (at, au, av)],
                               nz, ny, nx, NF_F32 if dt == numpy.float32 else NF_F64, 1 if wrapX else 0, _marker(markers[0]),
                               _marker(markers[1]), _marker(static_markers[0]), _marker(static_markers[1]), stream))
    if computed:
        check(lib.nf_synchronize())     # the column depths computed here are released at return
    return outs


class SshThickness(object):
    """The derived cell thickness for Field.setCellThickness(SshThickness(...)) of z* output (ln_vvl_zstar, key_qco,
    key_linssh), which holds the 2-D sea surface height and a static mesh_mask and no 3-D thickness: e3u = e3u0 * (1 + ssh_u /
    hu0) and e3v likewise (nf_ssh_thickness).  ssh: anything Field.setDepthSurfaces takes for one surface -- a host array, a
    torch CUDA tensor or DeviceArray, or a (path, name) pair read whole with its CF markers (a packed one decoded) -- of the dtype of
    uo / vo, static (ny, nx) / (1, ny, nx) or (nt, ny, nx).  The statics: either e3u0 and e3v0 (e3u_0, e3v_0 of a mesh_mask),
    or e3t0 alone, from which the two are derived once on the device by nf_face_thickness with rule 'min', NEMO's own
    partial-step rule for e3u_0; static arrays of the kinds FaceThickness takes or (path, name) pairs.  hu0 / hv0: the column
    depths at the U and V points, (ny, nx) arrays such as a mesh file's, or (path, name) pairs; None: nf_column_depth of the
    face statics.  areas: None, or the triple (e1e2t, e1e2u, e1e2v) of (ny, nx) arrays or (path, name) pairs -- NEMO's
    area-weighted ssh at the faces.  wrapX: the east face of the last column takes the first column as its neighbour.
    fill_value / missing_value: the markers of ssh; static_fill_value / static_missing_value: those of the statics; a file's
    when not given."""

    def __init__(self, ssh, e3u0=None, e3v0=None, e3t0=None, hu0=None, hv0=None, areas=None, wrapX=True, fill_value=None,
                 missing_value=None, static_fill_value=None, static_missing_value=None):
        if e3t0 is not None and (e3u0 is not None or e3v0 is not None):
            raise RuntimeError('ERROR: SshThickness: give either e3u0 and e3v0, or e3t0 alone (e3u0 and e3v0 are then derived '
                               'from it), not both')
        if e3t0 is None and (e3u0 is None or e3v0 is None):
            raise RuntimeError('ERROR: SshThickness needs the static thicknesses: e3u0 and e3v0, or e3t0 alone')
        if (hu0 is None) != (hv0 is None):
            raise RuntimeError('ERROR: SshThickness: hu0 and hv0 go together: both or neither')
        areas = _areas(areas, 'SshThickness')
        self.wrapX = bool(wrapX)
        self.ssh, self.markers = _open_source(ssh, fill_value, missing_value, 'the ssh of an SshThickness')
        self.ssh = _decoded(self.ssh)
        self.shape, self.dtype = _shape(self.ssh), _np_dtype(self.ssh)
        self.from_e3t0 = e3t0 is not None
        self.statics, marks = [], []
        for src, what in ((e3t0, 'e3t0'),) if self.from_e3t0 else ((e3u0, 'e3u0'), (e3v0, 'e3v0')):
            src, m = _open_source(src, None, None, f'the {what} of an SshThickness')
            self.statics.append(src)
            for x in m:
                if x is not None and x not in marks:
                    marks.append(x)
        if len(marks) > 2:
            raise RuntimeError(f'ERROR: e3u0 / e3v0 carry {len(marks)} different _FillValue / missing_value markers '
                               f'({marks}); the engine masks at most two')
        if static_fill_value is None:
            static_fill_value = marks[0] if marks else None
        if static_missing_value is None:
            static_missing_value = marks[1] if len(marks) > 1 else None
        self.static_markers = (None if static_fill_value is None else float(static_fill_value),
                               None if static_missing_value is None else float(static_missing_value))
        # the float64 planes: a masked value of a file arrives as NaN, which the definition takes as "not there"
        self.depths = None if hu0 is None else tuple(_plane_source(a, w) for a, w in ((hu0, 'hu0'), (hv0, 'hv0')))
        self.areas = None if areas[0] is None else tuple(_plane_source(a, f'areas[{k}]') for k, a in enumerate(areas))


def _decoded(src):
    """a file variable of fewer than four dimensions (ssh, a plane) as a host array: the readers hand such a variable over
    whole -- only (nt, nz, ny, nx) variables are read one time step at a time -- and a packed one (io.CFDecodedVariable)
    decodes whole whatever step is asked for, its masked values NaN"""
    if hasattr(src, 'read_step') and len(src.shape) < 4:
        return src.read_step(0)
    return src


def _plane_source(src, what):
    """a float64 (ny, nx) plane of an SshThickness: a device array as it is, anything else read now with its markers as NaN"""
    if _is_device(src):
        return src
    src, marks = _open_source(src, None, None, f'the {what} of an SshThickness')
    a = numpy.array(_decoded(src), dtype=numpy.float64)
    for m in marks:
        if m is not None:
            a[a == m] = numpy.nan
    return a
