"""Field: the flux engine, same surface as nemoflux/field.py:15-234, running on the gfx950 kernels.

What fluxviz.py / fluxplot.py read stays available under the same names: timeIndex, nt, nz,
ny, nx, dx, lonmin..latmax, sverdrup, maxAbsFlux, lonlat, edgeFluxesUArray, edgeFluxesVArray,
integratedVelocity, vectorPoints, vectorValues, plis, timeObj, gr, thickness, arcLengths; update(),
getFluxText(); plus computeFlux(tIndex) / computeAll() (BASELINE.json north_star).  The host arrays that
VTK aliases (fluxviz.py:148,160,168) are written IN PLACE at every update().
"""
import ctypes
import re

import numpy

from . import _lib, mint
from ._lib import lib, check, NF_F64, NF_F32
from ._sources import Layout, SigmaProducer, ThicknessProducer, IsoDepthProducer, _native, _nan_if_none
from .horizgrid import HorizGrid
from .io import open_tfile, open_uvfile
from .timeobj import TimeObj

EARTH_RADIUS = 6371000.0  # field.py:12


def _dtype_code(a):
    import torch
    dt = a.dtype
    if isinstance(dt, numpy.dtype):
        dt = dt.type
    if dt in (numpy.float64, torch.float64):
        return NF_F64
    if dt in (numpy.float32, torch.float32):
        return NF_F32
    raise RuntimeError(f'ERROR: unsupported dtype {dt} (need float64 or float32)')


def _native_dtype(a):
    """numpy dtype, in native byte order, of a host array, a file variable, a DeviceArray or a torch tensor"""
    dt = a.dtype
    if isinstance(dt, numpy.dtype):
        return dt.newbyteorder('=')
    return numpy.dtype(str(dt).replace('torch.', ''))


def _open_pair(a):
    """(variable, its CF markers) of a (path, name) pair, opened with nemoflux_amd.io; anything else as it is, with none"""
    if isinstance(a, tuple) and len(a) == 2 and isinstance(a[1], str):
        var, _, d = open_uvfile(a[0], a[1], with_all=True)
        return var, list(d['_markers_' + a[1]])
    return a, []


def _two_markers(markers, fill_value, missing_value, subject, merge=False):
    """The engine's (fill, missing), NaN for none, from the markers the files carry and the caller's fill_value / missing_value,
    which come first; more than two file markers raise in the words of `subject`.  merge: the caller's count among them."""
    for m in (fill_value, missing_value) if merge else ():
        if m is not None and float(m) == float(m) and float(m) not in markers:
            markers.append(float(m))
    if len(markers) > 2:
        raise RuntimeError(f'ERROR: {subject} {len(markers)} different _FillValue / missing_value markers '
                           f'({markers}); the engine masks at most two')
    if fill_value is None:
        fill_value = markers[0] if markers else None
    if missing_value is None:
        missing_value = markers[1] if len(markers) > 1 else None
    return tuple(float(m) for m in _nan_if_none((fill_value, missing_value)))


def _geometry_only(bounds_lon, bounds_lat):
    """Run the geometry kernel alone: {'points': (ncell,4,3), 'arcLengths': (ncell,4), 'box': 4 floats}."""
    h = ctypes.c_void_p()
    check(lib.nf_field_new(ctypes.byref(h)))
    try:
        blon = _native(bounds_lon)
        blat = _native(bounds_lat)
        if blon.dtype != blat.dtype:
            blat = blat.astype(blon.dtype)
        ny, nx, _ = blon.shape
        check(lib.nf_field_set_bounds(ctypes.byref(h), blon.ctypes.data, blat.ctypes.data, ny, nx, _dtype_code(blon), 0))
        pts = numpy.empty((ny * nx, 4, 3), numpy.float64)
        arc = numpy.empty((ny * nx, 4), numpy.float64)
        check(lib.nf_field_get_points(ctypes.byref(h), _lib.dptr(pts)))
        check(lib.nf_field_get_arclengths(ctypes.byref(h), _lib.dptr(arc)))
        b = [ctypes.c_double() for _ in range(4)]
        check(lib.nf_field_get_box(ctypes.byref(h), *[ctypes.byref(x) for x in b]))
        return dict(points=pts, arcLengths=arc, box=[x.value for x in b])
    finally:
        lib.nf_field_del(ctypes.byref(h))


def _band_sum(P, bounds_depth, ztop, zbot):
    """sum_z P[z] * overlap([ztop, zbot], layer z) / thickness[z], in level order; layers outside the band or of zero
    thickness are skipped, a layer inside it whole enters with the factor 1 (so the band of whole layers is the plain sum)."""
    b = numpy.asarray(bounds_depth, dtype=numpy.float64)
    acc = numpy.zeros(P.shape[1:], numpy.float64)
    for z in range(P.shape[0]):
        lo, hi = min(b[z, 0], b[z, 1]), max(b[z, 0], b[z, 1])
        th = hi - lo
        ov = min(zbot, hi) - max(ztop, lo)
        if not (th > 0.0 and ov > 0.0):
            continue
        acc = acc + (P[z] if ov >= th else P[z] * (ov / th))
    return acc


def _arc_length(lon0, lat0, lon1, lat1):
    """great-circle distance on the unit sphere between points given in degrees: the units of Field.arcLengths (the angle
    between the two position vectors, as the cell edges' lengths are formed)"""
    d = numpy.pi / 180.
    lo0, la0, lo1, la1 = (numpy.asarray(x, dtype=numpy.float64) * d for x in (lon0, lat0, lon1, lat1))
    dot = numpy.cos(la0) * numpy.cos(la1) * numpy.cos(lo1 - lo0) + numpy.sin(la0) * numpy.sin(la1)
    return numpy.fabs(numpy.arccos(numpy.clip(dot, -1., 1.)))


class Crossings(object):
    """The crossings of a Field's transects (Field.getCrossings), in record order: one per (target segment, crossed cell), by
    segment and then along the segment.  Arrays of length ncross unless said otherwise:
    segment (global id), transect, offsets (ntransect + 1: the crossings of transect p are offsets[p]:offsets[p + 1]), cell,
    j, i, ta, tb (the piece's parameters on its own target segment), lon0, lat0, lon1, lat1 (the piece's ends: the segment's end
    points interpolated linearly in the planar lon-lat space the weights are built in), s0, s1 (distance along the transect
    to the piece's ends, in the units of arcLengths: the great-circle length of the earlier segments plus the fraction ta / tb
    of this one's)."""
    _names = ('segment', 'transect', 'offsets', 'cell', 'j', 'i', 'ta', 'tb', 'lon0', 'lat0', 'lon1', 'lat1', 's0', 's1')

    def __init__(self, **kw):
        for n in self._names:
            setattr(self, n, kw[n])

    def __len__(self):
        return int(self.segment.size)

    def asdict(self):
        return {n: getattr(self, n) for n in self._names}


class _TimeObj(object):
    """timeobj.TimeObj stand-in that tolerates a missing time axis."""

    def __init__(self, timeValues=None):
        self.timeVarName = 'time_counter' if timeValues is not None else ''
        self.timeValues = timeValues

    def getSize(self):
        return 0 if self.timeValues is None else len(self.timeValues)

    def getValues(self):
        return self.timeValues

    def getTimeAsDate(self, timeIndex):
        return timeIndex if self.timeValues is None else self.timeValues[timeIndex]

    def getTimeAsString(self, timeIndex):
        return f'{timeIndex}' if self.timeValues is None else f'{self.timeValues[timeIndex]}'


class _PinnedBlock(object):
    """Owner of one pinned host allocation; freed when the last numpy view of it is gone (VTK may outlive the Field)."""

    def __init__(self, nbytes):
        p = ctypes.c_void_p()
        check(lib.nf_host_alloc(ctypes.byref(p), max(int(nbytes), 8)))
        self.ptr = p.value

    def __del__(self):
        try:
            if self.ptr:
                lib.nf_host_free(self.ptr)
                self.ptr = None
        except Exception:
            pass


class _DerivedPlane(object):
    """plane `index` of a derived item (a nemoflux_amd.surfaces.IsoDepth) in the item list of setDepthSurfaces"""

    def __init__(self, item, index):
        self.item, self.index = item, index


class _DerivedThickness(object):
    """e3u (which = 0) or e3v (1) of a time-varying derived cell thickness (nemoflux_amd.thickness.FaceThickness) as a series
    of the time-mean walks: it lives nowhere, step t is computed straight into a device address."""

    def __init__(self, slot, producer, which, shape, dtype):
        self.slot, self.producer, self.which, self.shape, self.dtype = slot, producer, which, shape, numpy.dtype(dtype)

    def compute_step(self, tIndex, dst_ptr):
        """step tIndex of this face thickness at the HBM address dst_ptr; the other one goes to the slot's own buffer, which
        no longer holds the step the engine was given.  Complete at return."""
        self.slot['step'] = -1
        ptrs = [b.ptr for b in self.producer.out]
        ptrs[self.which] = dst_ptr
        self.producer.run(tIndex, *ptrs)
        check(lib.nf_synchronize())


class _Transect(object):
    """Entry of Field.plis: quacks like mint.PolylineIntegral.getIntegral (fluxplot.py:56).

    When asked about the Field's own integratedVelocity it returns the value the batched on-device
    reduction produced for the current step; any other data goes through a real PolylineIntegral."""

    def __init__(self, field, index, xyz):
        self._field, self._index, self._xyz = field, index, xyz
        self._pli = None

    def getIntegral(self, data, placement=mint.CELL_BY_CELL_DATA):
        f = self._field
        if data is f.integratedVelocity and f._row_valid:
            return float(f._row[f._nseg + self._index])
        if self._pli is None:
            self._pli = mint.PolylineIntegral()
            self._pli.setGrid(f.gr.getMintGrid())
            self._pli.buildLocator(numCellsPerBucket=128, periodX=f.periodX, enableFolding=False)
            self._pli.computeWeights(self._xyz, counterclock=False)
        return self._pli.getIntegral(data, placement)

    def getSegmentIntegrals(self):
        f = self._field
        o = f._tr_off
        return numpy.array(f._row[o[self._index]:o[self._index + 1]])


class Field(object):

    def __init__(self, tFile, uFile, vFile, lonLatZPoints, sverdrup=False, **kw):
        """Same positional signature as the reference (field.py:17).  tFile/uFile/vFile: NetCDF-4 files (read by
        nemoflux_amd.io / hdf5min; compressed uo/vo one time step at a time) or the .npz bundles of
        nemoflux_amd.datagen / subsetnemo; see fromArrays for in-memory / HBM data and _setup for the keywords
        (fill_value, periodX, slab_range, readback, compact, stream, unsupportedCells, overlappingCells, ...)."""
        t = open_tfile(tFile)
        if 'deptht_bounds' not in t:
            raise RuntimeError(f'ERROR: {tFile} has no variable deptht_bounds')
        uo, _, uvars = open_uvfile(uFile, 'uo', with_all=True)
        vo, _, vvars = open_uvfile(vFile, 'vo', with_all=True)
        # values that mean 'missing' (xarray's decode_cf masks _FillValue and missing_value, field.py:34-35, 157): the engine
        # compares every value of uo and vo with up to two markers
        markers = list(uvars['_markers_uo'])
        for m in vvars['_markers_vo']:
            if m not in markers:
                markers.append(m)
        if 'fill_value' in kw:
            markers = [float(kw.pop('fill_value'))] + [m for m in markers[1:2]]
        if len(markers) > 2:
            raise RuntimeError(f'ERROR: uo / vo carry {len(markers)} different _FillValue / missing_value markers '
                               f'({markers}); the engine masks at most two')
        kw.setdefault('timeObj', TimeObj.fromVariables(uvars))   # field.py:38: TimeObj(self.ncU)
        # The reference's constructor never raises over a target line that meets a distorted polar cell (field.py:44-49: mint's
        # computeWeights has no error path), so the drop-in signature leaves such cells out and warns (coverage + the number
        # of crossings dropped); Field.fromArrays -- the batch constructor of bench.py / fluxplot-style drivers -- refuses.
        kw.setdefault('unsupportedCells', 'skip')
        self._setup(t['bounds_lon'], t['bounds_lat'], t['deptht_bounds'], uo, vo, lonLatZPoints, sverdrup,
                    fill_value=markers[0] if markers else numpy.nan,
                    missing_value=markers[1] if len(markers) > 1 else numpy.nan, **kw)

    @classmethod
    def fromArrays(cls, bounds_lon, bounds_lat, deptht_bounds, uo, vo, lonLatZPoints, sverdrup=False, **kw):
        """bounds_*: (ny,nx,4) host arrays (f64/f32) or torch CUDA tensors; uo/vo: (nt,nz,ny,nx) [or (nz,ny,nx)]
        host arrays, torch CUDA tensors or DeviceArray (HBM-resident, used in place)."""
        self = cls.__new__(cls)
        self._setup(bounds_lon, bounds_lat, deptht_bounds, uo, vo, lonLatZPoints, sverdrup, **kw)
        return self

    # ------------------------------------------------------------------------------------------
    def _setup(self, bounds_lon, bounds_lat, deptht_bounds, uo, vo, lonLatZPoints, sverdrup,
               fill_value=numpy.nan, missing_value=numpy.nan, periodX=360., numCellsPerBucket=128, slab_range=None,
               readback=True,
               timeValues=None, stream=None, timeObj=None, compact=False, prefetch=True, gpu_decode=True,
               unsupportedCells='refuse', overlappingCells='refuse'):
        _lib.require_gpu()
        self.sverdrup = sverdrup
        self.periodX = periodX
        self._readback = readback
        self._stream = stream
        # what timeMean needs to build the Field of the mean state the way this one was built
        self._uv_markers = (float(fill_value), float(missing_value))
        self._build_kw = dict(periodX=periodX, numCellsPerBucket=numCellsPerBucket, readback=readback, compact=compact,
                              unsupportedCells=unsupportedCells, overlappingCells=overlappingCells)
        self._h = ctypes.c_void_p()
        check(lib.nf_field_new(ctypes.byref(self._h)))
        if stream is not None:
            check(lib.nf_field_set_stream(ctypes.byref(self._h), ctypes.c_void_p(stream)))
        self._keep = [bounds_lon, bounds_lat, uo, vo]  # borrowed buffers must outlive the handle

        # --- cell bounds -> geometry kernel (field.py:22-31, 42, 56)
        plon, plat = _lib.device_pointer(bounds_lon), _lib.device_pointer(bounds_lat)
        if plon is None:
            bounds_lon = _native(bounds_lon)
            bounds_lat = _native(bounds_lat)
            if bounds_lat.dtype != bounds_lon.dtype:
                bounds_lat = bounds_lat.astype(bounds_lon.dtype)
            self._keep += [bounds_lon, bounds_lat]
            plon, plat, on_dev = bounds_lon.ctypes.data, bounds_lat.ctypes.data, 0
        else:
            on_dev = 1
        if len(bounds_lon.shape) != 3 or bounds_lon.shape[2] != 4 or tuple(bounds_lon.shape) != tuple(bounds_lat.shape):
            raise RuntimeError('ERROR: bounds_lat/bounds_lon must have shape (ny, nx, 4)')
        self._bounds = (bounds_lon, bounds_lat)
        ny, nx = int(bounds_lon.shape[0]), int(bounds_lon.shape[1])
        check(lib.nf_field_set_bounds(ctypes.byref(self._h), plon, plat, ny, nx, _dtype_code(bounds_lon), on_dev))
        b = [ctypes.c_double() for _ in range(4)]
        check(lib.nf_field_get_box(ctypes.byref(self._h), *[ctypes.byref(x) for x in b]))
        self.lonmin, self.lonmax, self.latmin, self.latmax = [x.value for x in b]
        print(f'lon-lat box: {self.lonmin}, {self.latmin} -> {self.lonmax}, {self.latmax}')  # field.py:31

        self.timeIndex = 0
        self.timeObj = timeObj if timeObj is not None else _TimeObj(timeValues)

        # --- uo / vo (field.py:34-35, 122-136)
        self.nt, self.nz, sy, sx = self.getSizes(tuple(uo.shape))
        if (sy, sx) != (ny, nx) or tuple(vo.shape) != tuple(uo.shape):
            raise RuntimeError("ERROR: uo/vo shapes do not match the (ny, nx) of the cell bounds")
        self.ny, self.nx = ny, nx
        pu, pv = _lib.device_pointer(uo), _lib.device_pointer(vo)
        self._lazy = None
        if hasattr(uo, 'read_step') or hasattr(vo, 'read_step'):
            # file-backed variables inflated one time step at a time (nemoflux_amd.hdf5min.LazyVariable)
            self._lazy = (uo, vo)
            self._lazy_dtype = numpy.dtype(uo.dtype).newbyteorder('=')
            self._uv_code, self._fill = _dtype_code(uo), float(fill_value)
            self._lazy_step = -1
            # two slots of staging buffers: while the GPU works on the steps of one, a background host thread prepares the
            # next ones in the other; deflated HDF5 chunks are inflated on the device (nemoflux_amd.staging / ingest)
            from .staging import StepStager
            self._stager = StepStager((uo, vo), self.nt, self.nz, ny, nx, self._lazy_dtype, self._host_array,
                                      prefetch=prefetch, gpu_decode=gpu_decode)
            pu = pv = None
            uv_dev = 0
        elif pu is None:
            uo = _native(uo)
            vo = _native(vo)
            if vo.dtype != uo.dtype:
                vo = vo.astype(uo.dtype)
            self._keep += [uo, vo]
            pu, pv, uv_dev = uo.ctypes.data, vo.ctypes.data, 0
        else:
            uv_dev = 1
        self._uv = (uo, vo)
        if self._lazy is None:
            self._uv_code = _dtype_code(uo)
            check(lib.nf_field_set_uv(ctypes.byref(self._h), pu, pv, self.nt, self._uv_code, uv_dev, float(fill_value)))
        if missing_value == missing_value:   # a second marker (CF missing_value that differs from _FillValue)
            check(lib.nf_field_set_missing_value(ctypes.byref(self._h), float(missing_value)))
        check(lib.nf_field_set_sverdrup(ctypes.byref(self._h), 1 if sverdrup else 0))
        if compact:   # keep only (eU, eV) resident; the (ncell,4) copies and |.| arrays are derived at read-back
            check(lib.nf_field_set_compact(ctypes.byref(self._h), 1))
        if slab_range is not None:
            check(lib.nf_field_set_slab_range(ctypes.byref(self._h), int(slab_range[0]), int(slab_range[1])))
        self.slab_range = slab_range

        # --- layer thickness (field.py:51)
        self.bounds_depth = numpy.asarray(deptht_bounds)
        self.thickness = numpy.ascontiguousarray(self.bounds_depth[:, 1] - self.bounds_depth[:, 0], dtype=numpy.float64)
        if self.thickness.shape[0] != self.nz:
            raise RuntimeError('ERROR: deptht_bounds does not match the number of levels of uo')
        check(lib.nf_field_set_thickness(ctypes.byref(self._h), _lib.dptr(self.thickness), self.nz))

        # --- grid + transects (field.py:42-49): all polylines in one batched weight build
        self.gr = HorizGrid(_field=self)
        self._polylines = [numpy.ascontiguousarray(numpy.array(p, dtype=numpy.float64)).reshape(-1, 3)
                           for p in lonLatZPoints]
        self.plis = []
        for i, xyz in enumerate(self._polylines):
            tid = ctypes.c_int()
            check(lib.nf_field_add_transect(ctypes.byref(self._h), _lib.dptr(xyz), xyz.shape[0], 0, ctypes.byref(tid)))
            self.plis.append(_Transect(self, i, xyz))
        if unsupportedCells not in ('refuse', 'skip'):
            raise RuntimeError("ERROR: unsupportedCells must be 'refuse' or 'skip'")
        if unsupportedCells == 'skip':   # non-convex / pole-vertex cells drop out; the coverage warning below reports it
            check(lib.nf_field_set_unsupported_cells(ctypes.byref(self._h), 1))
        if overlappingCells not in ('refuse', 'warn'):
            raise RuntimeError("ERROR: overlappingCells must be 'refuse' or 'warn'")
        if overlappingCells == 'warn':   # a stretch of a line found in two overlapping cells counts twice; the warning below says so
            check(lib.nf_field_set_overlapping_cells(ctypes.byref(self._h), 1))
        check(lib.nf_field_build_weights(ctypes.byref(self._h), int(numCellsPerBucket), float(periodX)))
        n = ctypes.c_int()
        check(lib.nf_field_num_segments(ctypes.byref(self._h), ctypes.byref(n)))
        self._nseg = n.value
        self._tr_off = numpy.zeros(len(self.plis) + 1, numpy.int32)
        check(lib.nf_field_segment_offsets(ctypes.byref(self._h), self._tr_off.ctypes.data_as(_lib.c_int_p)))
        check(lib.nf_field_row_length(ctypes.byref(self._h), ctypes.byref(n)))
        self._rowlen = n.value
        self._row = numpy.zeros(self._row_width, numpy.float64)
        self._row_valid = False
        # coverage > 1 (overlapping cells: a stretch of the line would be counted twice) was refused by build_weights above
        # unless overlappingCells='warn'; coverage < 1 means part of the line lies in no cell: mint only warns there [recall],
        # and so does this
        n = ctypes.c_size_t()
        check(lib.nf_field_num_dropped_crossings(ctypes.byref(self._h), ctypes.byref(n)))
        self.droppedCrossings = n.value
        if self.droppedCrossings:
            import warnings
            warnings.warn(f'{self.droppedCrossings} crossing(s) of cells the weights are not defined on (not convex in the lon-lat '
                          f'plane / a corner at a geographic pole) were left out of the transects (unsupportedCells=\'skip\'); '
                          f'the coverage warnings below name the segments', RuntimeWarning, stacklevel=3)
        for i, cov in enumerate(self.getCoverage()):
            xyz = self._polylines[i]
            over = numpy.array([q for q in range(cov.size) if overlappingCells == 'warn' and
                                _lib.over_covered(cov[q], xyz[q], xyz[q + 1])], dtype=int)
            if over.size:
                import warnings
                warnings.warn(f'transect {i}: {over.size} of {cov.size} target segments are covered more than once by the cells '
                              f'of the grid (up to {cov[over].max():.9g} times, first: segment {over[0]}): that part of the line '
                              f'is counted twice', RuntimeWarning, stacklevel=3)
            low = numpy.nonzero(cov < 1.0 - 1.e-8)[0]
            if low.size:
                import warnings
                warnings.warn(f'transect {i}: {low.size} of {cov.size} target segments are not fully inside the grid '
                              f'(covered fraction {cov[low].min():.6g} .. {cov[low].max():.6g}, first: segment {low[0]}); '
                              f'the parts outside contribute no flux', RuntimeWarning, stacklevel=3)

        numCells = self.ny * self.nx
        self.dx = min((self.lonmax - self.lonmin) / float(self.nx), (self.latmax - self.latmin) / float(self.ny))
        self._arc = None

        # --- host mirrors of the per-step arrays (field.py:59-63); pinned, updated in place
        self.edgeFluxesUArray = self._host_zeros((numCells,))
        self.edgeFluxesVArray = self._host_zeros((numCells,))
        self.integratedVelocity = self._host_zeros((numCells, 4))
        self.maxAbsFlux = 0.

        # first step (field.py:65-67)
        self._compute(self.timeIndex)
        print(f'max vertically integrated edge |flux|: {self.maxAbsFlux}')

        self._lonlat = None
        # arrow seed points along the target lines (field.py:71-87)
        vectorPoints = []
        uVectors = []
        # (batch drivers -- readback=False -- never look at the arrows: a batch of 4 096 transects on the ORCA12-like grid would
        # seed 2 x 10^8 of them)
        for lonlatpts in (self._polylines if self._readback else []):
            for i in range(len(lonlatpts) - 1):
                begPoint = numpy.array(lonlatpts[i])
                endPoint = numpy.array(lonlatpts[i + 1])
                u = endPoint - begPoint
                distance = numpy.sqrt(u.dot(u))
                if distance == 0 or self.dx <= 0:
                    continue
                u /= distance
                nvpts = max(2, int(distance / self.dx))
                vdx = distance / float(nvpts - 1)
                # begPoint + u*j*vdx for j in range(nvpts) (field.py:84-86), vectorised over j
                vectorPoints.append(begPoint + (u * numpy.arange(nvpts)[:, None]) * vdx)
                uVectors.append(numpy.broadcast_to(u, (nvpts, 3)))
        self.uVectors = numpy.concatenate(uVectors) if uVectors else numpy.zeros((0, 3))
        vectorPoints = numpy.concatenate(vectorPoints) if vectorPoints else []
        self.vectorPoints = numpy.ascontiguousarray(vectorPoints) if len(vectorPoints) else numpy.zeros((0, 3))
        # compute the vector at the target line (field.py:89-95), from the resident planes (no host round trip)
        self.vectorValues = numpy.zeros((self.vectorPoints.shape[0], 3), numpy.float64)
        self.vinterp = None
        if self._readback:   # batch drivers (readback=False) never look at the arrows
            self.vinterp = mint.VectorInterp()
            self.vinterp.setGrid(self.gr.getMintGrid())
            self.vinterp.buildLocator(numCellsPerBucket=128, periodX=periodX)
            self.vinterp.findPoints(self.vectorPoints, tol2=1.e-12)
            self._update_vectors()

    # ------------------------------------------------------------------------------------------
    def _host_array(self, shape, dtype=numpy.float64):
        """Pinned host array (fast D2H / H2D); the allocation lives as long as any view of the array."""
        dtype = numpy.dtype(dtype)
        n = int(numpy.prod(shape))
        nbytes = max(n, 1) * dtype.itemsize
        block = _PinnedBlock(nbytes)
        buf = (ctypes.c_ubyte * nbytes).from_address(block.ptr)
        buf._owner = block  # the ctypes object is the numpy array's base: it keeps the block alive
        return numpy.ctypeslib.as_array(buf).view(dtype)[:n].reshape(shape)

    @property
    def _uv_dtype(self):
        """the dtype of uo / vo as numpy has it (_uv_code is how the C ABI has it)"""
        return numpy.dtype(numpy.float32 if self._uv_code == NF_F32 else numpy.float64)

    def _layout(self):
        """what the producers of nemoflux_amd._sources need to know of this Field"""
        return Layout(self.nt, self.nz, self.ny, self.nx, self._uv_dtype, self._uv_code, self._stream, self._host_array)

    def _host_zeros(self, shape):
        a = self._host_array(shape)
        a[...] = 0.0
        return a

    def __del__(self):
        try:
            if getattr(self, '_stager', None) is not None:
                self._stager.close()      # the prefetch thread writes into buffers this object owns
            if getattr(self, '_h', None):
                lib.nf_field_del(ctypes.byref(self._h))
        except Exception:
            pass

    def _download_points(self):
        pts = numpy.empty((self.ny * self.nx, 4, 3), numpy.float64)
        check(lib.nf_field_get_points(ctypes.byref(self._h), _lib.dptr(pts)))
        return pts

    @property
    def arcLengths(self):
        """(ncell, 4) great-circle edge lengths on the unit sphere (field.py:55-56, 170-181)."""
        if self._arc is None:
            self._arc = numpy.empty((self.ny * self.nx, 4), numpy.float64)
            check(lib.nf_field_get_arclengths(ctypes.byref(self._h), _lib.dptr(self._arc)))
        return self._arc

    @property
    def lonlat(self):
        """(ny, nx, 4, 3) corner coordinates for the VTK edge grids (field.py:138-143)."""
        if self._lonlat is None:
            self._lonlat = self.gr.getPoints().reshape((self.ny, self.nx, 4, 3))
        return self._lonlat

    def buildEdgeUVGrids(self, bounds_lon=None, bounds_lat=None):
        return self.lonlat

    def getSizes(self, shapeU=None):
        """field.py:122-136."""
        nt, nz, ny, nx = 1, 1, 0, 0
        if shapeU is None:
            return self.nt, self.nz, self.ny, self.nx
        if len(shapeU) == 4:
            nt, nz, ny, nx = shapeU
        elif len(shapeU) == 3:
            nz, ny, nx = shapeU
        elif len(shapeU) == 2:
            ny, nx = shapeU
        else:
            raise RuntimeError("ERROR: uo's shape does not match (t, z, y, x), (z, y, x) or (y, x)")
        return int(nt), int(nz), int(ny), int(nx)

    # ------------------------------------------------------------------------------------------
    def _stage(self, tIndex, prefetch_next=None):
        """Make step tIndex of a file-backed Field the one the engine reads (no-op for in-memory / HBM fields)."""
        if not (0 <= tIndex < self.nt):
            raise RuntimeError(f'ERROR: time index {tIndex} out of range [0, {self.nt})')
        if self._lazy is not None and self._lazy_step != tIndex:
            # one time step from the file(s): staged in pinned host memory or decoded into an HBM slab; the engine sees a
            # virtual (nt, nz, ny, nx) base that it only dereferences at step tIndex
            pu, pv, on_dev = self._stager.get(tIndex)
            self._lazy_step = tIndex
            off = tIndex * self._stager.step_bytes
            check(lib.nf_field_set_uv(ctypes.byref(self._h), pu - off, pv - off, self.nt, self._uv_code, on_dev, self._fill))
            # the steps that come next (fluxviz's 't' key, fluxplot's loop) are prepared on a host thread while the GPU works
            # on this one: the blocking C call below releases the GIL
            nxt = self._stager.next_after(tIndex)
            if prefetch_next is None or isinstance(prefetch_next, bool):
                self._stager.prefetch(nxt % self.nt if prefetch_next is None else (nxt if nxt < self.nt else -1))
            else:       # a step index: the next step of a walk over selected steps (meanEddySplit); -1: none
                self._stager.prefetch(int(prefetch_next))
        self._stage_cell_thickness(tIndex)

    def _compute(self, tIndex, readback=None, prefetch_next=None):
        self._stage(tIndex, prefetch_next)
        check(lib.nf_field_compute_flux(ctypes.byref(self._h), int(tIndex), _lib.dptr(self._row)))
        self._row_valid = True
        if self._readback if readback is None else readback:
            m = ctypes.c_double()
            check(lib.nf_field_read_step(ctypes.byref(self._h), _lib.dptr(self.integratedVelocity),
                                         _lib.dptr(self.edgeFluxesUArray), _lib.dptr(self.edgeFluxesVArray),
                                         ctypes.byref(m)))
            self.maxAbsFlux = max(self.maxAbsFlux, m.value)  # field.py:234
        return self._row

    def _update_vectors(self):
        if self.vectorValues.shape[0] and self.vinterp is not None:
            p = ctypes.c_void_p()
            check(lib.nf_field_device_ptr(ctypes.byref(self._h), 0, ctypes.byref(p)))
            self.vinterp.getFaceVectors(p.value, out=self.vectorValues, _layout=1)   # in place (fluxviz.py:301)

    def update(self):
        """field.py:112-120: recompute the current time step; host arrays are refreshed in place."""
        self._compute(self.timeIndex, readback=True)
        self._update_vectors()   # field.py:119-120

    def computeFlux(self, tIndex, readback=False):
        """BASELINE north_star's computeFlux(tIndex): set the time index, run the step on the GPU and return
        the total flux of every transect (list of floats).  = fluxplot.py:51-59 for one step."""
        self.timeIndex = int(tIndex)
        row = self._compute(self.timeIndex, readback=readback)
        return [float(row[self._nseg + i]) for i in range(len(self.plis))]

    @property
    def _row_width(self):
        """columns of the arrays that hold raw rows: row_length, but never 0 (a Field without transects)"""
        return max(self._rowlen, 1)

    def _rows_out(self, out, shape):
        """The `out=` tensor of the calls that leave raw rows in HBM: float64 of this shape, contiguous, on the GPU -- the
        library writes that many doubles through its pointer.  A new one when out is None."""
        import torch
        if out is None:
            return torch.empty(shape, dtype=torch.float64, device='cuda')
        if tuple(out.shape) != shape or not out.is_cuda or not out.is_contiguous() or out.dtype != torch.float64:
            raise RuntimeError(f'ERROR: out must be a contiguous float64 CUDA tensor of shape {shape}')
        return out

    def _product(self, stem, tIndex, front, carry=None, tracer=True, surfaces=False, width=None, out=None, prefetch_next=None):
        """The host rows, float64 of shape `front` + (row width,), of a per-step product of the C ABI for time step tIndex: the
        call `stem`, or `stem`_async into the tensor `out` when one is given.  Stages step tIndex first: uo / vo and the cell
        thickness, then the surfaces (surfaces=True), then the tracers (tracer=True).  carry (None: the call takes none) is
        passed as 0 / 1.  width: a function that gives the last axis where it is not the row width, called once the step is
        staged (the crossings); a result without elements makes no call."""
        tIndex = int(tIndex)
        self._stage(tIndex, prefetch_next)
        if surfaces:
            self._stage_surfaces(tIndex)
        if tracer:
            self._stage_tracer(tIndex)
        shape = tuple(front) + (self._row_width if width is None else width(),)
        args = (ctypes.byref(self._h), tIndex) + (() if carry is None else (1 if carry else 0,))
        if out is not None:
            out = self._rows_out(out, shape)
            if out.numel():
                check(getattr(lib, stem + '_async')(*args, ctypes.c_void_p(out.data_ptr())))
            return out.cpu().numpy()
        rows = numpy.zeros(shape, numpy.float64)
        if rows.size:
            check(getattr(lib, stem)(*args, _lib.dptr(rows)))
        return rows

    def _split_rows(self, rows):
        """(transect totals, per-segment sums) of rows laid out [segments | transects] along their last axis."""
        return rows[..., self._nseg:self._nseg + len(self.plis)], rows[..., :self._nseg]

    def getSegmentFluxes(self):
        """Per-target-segment sums of the last computed step, one array per transect."""
        return [numpy.array(self._row[self._tr_off[i]:self._tr_off[i + 1]]) for i in range(len(self.plis))]

    def computeAll(self, out=None):
        """All nt steps back to back on the GPU (no host round trip per step).  Returns (nt, ntransect)
        totals and (nt, nseg) per-segment sums.  `out`: optional torch CUDA tensor (nt, row_length) to
        receive the raw rows in HBM (for the RCCL reduce of nemoflux_amd.dist)."""
        import torch
        lazy = self._lazy is not None or self._cell_thickness_lazy()
        if out is not None or not lazy:
            out = self._rows_out(out, (self.nt, self._row_width))
        if lazy:
            # file-backed: one step on the GPU, the next one inflating into the other pinned slot (no wrap-around prefetch
            # after the last step)
            rows = numpy.array([self._compute(t, readback=False, prefetch_next=True).copy() for t in range(self.nt)])
            if out is not None:
                out.copy_(torch.from_numpy(rows))
            return self._split_rows(rows)
        check(lib.nf_field_compute_all_async(ctypes.byref(self._h), ctypes.c_void_p(out.data_ptr())))
        rows = out.cpu().numpy()
        return self._split_rows(rows)

    def computeFluxProfile(self, tIndex, out=None, prefetch_next=None):
        """Depth-resolved fluxes of time step tIndex: (nz, ntransect) totals and (nz, nseg) per-segment sums, row z = the
        flux carried by level z alone (the rows of computeFlux, one per level; their sum over z is the full-depth row up to
        rounding).  Levels this rank does not own (slab_range) are zeros.  The resident edge fluxes, the running max and the
        row of the last computeFlux are left as they are.  `out`: optional torch CUDA tensor (nz, row_length) that receives
        the raw rows in HBM (for nemoflux_amd.dist.reduce_rows)."""
        rows = self._product('nf_field_compute_profile', tIndex, (self.nz,), tracer=False, out=out, prefetch_next=prefetch_next)
        return self._split_rows(rows)

    def setTracer(self, tracer, fill_value=None, missing_value=None, reference=0.0, wrapX=True):
        """A tracer at T-points (potential temperature, salinity) for computeTracerFlux / computeTracerAll: the same
        (nt, nz, ny, nx) and dtype as uo / vo.  `tracer`: a host array (staged one time step at a time), a torch CUDA tensor
        or a DeviceArray (used in place), or a (path, name) pair read with nemoflux_amd.io one time step at a time, its CF
        markers and scale / offset decoded as for uo; or a nemoflux_amd.eos.Sigma(thetao, so, pref): potential density computed
        from temperature and salinity on the GPU, one time step at a time (it carries its own markers).  fill_value /
        missing_value: the tracer's own missing markers (a file's
        _FillValue / missing_value when not given; NaN always counts as missing).  reference: subtracted from every face value
        (theta_ref of a heat transport).  wrapX: the east face of the last column takes the first column as its neighbour
        (the periodic rule of the volume rows)."""
        self._tracer = self._tracer_slot(tracer, fill_value, missing_value, lib.nf_field_set_tracer,
                                         lib.nf_field_set_tracer_missing_value)
        check(lib.nf_field_set_tracer_reference(ctypes.byref(self._h), float(reference)))
        check(lib.nf_field_set_tracer_wrap(ctypes.byref(self._h), 1 if wrapX else 0))
        self._tracer_reference, self._tracer_wrapX = float(reference), bool(wrapX)

    def _tracer_slot(self, tracer, fill_value, missing_value, set_tracer, set_missing):
        """Hand a tracer at T-points to one of the engine's two tracer slots (set_tracer / set_missing: the slot's C calls) and
        return what staging it needs: host arrays and device arrays are set once; a (path, name) pair is opened with its CF
        markers and read one time step at a time into one pinned host buffer by _stage_slot; a Sigma is computed one time step
        at a time into one device buffer by _stage_slot."""
        from .eos import Sigma
        if isinstance(tracer, Sigma):
            if fill_value is not None or missing_value is not None:
                raise RuntimeError('ERROR: a Sigma carries the markers of thetao and so itself; give them to Sigma(...)')
            return self._sigma_slot(tracer, set_tracer, set_missing)
        given = tracer
        tracer, markers = _open_pair(tracer)
        fill, missing = _two_markers(markers, fill_value, missing_value, f'tracer {given[1]} carries' if markers else '')
        shape = tuple(int(x) for x in tracer.shape)
        if self.getSizes(shape) != (self.nt, self.nz, self.ny, self.nx):
            raise RuntimeError(f'ERROR: the tracer has shape {shape}; uo/vo have (nt, nz, ny, nx) = '
                               f'{(self.nt, self.nz, self.ny, self.nx)}')
        slot = dict(lazy=None, step=-1, stage=None, code=_dtype_code(tracer), fill=fill, missing=missing)
        ptr = _lib.device_pointer(tracer)
        on_dev = 1
        if hasattr(tracer, 'read_step'):
            # file-backed: step t is read into one pinned host buffer and handed over as a host-resident tracer through a
            # virtual (nt, nz, ny, nx) base that the engine only dereferences at step t (as _stage does for uo / vo)
            slot['lazy'] = (tracer,)
            buf = self._host_array((self.nz, self.ny, self.nx), numpy.dtype(tracer.dtype).newbyteorder('='))
            slot['stage'] = self._slot_stager(set_tracer, slot['code'], 0, fill, lambda t: tracer.read_step(t, out=buf),
                                              [buf.ctypes.data], buf.nbytes)
            ptr = None
        elif ptr is None:
            tracer = _native(tracer)
            ptr, on_dev = tracer.ctypes.data, 0
        slot['keep'] = tracer    # a borrowed buffer must outlive the handle
        if ptr is not None:
            check(set_tracer(ctypes.byref(self._h), ptr, self.nt, slot['code'], on_dev, fill))
        check(set_missing(ctypes.byref(self._h), missing))
        return slot

    def _slot_stager(self, set_call, code, on_dev, fill, fetch, ptrs, nbytes):
        """stage(t) of a slot that needs work at every step -- a tracer, or the e3u / e3v pair of a time-varying cell thickness:
        fetch(t) brings step t to the addresses ptrs (nbytes each; fetch keeps their owner alive), and set_call hands them
        to the engine through a virtual (nt, nz, ny, nx) base that it only dereferences at step t.  (The closure holds the
        handle, not the Field: a slot must not keep its Field alive.)"""
        h, nt = self._h, self.nt

        def stage(t):
            fetch(t)
            check(set_call(ctypes.byref(h), *[p - t * nbytes for p in ptrs], nt, code, on_dev, fill))
        return stage

    def _sigma_slot(self, sigma, set_tracer, set_missing):
        """The slot of a derived tracer (nemoflux_amd.eos.Sigma): thetao and so each stay where they are -- device arrays are
        read in place by offset, host arrays and file variables go one time step at a time through a pinned buffer of their
        own into a device buffer -- and _stage_slot has a SigmaProducer write step t into its (nz, ny, nx) device buffer of the
        dtype of uo / vo, which the engine reads as a device-resident tracer whose fill is NaN."""
        self._check_sigma(sigma, 'the Sigma')
        sg = SigmaProducer(self._layout(), sigma)
        slot = dict(lazy=tuple(sigma.sources), step=-1, code=self._uv_code, fill=numpy.nan, missing=numpy.nan, keep=sigma, sigma=sg,
                    stage=self._slot_stager(set_tracer, self._uv_code, 1, numpy.nan, lambda t: sg.run(t, sg.out.ptr), [sg.out.ptr],
                                            sg.nbytes))
        check(set_missing(ctypes.byref(self._h), numpy.nan))
        return slot

    def _check_sigma(self, sigma, what):
        uv_dtype = self._uv_dtype
        if self.getSizes(sigma.shape) != (self.nt, self.nz, self.ny, self.nx):
            raise RuntimeError(f'ERROR: thetao and so of {what} have shape {sigma.shape}; uo/vo have (nt, nz, ny, nx) = '
                               f'{(self.nt, self.nz, self.ny, self.nx)}')
        if sigma.dtype != uv_dtype:
            raise RuntimeError(f'ERROR: thetao and so of {what} are {sigma.dtype.name}, uo/vo are {uv_dtype.name}')

    def _sigma_refused(self, what):
        for slot in (getattr(self, '_tracer', None), getattr(self, '_class_tracer', None)):
            if slot is not None and slot.get('sigma') is not None:
                raise RuntimeError(f'ERROR: {what}: this Field holds a Sigma (potential density computed from thetao and so); '
                                   f'the mean of sigma and sigma of the means are different quantities and neither is chosen '
                                   f'here: set a plain tracer')

    def _stage_slot(self, slot, tIndex):
        """make step tIndex of a slot that needs work at every step -- a file-backed or derived tracer, or the e3u / e3v pair
        of a time-varying cell thickness -- the one the engine reads (no-op for in-memory / HBM arrays)"""
        if slot is not None and slot.get('stage') is not None and slot['step'] != tIndex:
            slot['stage'](tIndex)
            slot['step'] = tIndex

    def _stage_tracer(self, tIndex):
        if getattr(self, '_tracer', None) is None:
            raise RuntimeError('ERROR: call setTracer first')
        self._stage_slot(self._tracer, tIndex)
        self._stage_slot(getattr(self, '_class_tracer', None), tIndex)

    def setClassTracer(self, tracer, fill_value=None, missing_value=None):
        """A second tracer at T-points (potential density) whose classes computeClassTransport and
        computeClassTracerTransport bin by, instead of the tracer of setTracer -- which is then only carried: heat by density
        class.  Same (nt, nz, ny, nx) and dtype as uo / vo; a host array, a torch CUDA tensor or DeviceArray, or a
        (path, name) pair read one time step at a time, as in setTracer.  It has its own missing markers, no reference, and
        the wrapX of setTracer.  setClassTracer(None): back to the tracer of setTracer as the class field."""
        self._class_tracer = None
        if tracer is None:
            check(lib.nf_field_set_class_tracer(ctypes.byref(self._h), None, 0, NF_F64, 0, numpy.nan))
            return
        self._class_tracer = self._tracer_slot(tracer, fill_value, missing_value, lib.nf_field_set_class_tracer,
                                               lib.nf_field_set_class_tracer_missing_value)

    # ------------------------------------------------------------------------------------------
    def setCellThickness(self, e3u, e3v=None, fill_value=None, missing_value=None):
        """Per-cell layer thicknesses (partial steps, z* / variable-volume runs) in place of the one number per level of
        deptht_bounds: e3u at the U points (the index of uo), e3v at the V points (the index of vo) -- the model's e3u / e3v,
        or thkcello on the U and V grids.  Shape (nz, ny, nx) or (1, nz, ny, nx): static; (nt, nz, ny, nx): one per time step.
        Each of e3u, e3v is a host array, a torch CUDA tensor or a DeviceArray (used in place), or a (path, name) pair read
        with nemoflux_amd.io, its CF markers and scale / offset decoded as for uo: a time-varying pair one step at a time
        into pinned buffers, a static one once.  A static host array of another float dtype is cast to the dtype of uo / vo
        (a float64 mesh_mask thickness beside float32 velocities is rounded to float32); a device array or a time-varying
        array of another dtype raises.  fill_value / missing_value: the thickness's own missing markers (a file's when not
        given); a thickness that is NaN or a marker counts as 0.
        computeFlux, computeAll, update, computeFluxProfile, computeTracerFlux, computeTracerAll, computeAreaProfile, computeClassArea and
        computeGrossProfile, computeGrossClassTransport and computeGrossClassRemap (both forms) then integrate with these thicknesses; computeTracerProfile, computeClassTransport and computeClassTracerTransport raise while they are
        set.  timeMean and meanEddyTracerTransport carry a static thickness over to the mean state and take a time-varying one
        with thicknessWeighted=True (thickness-weighted mean velocities, mean thicknesses).  setCellThickness(None, None) goes
        back to deptht_bounds.
        setCellThickness(FaceThickness(e3t, rule, ...)) (nemoflux_amd.thickness; e3v left None): e3u and e3v derived on the GPU
        from the thickness at T-points -- e3t of grid_T, thkcello -- a static e3t once, a time-varying one step by step into
        two (nz, ny, nx) device buffers; the descriptor carries its own markers.
        setCellThickness(SshThickness(ssh, e3u0, e3v0, ...)) (the same module; e3v left None): the z* thicknesses
        e3u0 * (1 + ssh_u / hu0) derived on the GPU from the 2-D sea surface height and the static mesh_mask thicknesses -- one
        (ny, nx) plane per time step in place of a volume -- handled like a FaceThickness from there on."""
        from .thickness import FaceThickness, SshThickness
        self._e3 = None
        self._row_valid = False
        if isinstance(e3u, SshThickness):
            if e3v is not None:
                raise RuntimeError('ERROR: setCellThickness: an SshThickness describes both e3u and e3v; leave e3v None')
            if fill_value is not None or missing_value is not None:
                raise RuntimeError('ERROR: an SshThickness carries the markers of ssh and of the statics itself; give them to '
                                   'SshThickness(...)')
            self._ssh_thickness_slot(e3u)
            return
        if isinstance(e3u, FaceThickness):
            if e3v is not None:
                raise RuntimeError('ERROR: setCellThickness: a FaceThickness describes both e3u and e3v; leave e3v None')
            if fill_value is not None or missing_value is not None:
                raise RuntimeError('ERROR: a FaceThickness carries the markers of e3t and of the statics itself; give them to '
                                   'FaceThickness(...)')
            self._face_thickness_slot(e3u)
            return
        if e3u is None or e3v is None:
            if e3u is not None or e3v is not None:
                raise RuntimeError('ERROR: setCellThickness needs both e3u and e3v, or None for both')
            check(lib.nf_field_set_cell_thickness(ctypes.byref(self._h), None, None, 0, NF_F64, 0, numpy.nan))
            self._face_keep = None
            return
        uv_dtype = self._uv_dtype
        markers, arrs = [], []
        for e3, which in ((e3u, 'e3u'), (e3v, 'e3v')):
            e3, own = _open_pair(e3)
            for m in own:
                if m not in markers:
                    markers.append(m)
            shape = tuple(int(x) for x in e3.shape)
            nt_th = self.getSizes(shape)[0] if len(shape) in (3, 4) else -1
            if len(shape) not in (3, 4) or self.getSizes(shape)[1:] != (self.nz, self.ny, self.nx) or nt_th not in (1, self.nt):
                raise RuntimeError(f'ERROR: {which} has shape {shape}; need (nz, ny, nx) = {(self.nz, self.ny, self.nx)}, '
                                   f'(1, nz, ny, nx) or (nt, nz, ny, nx) = {(self.nt, self.nz, self.ny, self.nx)}')
            if hasattr(e3, 'read_step') and nt_th == 1:
                e3 = e3.read_step(0)       # a static file variable: read once
            arrs.append((e3, nt_th))
        if arrs[0][1] != arrs[1][1]:
            raise RuntimeError(f'ERROR: e3u has {arrs[0][1]} time step(s) and e3v {arrs[1][1]}: both static or both per time step')
        nt_th = arrs[0][1]
        fill, missing = _two_markers(markers, fill_value, missing_value, 'e3u / e3v carry')
        slot = dict(lazy=None, step=-1, stage=None, code=self._uv_code, nt=nt_th, fill=fill, missing=missing, keep=[], arrays=[])
        ptrs, on_dev, lazy = [], None, []
        for (e3, _), which in zip(arrs, ('e3u', 'e3v')):
            dt = numpy.dtype(_native_dtype(e3))
            ptr = _lib.device_pointer(e3)
            is_lazy = hasattr(e3, 'read_step')
            if dt != uv_dtype:
                if ptr is not None or is_lazy or nt_th != 1 or dt.kind != 'f':
                    raise RuntimeError(f'ERROR: {which} is {dt.name}, uo/vo are {uv_dtype.name}: only a static host array of '
                                       f'another float dtype is cast')
                e3 = numpy.asarray(e3).astype(uv_dtype)
            dev = ptr is not None
            if on_dev is not None and dev != on_dev:
                raise RuntimeError('ERROR: e3u and e3v must both be host arrays or both be device arrays')
            on_dev = dev
            lazy.append(is_lazy)
            if is_lazy:
                buf = self._host_array((self.nz, self.ny, self.nx), uv_dtype)
                slot['keep'].append(buf)
                ptrs.append(buf)
            elif not dev:
                e3 = _native(e3)
                ptrs.append(e3.ctypes.data)
            else:
                ptrs.append(ptr)
            slot['keep'].append(e3)     # a borrowed buffer must outlive the handle
            slot['arrays'].append(e3)
        if lazy[0] != lazy[1]:
            raise RuntimeError('ERROR: e3u and e3v must both be read from files one step at a time, or neither')
        if lazy[0]:
            slot['lazy'] = pair = (arrs[0][0], arrs[1][0])
            slot['stage'] = self._slot_stager(lib.nf_field_set_cell_thickness, self._uv_code, 0, fill,
                                              lambda t: [src.read_step(t, out=buf) for src, buf in zip(pair, ptrs)],
                                              [buf.ctypes.data for buf in ptrs], ptrs[0].nbytes)
        else:
            check(lib.nf_field_set_cell_thickness(ctypes.byref(self._h), ptrs[0], ptrs[1], nt_th, self._uv_code,
                                                  1 if on_dev else 0, fill))
        check(lib.nf_field_set_cell_thickness_missing_value(ctypes.byref(self._h), missing))
        self._e3 = slot
        self._face_keep = None

    def _check_static_input(self, a, which, dims):
        uv_dtype = self._uv_dtype
        names = ('(nz, ny, nx)', '(1, nz, ny, nx)') if len(dims) == 3 else ('(ny, nx)', '(1, ny, nx)')
        shape = tuple(int(x) for x in a.shape)
        if shape not in (tuple(dims), (1,) + tuple(dims)):
            raise RuntimeError(f'ERROR: {which} has shape {shape}; need {names[0]} = {tuple(dims)} or {names[1]}')
        dt = numpy.dtype(_native_dtype(a))
        if dt != uv_dtype and (_lib.device_pointer(a) is not None or dt.kind != 'f'):
            raise RuntimeError(f'ERROR: {which} is {dt.name}, uo/vo are {uv_dtype.name}: only a static host array of '
                               f'another float dtype is cast')

    def _face_thickness_slot(self, ft):
        """The cell-thickness slot of a derived pair (nemoflux_amd.thickness.FaceThickness).  e3t stays where it is -- a device
        array is read in place by offset, a host array or a file variable goes one time step at a time through a pinned buffer
        into a device buffer -- the statics go to the device once, and nf_face_thickness writes two (nz, ny, nx) device buffers
        of the dtype of uo / vo on the Field's stream.  A static e3t: computed once, here, and set as a static HBM thickness.
        A time-varying one: _stage_slot computes step t and hands the buffers over through a virtual (nt, nz, ny, nx) base."""
        uv_dtype = self._uv_dtype
        dims = (self.nz, self.ny, self.nx)
        shape = ft.shape
        nt_th = self.getSizes(shape)[0] if len(shape) in (3, 4) else -1
        if len(shape) not in (3, 4) or self.getSizes(shape)[1:] != dims or nt_th not in (1, self.nt):
            raise RuntimeError(f'ERROR: e3t has shape {shape}; need (nz, ny, nx) = {dims}, (1, nz, ny, nx) or '
                               f'(nt, nz, ny, nx) = {(self.nt,) + dims}')
        if nt_th == 1:
            self._check_static_input(ft.e3t, 'e3t', dims)
        elif ft.dtype != uv_dtype:
            raise RuntimeError(f'ERROR: e3t is {ft.dtype.name}, uo/vo are {uv_dtype.name}: only a static host array of '
                               f'another float dtype is cast')
        for a, which in zip(ft.statics, ('e3t0', 'e3u0', 'e3v0')):
            self._check_static_input(a, which, dims)
        self._derived_slot(ThicknessProducer.face(self._layout(), ft, nt_th), ft.e3t, nt_th)

    def _ssh_thickness_slot(self, st):
        """The cell-thickness slot of a z* pair derived from the sea surface height (nemoflux_amd.thickness.SshThickness).  The
        static face thicknesses (given, or derived once from e3t0 by nf_face_thickness with NF_E3_MIN), the column depths
        (given, or nf_column_depth of the face statics over all levels, whatever levels this rank owns) and the areas go to the
        device once; ssh stays where it is -- a (ny, nx) plane in HBM is read in place by offset, a host plane (a file's ssh
        is a host array by now: the descriptor read it whole) goes through a pinned buffer -- and nf_ssh_thickness writes the slot's two (nz, ny, nx) device buffers on the Field's
        stream, as nf_face_thickness does for a FaceThickness: the rest is _derived_slot."""
        uv_dtype = self._uv_dtype
        dims, cells = (self.nz, self.ny, self.nx), (self.ny, self.nx)
        shape = st.shape
        nt_th = 1 if len(shape) == 2 else (shape[0] if len(shape) == 3 else -1)
        if shape[-2:] != cells or nt_th not in (1, self.nt):
            raise RuntimeError(f'ERROR: ssh has shape {shape}; need (ny, nx) = {cells}, (1, ny, nx) or (nt, ny, nx) = '
                               f'{(self.nt,) + cells}')
        if nt_th == 1:
            self._check_static_input(st.ssh, 'ssh', cells)
        elif st.dtype != uv_dtype:
            raise RuntimeError(f'ERROR: ssh is {st.dtype.name}, uo/vo are {uv_dtype.name}: only a static host array of '
                               f'another float dtype is cast')
        for a, which in zip(st.statics, ('e3t0',) if st.from_e3t0 else ('e3u0', 'e3v0')):
            self._check_static_input(a, which, dims)
        planes = [(a, w) for a, w in zip(st.depths or (), ('hu0', 'hv0'))]
        planes += [(a, f'areas[{k}]') for k, a in enumerate(st.areas or ())]
        for a, which in planes:
            shp, dt = tuple(int(x) for x in a.shape), numpy.dtype(_native_dtype(a))
            if shp not in (cells, (1,) + cells):
                raise RuntimeError(f'ERROR: {which} has shape {shp}; need (ny, nx) = {cells} or (1, ny, nx)')
            if dt != numpy.float64 and (_lib.device_pointer(a) is not None or dt.kind != 'f'):
                raise RuntimeError(f'ERROR: {which} is {dt.name}: a device array must be float64, a host array a float array')
        self._derived_slot(ThicknessProducer.ssh(self._layout(), st, nt_th), st.ssh, nt_th)

    def _derived_slot(self, producer, src, nt_th):
        """the common part of the derived cell-thickness slots: producer.run(t, e3u_ptr, e3v_ptr) writes the pair of step t of
        src on the Field's stream.  A static src: computed once, here, and set as a static HBM thickness.  A time-varying
        one: _stage_slot computes step t into the producer's two (nz, ny, nx) device buffers and hands them over through a
        virtual (nt, nz, ny, nx) base."""
        uv_dtype, dims, nan = self._uv_dtype, (self.nz, self.ny, self.nx), numpy.nan
        outs = [b.ptr for b in producer.out]
        slot = dict(lazy=None, step=-1, stage=None, code=self._uv_code, nt=nt_th, fill=nan, missing=nan, keep=producer)
        if nt_th == 1:
            producer.run(0, *outs)
            check(lib.nf_synchronize())
            slot['arrays'] = [_lib.DeviceArray(b.ptr, dims, uv_dtype, keepalive=b) for b in producer.out]
            check(lib.nf_field_set_cell_thickness(ctypes.byref(self._h), outs[0], outs[1], 1, self._uv_code, 1, nan))
        else:
            slot['lazy'] = (src,)
            slot['stage'] = self._slot_stager(lib.nf_field_set_cell_thickness, self._uv_code, 1, nan,
                                              lambda t: producer.run(t, *outs), outs, producer.nbytes)
            slot['arrays'] = [_DerivedThickness(slot, producer, k, (self.nt,) + dims, uv_dtype) for k in (0, 1)]
        check(lib.nf_field_set_cell_thickness_missing_value(ctypes.byref(self._h), nan))
        self._e3 = slot
        self._face_keep = slot       # the engine reads these buffers until another thickness is set

    def _cell_thickness_lazy(self):
        e3 = getattr(self, '_e3', None)
        return e3 is not None and e3['lazy'] is not None

    def _stage_cell_thickness(self, tIndex):
        """make step tIndex of a file-backed, time-varying cell thickness the one the engine reads"""
        self._stage_slot(getattr(self, '_e3', None), tIndex)

    def computeTracerFlux(self, tIndex):
        """Tracer transport of time step tIndex across the transects (setTracer first): (ntransect,) totals and (nseg,)
        per-segment sums in tracer x flux units (x rho0 * c_p for a heat transport in W, and x 1e6 in Sverdrup mode).  Levels
        this rank does not own (slab_range) contribute nothing.  The volume rows, resident edge fluxes and the running max are
        left as they are."""
        tIndex = int(tIndex)
        self._stage(tIndex)
        self._stage_tracer(tIndex)
        row = numpy.zeros(self._row_width, numpy.float64)
        check(lib.nf_field_compute_tracer_flux(ctypes.byref(self._h), tIndex, _lib.dptr(row)))
        return self._split_rows(row)

    def computeTracerAll(self, out=None):
        """Tracer transport of all nt steps: (nt, ntransect) totals and (nt, nseg) per-segment sums.  `out`: optional torch
        CUDA tensor (nt, row_length) that receives the raw rows in HBM (for nemoflux_amd.dist.reduce_rows)."""
        import torch
        lazy = (self._lazy is not None or (getattr(self, '_tracer', None) or {}).get('lazy') is not None or
                self._cell_thickness_lazy())
        if out is not None or not lazy:
            out = self._rows_out(out, (self.nt, self._row_width))
        if lazy:
            # file-backed fields or tracer: one step at a time through the host
            rows = numpy.zeros((self.nt, self._row_width), numpy.float64)
            for t in range(self.nt):
                tot, seg = self.computeTracerFlux(t)
                rows[t, :self._nseg], rows[t, self._nseg:self._nseg + len(self.plis)] = seg, tot
            if out is not None:
                out.copy_(torch.from_numpy(rows))
        else:
            self._stage_tracer(0)
            check(lib.nf_field_compute_tracer_all_async(ctypes.byref(self._h), ctypes.c_void_p(out.data_ptr())))
            rows = out.cpu().numpy()
        return self._split_rows(rows)

    def computeTracerProfile(self, tIndex, out=None, prefetch_next=None):
        """Depth-resolved tracer transport of time step tIndex (setTracer first): (nz, ntransect) totals and (nz, nseg)
        per-segment sums, row z = the tracer transport carried by level z alone -- the rows of computeFluxProfile with every
        term times the tracer at its face (reference subtracted), and the computeTracerFlux row of a field whose only layer is
        level z, bit for bit; their sum over z is the computeTracerFlux row up to rounding.  Levels this rank does not own
        (slab_range) are zeros.  Leaves the resident edge fluxes, the running max, the row of the last computeFlux and the
        tracer rows as they are.  `out`: optional contiguous float64 torch CUDA tensor (nz, row_length) that receives the raw
        rows in HBM (for nemoflux_amd.dist.reduce_rows)."""
        rows = self._product('nf_field_compute_tracer_profile', tIndex, (self.nz,), out=out, prefetch_next=prefetch_next)
        return self._split_rows(rows)

    def computeAreaProfile(self, tIndex, out=None, prefetch_next=None):
        """Section area and area-weighted tracer of time step tIndex, level by level (setTracer first): the pair
        (area, tracerArea), each split like computeFluxProfile into (nz, ntransect) totals and (nz, nseg) per-segment sums.
        area[z] = sum of |w| * th * arc over the faces of level z that count (velocity present, tracer face value finite),
        tracerArea[z] = the same sum with every term times (tracer face value - reference); th is thickness[z], or the cell
        thickness at the face when one is set.  No Sverdrup scale: only ratios of these rows are used (overturningGyre).  For
        a line that cuts cells obliquely the area is the staircase area (zonal plus meridional extent): a weight for the
        mean, not a geometric length.  Levels this rank does not own (slab_range) are zeros.  Leaves the resident edge fluxes,
        the running max, the row of the last computeFlux and the tracer rows as they are.  `out`: optional contiguous float64
        torch CUDA tensor (2, nz, row_length) that receives the raw rows in HBM (for nemoflux_amd.dist.reduce_rows)."""
        rows = self._product('nf_field_compute_area_profile', tIndex, (2, self.nz), out=out, prefetch_next=prefetch_next)
        return self._split_rows(rows[0]), self._split_rows(rows[1])

    def computeGrossProfile(self, tIndex, carry=False, out=None, prefetch_next=None):
        """Gross transports of time step tIndex, level by level: (totals, segments) of shape (2, nz, ntransect) and
        (2, nz, nseg), part 0 = P, what goes through the section in the direction computeFlux counts positive, part 1 = N,
        what comes back (<= 0 in the volume form).  Every term of the computeFluxProfile row goes to P where it is > 0 and to N
        where it is < 0, per weight entry, slot and level; P + N is that row up to rounding.  carry=True (setTracer first): the
        terms of computeTracerProfile instead, split by the direction of the water at their slot, not by their own sign -- P is
        what the flow carries forward, N what it carries back; this form takes a cell thickness (setCellThickness) too.
        Levels this rank does not own (slab_range) are zeros.  Leaves the resident edge fluxes, the running max, the row of the
        last computeFlux and the tracer rows as they are.  `out`: optional contiguous float64 torch CUDA tensor
        (2 * nz, row_length), P's rows then N's, that receives the raw rows in HBM (for nemoflux_amd.dist.reduce_rows)."""
        rows = self._product('nf_field_compute_gross_profile', tIndex, (2 * self.nz,), carry=bool(carry),
                             tracer=carry, out=out, prefetch_next=prefetch_next)
        return self._split_rows(rows.reshape(2, self.nz, self._row_width))

    def _num_crossings(self):
        n = ctypes.c_size_t()
        check(lib.nf_field_num_crossings(ctypes.byref(self._h), ctypes.byref(n)))
        return n.value

    def getCrossings(self):
        """The crossings of the batched transect set: a Crossings object (see there), in the record order of getWeights() --
        crossing k is entries 4k .. 4k + 3.  Identical duplicates (halo columns, a north-fold row) keep their separate records
        with the same [ta, tb] and half the weight each; a crossing found through a periodic image has ta, tb in the parameter
        of its own target segment, so its lon0 .. lon1 lie on the line as the caller gave it."""
        n = self._num_crossings()
        seg, cell = numpy.zeros(n, numpy.int32), numpy.zeros(n, numpy.int64)
        ta, tb = numpy.zeros(n, numpy.float64), numpy.zeros(n, numpy.float64)
        if n:
            check(lib.nf_field_get_crossings(ctypes.byref(self._h), seg.ctypes.data_as(_lib.c_int_p),
                                             cell.ctypes.data_as(_lib.c_int64_p), _lib.dptr(ta), _lib.dptr(tb)))
        off = numpy.asarray(self._tr_off, dtype=numpy.int64)
        transect = numpy.searchsorted(off, seg, side='right') - 1
        # per global segment: its end points and the distance along its transect at which it begins
        p0 = numpy.concatenate([p[:-1, :2] for p in self._polylines] + [numpy.zeros((0, 2))])
        p1 = numpy.concatenate([p[1:, :2] for p in self._polylines] + [numpy.zeros((0, 2))])
        length = _arc_length(p0[:, 0], p0[:, 1], p1[:, 0], p1[:, 1])
        start = numpy.zeros(self._nseg, numpy.float64)
        for q in range(len(self.plis)):
            a, b = off[q], off[q + 1]
            start[a:b] = numpy.concatenate([[0.], numpy.cumsum(length[a:b])[:-1]]) if b > a else []
        d = p1[seg] - p0[seg]
        return Crossings(segment=seg, transect=transect.astype(numpy.int32), offsets=numpy.searchsorted(seg, off, side='left'),
                         cell=cell, j=cell // self.nx, i=cell % self.nx, ta=ta, tb=tb,
                         lon0=p0[seg, 0] + ta * d[:, 0], lat0=p0[seg, 1] + ta * d[:, 1],
                         lon1=p0[seg, 0] + tb * d[:, 0], lat1=p0[seg, 1] + tb * d[:, 1],
                         s0=start[seg] + ta * length[seg], s1=start[seg] + tb * length[seg])

    def computeCrossings(self, tIndex, carry=False, out=None, prefetch_next=None):
        """The integrand of every other product, for time step tIndex: per level and crossing (getCrossings: the piece of one
        target segment inside one grid cell) what flows through the piece, its section area and the tracer on it.  Returns
        (2, nz, ncross) = q, g, or with carry=True (setTracer first) (4, nz, ncross) = q, c, a, b:
            q  the volume transport through the piece: the crossing's terms of computeFluxProfile (Sverdrup scale when on)
            g  its section area |w| * th * arc over the faces whose velocity is present -- no tracer condition, no scale
            c  the tracer transport through the piece: its terms of computeTracerProfile (of P + N of
               computeGrossProfile(carry=True) with a cell thickness)
            a, b  its terms of computeAreaProfile: the area of the faces that count and that area times (tracer - reference)
        Both forms take a cell thickness (setCellThickness).  The sum of a plane over a segment's crossings is that segment's
        column of the product named, up to rounding (bit for bit where the segment has one crossing).  Nothing is reduced, so
        the planes of sharded ranks add up exactly; levels this rank does not own (slab_range) are zeros.  Leaves the resident
        edge fluxes, the running max, the row of the last computeFlux and the tracer rows as they are.  `out`: optional
        contiguous float64 torch CUDA tensor of the result's shape that receives the planes in HBM."""
        if carry not in (False, True, 0, 1):
            raise RuntimeError(f'ERROR: carry must be False or True, got {carry!r}')
        return self._product('nf_field_compute_crossings', tIndex, (4 if carry else 2, self.nz), carry=bool(carry), tracer=carry,
                             width=self._num_crossings, out=out, prefetch_next=prefetch_next)

    @staticmethod
    def _crossing_area(parts):
        P = numpy.asarray(parts, dtype=numpy.float64)
        if P.ndim != 3 or P.shape[0] not in (2, 4):
            raise ValueError(f'the planes of computeCrossings have shape (2 or 4, nz, ncross), got {P.shape}')
        return P, P[1] if P.shape[0] == 2 else P[2]

    @staticmethod
    def crossingVelocity(parts):
        """Mean normal velocity through every piece and level: q / g of the volume form, q / a of the carried form (the area of
        the faces that also have a tracer value), (nz, ncross); NaN where the area is 0.  In the units of uo / vo without the Sverdrup scale;
        with it q carries the factor 6.371 (Earth radius / 1e6) and the areas never do, so the ratio is 6.371 times the
        velocity: divide by 6.371 for m/s."""
        P, area = Field._crossing_area(parts)
        with numpy.errstate(divide='ignore', invalid='ignore'):
            return numpy.where(area != 0.0, P[0] / area, numpy.nan)

    @staticmethod
    def crossingTracer(parts, reference=0.0):
        """Mean tracer on every piece and level, from the carried form's planes: reference + b / a, (nz, ncross); NaN where
        a == 0.  `reference`: the reference of setTracer, which b has subtracted."""
        P = numpy.asarray(parts, dtype=numpy.float64)
        if P.ndim != 3 or P.shape[0] != 4:
            raise ValueError(f'crossingTracer needs the planes of computeCrossings(carry=True), (4, nz, ncross), got {P.shape}')
        with numpy.errstate(divide='ignore', invalid='ignore'):
            return numpy.where(P[2] != 0.0, float(reference) + P[3] / P[2], numpy.nan)

    @staticmethod
    def cumulativeTransport(parts, crossings, ztop=None, zbot=None, bounds_depth=None):
        """Cumulative volume transport along every transect, (ncross,): per transect the running sum, in record order, of q
        summed over depth -- or over the depth band [ztop, zbot] as in depthBandFlux (bounds_depth (nz, 2) is then needed).
        The last value of a transect is its computeFlux up to rounding.  parts: the planes of either form of
        computeCrossings; crossings: getCrossings()."""
        P, _ = Field._crossing_area(parts)
        q = P[0]
        if q.shape[1] != len(crossings):
            raise ValueError(f'cumulativeTransport: {q.shape[1]} columns for {len(crossings)} crossings')
        if ztop is None and zbot is None:
            col = q.sum(axis=0)
        else:
            if ztop is None or zbot is None or bounds_depth is None:
                raise ValueError('cumulativeTransport: a depth band needs ztop, zbot and bounds_depth')
            ztop, zbot = float(ztop), float(zbot)
            if not ztop <= zbot:
                raise ValueError(f'cumulativeTransport: need ztop <= zbot, got {ztop}, {zbot}')
            if numpy.shape(bounds_depth) != (q.shape[0], 2):
                raise ValueError(f'cumulativeTransport: bounds_depth must have shape {(q.shape[0], 2)}, got '
                                 f'{numpy.shape(bounds_depth)}')
            col = _band_sum(q, bounds_depth, ztop, zbot)
        out = numpy.zeros(col.shape, numpy.float64)
        off = numpy.asarray(crossings.offsets)
        for p in range(off.size - 1):
            out[off[p]:off[p + 1]] = numpy.cumsum(col[off[p]:off[p + 1]])
        return out

    @staticmethod
    def grossTransport(parts, ztop=None, zbot=None, bounds_depth=None):
        """Depth sum of both parts of computeGrossProfile: parts (2, nz, n), totals or segments alike, gives (2, n) = P, N
        (of the parts of computeGrossClassTransport, (2, nedges+2, n): the sum over the classes, without a band).
        With ztop < zbot (the units of deptht_bounds) the sum over that depth band instead, level z entering with
        overlap([ztop, zbot], layer z) / thickness[z] as in depthBandFlux; bounds_depth (nz, 2) is then needed (a Field's
        bounds_depth)."""
        P = numpy.asarray(parts, dtype=numpy.float64)
        if P.ndim < 2 or P.shape[0] != 2:
            raise ValueError(f'grossTransport: the parts must have shape (2, nz, ...), got {P.shape}')
        if ztop is None and zbot is None:
            return P.sum(axis=1)
        if ztop is None or zbot is None or bounds_depth is None:
            raise ValueError('grossTransport: a depth band needs ztop, zbot and bounds_depth')
        ztop, zbot = float(ztop), float(zbot)
        if not ztop <= zbot:
            raise ValueError(f'grossTransport: need ztop <= zbot, got {ztop}, {zbot}')
        if numpy.shape(bounds_depth) != (P.shape[1], 2):
            raise ValueError(f'grossTransport: bounds_depth must have shape {(P.shape[1], 2)}, got {numpy.shape(bounds_depth)}')
        return numpy.stack([_band_sum(P[0], bounds_depth, ztop, zbot), _band_sum(P[1], bounds_depth, ztop, zbot)])

    @staticmethod
    def transportWeightedTracer(volumeParts, carriedParts, reference=0.0):
        """Transport-weighted mean tracer of the inflow and of the outflow: carried / volume + reference per direction, from
        the volume parts and the carried parts (computeGrossProfile or computeGrossClassTransport with carry=False and
        carry=True, or their grossTransport sums) of one shape (2, ...); `reference`: the reference of setTracer, which the carried parts have subtracted.  NaN
        where the volume part is 0.  It ASSUMES that the tracer is present wherever the velocity is: a face with a velocity
        and no tracer value adds to the volume part and nothing to the carried part, and pulls the mean towards the
        reference."""
        V = numpy.asarray(volumeParts, dtype=numpy.float64)
        C = numpy.asarray(carriedParts, dtype=numpy.float64)
        if V.shape != C.shape or V.shape[:1] != (2,):
            raise ValueError(f'transportWeightedTracer: need two arrays of one shape (2, ...), got {V.shape}, {C.shape}')
        with numpy.errstate(divide='ignore', invalid='ignore'):
            return numpy.where(V != 0.0, C / V + float(reference), numpy.nan)

    @staticmethod
    def overturningGyre(volumeProfile, areaRows, tracerRow):
        """Split a tracer transport into its throughflow, overturning and gyre parts.  Host only, float64, on rows that have
        been summed over all ranks first (the step is not linear).  volumeProfile: V (nz, n) of computeFluxProfile;
        areaRows: the pair (A, T), each (nz, n), of computeAreaProfile; tracerRow: H (n,) of computeTracerFlux -- totals or
        segments alike; the rows may be classes instead of levels: V of computeClassTransport, (A, B) of computeClassArea
        (decomposeTracerTransportByClass).  Per column, with m(z) = T(z) / A(z) (0 where A(z) = 0) and M = sum_z T / sum_z A (0 where the sum is 0):
            throughflow = (sum_z V(z)) * M,   overturning = sum_z V(z) * (m(z) - M),   gyre = H - throughflow - overturning.
        Returns a dict of 'total' (= H), 'throughflow', 'overturning', 'gyre', each (n,), and 'mean' = m, (nz, n)."""
        V = numpy.asarray(volumeProfile, dtype=numpy.float64)
        A, T = (numpy.asarray(x, dtype=numpy.float64) for x in areaRows)
        H = numpy.asarray(tracerRow, dtype=numpy.float64)
        if V.ndim != 2 or A.shape != V.shape or T.shape != V.shape or H.shape != V.shape[1:]:
            raise ValueError(f'overturningGyre: need V, A, T of one shape (nz, n) and H of shape (n,), got {V.shape}, {A.shape}, '
                             f'{T.shape}, {H.shape}')
        with numpy.errstate(divide='ignore', invalid='ignore'):
            m = numpy.where(A != 0.0, T / A, 0.0)
            sA, sT = A.sum(axis=0), T.sum(axis=0)
            M = numpy.where(sA != 0.0, sT / sA, 0.0)
        through = V.sum(axis=0) * M
        over = (V * (m - M)).sum(axis=0)
        return dict(total=H, throughflow=through, overturning=over, gyre=H - through - over, mean=m)

    def decomposeTracerTransport(self, tIndex):
        """The tracer transport of time step tIndex (setTracer first) and its throughflow, overturning and gyre parts, for
        the transect totals: computeFluxProfile, computeAreaProfile and computeTracerFlux, then overturningGyre.  On one rank
        only; sharded runs reduce the rows first (docs/MULTIGPU.md)."""
        V = self.computeFluxProfile(tIndex)[0]
        (A, _), (T, _) = self.computeAreaProfile(tIndex)
        H = self.computeTracerFlux(tIndex)[0]
        return self.overturningGyre(V, (A, T), H)

    # ------------------------------------------------------------------------------------------
    _MEAN_STAGE_BYTES = 256 << 20     # host arrays go to the GPU in groups of steps of at most this many bytes

    def _step_range(self, steps):
        t0, t1 = (0, self.nt) if steps is None else (int(steps[0]), int(steps[1]))
        if not 0 <= t0 < t1 <= self.nt:
            raise RuntimeError(f'ERROR: steps must be None or a half-open (t0, t1) with 0 <= t0 < t1 <= {self.nt}, got {steps}')
        return t0, t1

    def _step_table(self, what, steps, select, weights):
        """The steps a time mean visits and their weights: (list of ascending step indices, float64 weights or None for all 1,
        the float64 sum of the weights added in order).  steps: None or a half-open (t0, t1); select: a strictly ascending
        sequence of step indices, instead of steps; weights: one positive finite number per visited step, or 'bounds' for the
        step lengths of the file's time bounds (TimeObj.getStepLengths)."""
        if select is not None:
            if steps is not None:
                raise RuntimeError(f'ERROR: {what}: give steps or select, not both')
            idx = [int(t) for t in select]
            if [float(t) for t in idx] != [float(t) for t in select]:
                raise RuntimeError(f'ERROR: {what}: select must hold whole step indices, got {list(select)}')
            if not idx or idx[0] < 0 or idx[-1] >= self.nt or any(b <= a for a, b in zip(idx, idx[1:])):
                raise RuntimeError(f'ERROR: {what}: select must be a strictly ascending sequence of step indices in '
                                   f'[0, {self.nt}), got {idx}')
        else:
            idx = list(range(*self._step_range(steps)))
        if weights is None:
            return idx, None, float(len(idx))
        if isinstance(weights, str):
            if weights != 'bounds':
                raise RuntimeError(f"ERROR: {what}: weights must be numbers or 'bounds', got '{weights}'")
            lengths = getattr(self.timeObj, 'getStepLengths', lambda: None)()
            if lengths is None or len(lengths) != self.nt:
                name = getattr(self.timeObj, 'timeVarName', '') or 'none found'
                raise RuntimeError(f"ERROR: {what}: weights='bounds' needs the bounds of the time variable ({name}): its "
                                   f'`bounds` attribute must name a (nt, 2) variable of the U file')
            w = numpy.asarray(lengths, dtype=numpy.float64)[idx]
        else:
            w = numpy.array(weights, dtype=numpy.float64).reshape(-1)
            if w.size != len(idx):
                raise RuntimeError(f'ERROR: {what}: {w.size} weights for {len(idx)} steps')
        if not (numpy.isfinite(w).all() and (w > 0).all()):
            raise RuntimeError(f'ERROR: {what}: every weight must be finite and > 0, got {w.tolist()}')
        total = numpy.float64(0.0)
        for x in w:
            total = total + x
        return idx, numpy.ascontiguousarray(w), float(total)

    def _time_mean_groups(self, series, markers, idx, nacc, contiguous, carry_wsum, call):
        """The steps idx (ascending) of a list of (nt, nz, ny, nx) arrays of one dtype, each in any of its homes (HBM, host,
        file-backed, derived), in groups through one of the time-mean kernels into `nacc` float64 torch CUDA tensors
        (1, nz, ny, nx).  call(accs, wsum, cnt, ptrs, offsets, j0, k, n, code, size, fill, missing, first, last, fill_out) makes
        the C call for the k steps idx[j0:j0 + k]: series j's steps are at the element offsets offsets[j] (int64, ascending)
        from the HBM address ptrs[j]; fill / missing: `markers` without NaN.  All in HBM: one call on the offsets idx * n,
        nothing carried.  Host arrays: groups of steps within _MEAN_STAGE_BYTES for all the series together, packed into
        staging buffers -- a group in one copy when idx is `contiguous`, else step by step.  File-backed or derived: one
        step at a time; a step that is not in idx is never read.  carry_wsum: the kernel carries a sum of weights
        (NF_MEAN_OVER_PRESENT).  Returns the tensors and fill_out -- the first marker as the dtype of the arrays holds it, NaN
        without one -- which stands where the value is missing at every step.  The bits do not depend on the homes or on the
        grouping of the steps."""
        import torch
        dt = numpy.dtype(_native_dtype(series[0]))
        code, size = (NF_F32 if dt == numpy.float32 else NF_F64), dt.itemsize
        marks = [float(m) for m in markers if m == m]
        with numpy.errstate(over='ignore'):
            fill_out = float(dt.type(marks[0])) if marks else numpy.nan
        fill, missing = (marks + [numpy.nan, numpy.nan])[:2]
        n = self.nz * self.ny * self.nx
        accs = [torch.empty((1, self.nz, self.ny, self.nx), dtype=torch.float64, device='cuda') for _ in range(nacc)]
        ptrs = [_lib.device_pointer(x) for x in series]
        staged = [p is None for p in ptrs]

        def run(cur, offsets, j0, k, wsum=None, cnt=None):
            call([x.data_ptr() for x in accs], None if wsum is None else wsum.data_ptr(), None if cnt is None else cnt.data_ptr(),
                 cur, [numpy.ascontiguousarray(o, dtype=numpy.int64) for o in offsets], j0, k, n, code, size, fill, missing,
                 1 if j0 == 0 else 0, 1 if j0 + k == len(idx) else 0, fill_out)

        everywhere = numpy.array(idx, dtype=numpy.int64) * n
        if not any(staged):       # all in HBM: one pass, nothing carried
            run(ptrs, [everywhere] * len(series), 0, len(idx))
        else:
            cnt = torch.empty(n, dtype=torch.int32, device='cuda')
            wsum = torch.empty(n, dtype=torch.float64, device='cuda') if carry_wsum else None
            lazy = [hasattr(x, 'read_step') for x in series]
            derived = [hasattr(x, 'compute_step') for x in series]     # a derived cell thickness: one step at a time too
            group = 1 if any(lazy) or any(derived) else max(1, self._MEAN_STAGE_BYTES // (sum(staged) * n * size))
            bufs = [self._host_array((self.nz, self.ny, self.nx), dt) if z else None for z in lazy]
            hosts = [_native(x).reshape(self.nt, n) if st and not z and not d else None
                     for x, st, z, d in zip(series, staged, lazy, derived)]
            stage = [_lib.DeviceBuffer(min(group, len(idx)) * n * size) if st else None for st in staged]
            for j0 in range(0, len(idx), group):
                k = min(group, len(idx) - j0)
                cur, offsets = [], []
                for j in range(len(series)):
                    if not staged[j]:
                        cur.append(ptrs[j])
                        offsets.append(everywhere[j0:j0 + k])
                        continue
                    # the steps of this group, packed; (first packed step, number of steps) of every copy
                    for m, c in [(0, k)] if contiguous and hosts[j] is not None else [(m, 1) for m in range(k)]:
                        t, dst = idx[j0 + m], stage[j].ptr + m * n * size
                        if derived[j]:      # computed straight into the staging buffer
                            series[j].compute_step(t, dst)
                            continue
                        if lazy[j]:
                            series[j].read_step(t, out=bufs[j])
                        check(lib.nf_memcpy_h2d(dst, bufs[j].ctypes.data if lazy[j] else hosts[j][t:t + c].ctypes.data,
                                                c * n * size))
                    cur.append(stage[j].ptr)
                    offsets.append(numpy.arange(k, dtype=numpy.int64) * n)
                run(cur, offsets, j0, k, wsum, cnt)
                check(lib.nf_synchronize())     # the staging buffers are written again by the next group
            for b in stage:
                if b is not None:
                    b.free()
        check(lib.nf_synchronize())
        return accs, fill_out

    def _time_mean_walk_table(self, series, markers, table, nacc, kernel, carry_wsum):
        """_time_mean_groups over a table (_step_table) of selected, weighted steps.  kernel(accs, wsum, cnt, ptrs, offsets,
        weights, nsteps, n, code, fill, missing, first, last, total_weight, fill_out) makes the C call for nsteps table entries:
        series j's steps at the element offsets offsets[j] (int64) from the HBM address ptrs[j]."""
        idx, w, total = table

        def call(accs, wsum, cnt, ptrs, offsets, j0, k, n, code, size, fill, missing, first, last, fill_out):
            kernel(accs, wsum, cnt, ptrs, offsets, None if w is None else w[j0:j0 + k], k, n, code, fill, missing, first, last,
                   total, fill_out)

        return self._time_mean_groups(series, markers, idx, nacc, False, carry_wsum, call)

    def _time_mean_walk(self, series, markers, t0, t1, nacc, kernel):
        """_time_mean_groups over the steps [t0, t1).  kernel(accs, cnt, ptrs, nsteps, n, code, fill, missing, first, last,
        total_steps, fill_out) makes the C call for nsteps steps that begin at the HBM addresses ptrs (one per series).  The
        selected, weighted form of the walk is _time_mean_walk_table."""
        def call(accs, wsum, cnt, ptrs, offsets, j0, k, n, code, size, fill, missing, first, last, fill_out):
            kernel(accs, cnt, [p + int(o[0]) * size for p, o in zip(ptrs, offsets)], k, n, code, fill, missing, first, last,
                   t1 - t0, fill_out)

        return self._time_mean_groups(series, markers, list(range(t0, t1)), nacc, True, False, call)

    def _time_mean_array(self, a, markers, rule, t0, t1, table=None):
        """The mean over the steps [t0, t1) of a (nt, nz, ny, nx) array in any of its three homes, by nf_time_mean: a float64
        torch CUDA tensor (1, nz, ny, nx) and its fill (_time_mean_walk).  table (_step_table) instead of t0, t1: the mean over
        its selected, weighted steps by nf_time_mean_steps (_time_mean_walk_table)."""
        if table is not None:
            def steps_kernel(accs, wsum, cnt, ptrs, offsets, w, nsteps, n, code, fill, missing, first, last, total, fill_out):
                check(lib.nf_time_mean_steps(accs[0], wsum, cnt, ptrs[0], offsets[0].ctypes.data_as(_lib.c_ll_p),
                                             None if w is None else _lib.dptr(w), nsteps, n, code, fill, missing, first, last,
                                             rule, total, fill_out, None))

            (acc,), fill_out = self._time_mean_walk_table([a], markers, table, 1, steps_kernel, rule == _lib.NF_MEAN_OVER_PRESENT)
            return acc, fill_out

        def kernel(accs, cnt, ptrs, nsteps, n, code, fill, missing, first, last, total, fill_out):
            check(lib.nf_time_mean(accs[0], cnt, ptrs[0], nsteps, n, n, code, fill, missing, first, last, rule, total, fill_out,
                                   None))

        (acc,), fill_out = self._time_mean_walk([a], markers, t0, t1, 1, kernel)
        return acc, fill_out

    def _time_mean_weighted_arrays(self, a, markers, thk, thk_markers, t0, t1, table=None):
        """The thickness-weighted mean over the steps [t0, t1) of the (nt, nz, ny, nx) velocity `a` and the mean of the
        thickness `thk` at its points, by nf_time_mean_weighted; each of the two in any of the three homes.  Returns two
        float64 torch CUDA tensors (1, nz, ny, nx) and the fill of the first (_time_mean_walk).  table (_step_table) instead
        of t0, t1: over its selected, weighted steps by nf_time_mean_weighted_steps (_time_mean_walk_table)."""
        dt = numpy.dtype(_native_dtype(a))
        if numpy.dtype(_native_dtype(thk)) != dt:
            raise RuntimeError(f'ERROR: timeMean: the cell thickness is {numpy.dtype(_native_dtype(thk)).name}, uo/vo are {dt.name}')
        if table is not None:
            def steps_kernel(accs, wsum, cnt, ptrs, offsets, w, nsteps, n, code, fill, missing, first, last, total, fill_out):
                check(lib.nf_time_mean_weighted_steps(accs[0], accs[1], cnt, ptrs[0], offsets[0].ctypes.data_as(_lib.c_ll_p),
                                                      ptrs[1], offsets[1].ctypes.data_as(_lib.c_ll_p),
                                                      None if w is None else _lib.dptr(w), nsteps, n, code, fill, missing,
                                                      float(thk_markers[0]), float(thk_markers[1]), first, last, total,
                                                      fill_out, None))

            (accf, acch), fill_out = self._time_mean_walk_table([a, thk], markers, table, 2, steps_kernel, False)
            return accf, acch, fill_out

        def kernel(accs, cnt, ptrs, nsteps, n, code, fill, missing, first, last, total, fill_out):
            check(lib.nf_time_mean_weighted(accs[0], accs[1], cnt, ptrs[0], n, ptrs[1], n, nsteps, n, code, fill, missing,
                                            float(thk_markers[0]), float(thk_markers[1]), first, last, total, fill_out, None))

        (accf, acch), fill_out = self._time_mean_walk([a, thk], markers, t0, t1, 2, kernel)
        return accf, acch, fill_out

    def timeMean(self, steps=None, thicknessWeighted=False, select=None, weights=None):
        """The mean state of the steps [t0, t1) (steps=None: all of them) as a new Field with nt = 1 and float64 fields in HBM,
        built through fromArrays from the same bounds, deptht_bounds, transects, sverdrup, periodX and cell policies: every
        diagnostic of the engine works on it unchanged.  uo / vo: sum over the steps of the present values / number of steps
        (a missing velocity counts as 0, as in every flux kernel, so the volume flux of the mean state is the mean of the
        volume fluxes); a value missing at every step is the new Field's fill, the source's first marker as its dtype holds it
        (NaN without one).  A tracer of setTracer / setClassTracer: the mean of its present values, set on the new Field with
        the same reference and wrapX; the class edges and the depth edges are carried over.  A static cell thickness is carried over as float64;
        a sharded Field (slab_range) raises, and so does a time-varying cell thickness unless thicknessWeighted=True;
        a Field that holds a Sigma (nemoflux_amd.eos) raises too.  The sums
        are float64, left to right in step order (nf_time_mean), wherever the arrays live: HBM (one pass), host (uploaded in
        groups of steps) or files (one step at a time).  Nothing of this Field changes.
        thicknessWeighted=True (setCellThickness first): the mean state of z* / variable-volume output.  With a time-varying
        thickness the velocities are the thickness-weighted means <e3u uo> / <e3u>, <e3v vo> / <e3v> (nf_time_mean_weighted:
        a missing velocity adds nothing to the numerator, a thickness that is NaN or a marker counts as 0, a velocity missing
        at every step is the fill, 0 where the thickness sums to 0), and the new Field gets the mean thicknesses <e3u>, <e3v>
        as a static float64 cell thickness in HBM: (mean thickness) x (mean velocity) is the mean volume flux face by face,
        so the volume flux of the mean state is again the mean of the volume fluxes.  The tracers keep the plain mean of
        their present values (there is no e3t to weight them with).  With a static thickness the weights cancel: the result
        of timeMean(steps), bit for bit.
        select: a strictly ascending sequence of step indices instead of the range `steps` (a season of every year, a
        climatological month, everything but the spin-up); weights: one positive finite number per visited step, or 'bounds'
        for the step lengths of the file's time bounds (months of 28 to 31 days).  The sums become sum of w_j x over the visited
        steps in their order, divided by the sum of all weights (velocities, thicknesses) or of the weights of the present
        values (tracers): nf_time_mean_steps / nf_time_mean_weighted_steps, one pass over the selected steps in HBM, selected
        steps packed into the staging buffer from the host, one selected step at a time from files -- a step that is not
        selected is never read.  select without weights over a range gives timeMean(steps) of that range, bit for bit; with
        both None the code and the bits are those of before."""
        self._sigma_refused('timeMean')
        if self.slab_range is not None:
            raise RuntimeError('ERROR: timeMean: the mean state of a sharded Field (slab_range) is not defined here; build the '
                               'Field without slab_range')
        e3 = getattr(self, '_e3', None)
        if thicknessWeighted and e3 is None:
            raise RuntimeError('ERROR: timeMean: thicknessWeighted=True needs a cell thickness; call setCellThickness first')
        weighted = bool(thicknessWeighted) and e3['nt'] != 1
        if e3 is not None and e3['nt'] != 1 and not weighted:
            raise RuntimeError('ERROR: timeMean: the mean state of a time-varying cell thickness is not defined here (it would '
                               'need thickness-weighted means); set a static thickness or none')
        if select is None and weights is None:
            (t0, t1), table = self._step_range(steps), None
        else:
            t0 = t1 = None
            table = self._step_table('timeMean', steps, select, weights)
        if weighted:
            thk_markers = (e3['fill'], e3['missing'])
            u, hu, fill = self._time_mean_weighted_arrays(self._uv[0], self._uv_markers, e3['arrays'][0], thk_markers, t0, t1, table)
            v, hv, _ = self._time_mean_weighted_arrays(self._uv[1], self._uv_markers, e3['arrays'][1], thk_markers, t0, t1, table)
        else:
            u, fill = self._time_mean_array(self._uv[0], self._uv_markers, _lib.NF_MEAN_OVER_STEPS, t0, t1, table)
            v, _ = self._time_mean_array(self._uv[1], self._uv_markers, _lib.NF_MEAN_OVER_STEPS, t0, t1, table)
        mean = Field.fromArrays(self._bounds[0], self._bounds[1], self.bounds_depth, u, v, self._polylines, self.sverdrup,
                                fill_value=fill, **self._build_kw)

        def none_if_nan(x):
            return None if x != x else x

        tr = getattr(self, '_tracer', None)
        if tr is not None:
            tau, tfill = self._time_mean_array(tr['keep'], (tr['fill'], tr['missing']), _lib.NF_MEAN_OVER_PRESENT, t0, t1, table)
            mean.setTracer(tau, fill_value=none_if_nan(tfill), reference=self._tracer_reference, wrapX=self._tracer_wrapX)
        ct = getattr(self, '_class_tracer', None)
        if ct is not None:
            sig, sfill = self._time_mean_array(ct['keep'], (ct['fill'], ct['missing']), _lib.NF_MEAN_OVER_PRESENT, t0, t1, table)
            mean.setClassTracer(sig, fill_value=none_if_nan(sfill))
        if getattr(self, '_class_edges', None) is not None:
            mean.setClassEdges(self._class_edges)
        if getattr(self, '_joint_edges', None) is not None:
            mean.setJointClassEdges(*self._joint_edges)
        if getattr(self, '_depth_edges', None) is not None:
            mean.setDepthEdges(*self._depth_edges)
        self._mean_surfaces(mean, table, t0, t1)
        if weighted:
            mean.setCellThickness(hu, hv)       # the mean thicknesses: static, float64, in HBM, no markers
        elif e3 is not None:
            dt = self._uv_dtype
            with numpy.errstate(over='ignore'):
                marks = [none_if_nan(float(dt.type(m))) if m == m else None for m in (e3['fill'], e3['missing'])]
            mean.setCellThickness(*[self._as_float64(x) for x in e3['arrays']], fill_value=marks[0], missing_value=marks[1])
        return mean

    @staticmethod
    def _as_float64(a):
        """a static thickness as float64, where it lives"""
        import torch
        if isinstance(a, torch.Tensor):
            return a.to(torch.float64)
        if isinstance(a, _lib.DeviceArray):
            if a.dtype == numpy.float64:
                return a
            host = numpy.empty(a.shape, a.dtype)
            check(lib.nf_memcpy_d2h(host.ctypes.data, a.ptr, host.nbytes))
            a = host
        return numpy.ascontiguousarray(a, dtype=numpy.float64)

    _SPLIT_METHODS = ('computeTracerFlux', 'computeFluxProfile', 'computeTracerProfile', 'computeClassTransport',
                      'computeClassTracerTransport', 'computeClassRemap', 'computeDepthTransport', 'computeGrossProfile',
                      'computeGrossClassTransport', 'computeGrossClassRemap', 'computeSurfaceTransport')

    def meanEddySplit(self, method, steps=None, select=None, weights=None, thicknessWeighted=False, **kw):
        """The time mean of one per-step row product split into the part of the mean state and the rest.  method: the name of
        the product -- computeTracerFlux, computeFluxProfile, computeTracerProfile, computeClassTransport,
        computeClassTracerTransport, computeClassRemap, computeDepthTransport, computeGrossProfile,
        computeGrossClassTransport, computeGrossClassRemap or computeSurfaceTransport; kw goes to it (carry=).  steps / select / weights choose and weight the steps as in
        timeMean.  Returns a dict: 'total' = sum of w_j rows_j over the visited steps / sum of w_j, formed on the host in float64
        step by step in their order; 'mean' = the same product at step 0 of 'meanField' = timeMean(steps, thicknessWeighted,
        select, weights), the transport by the mean flow of the mean tracer in the classes of the mean class field; 'eddy' =
        total - mean, what the transients carry (how much of MOC(sigma) is eddy-induced, at which depth and in which class
        the fluctuations carry the heat).  total, mean and eddy are (totals, segments) pairs shaped as the product returns them.
        The mean state and the total use the same steps and weights, so the split closes: for a product that is linear in
        (uo, vo) with everything else constant in time, eddy is rounding.  What the product refuses (a cell thickness, a
        Sigma) it refuses here with its own words."""
        if method not in self._SPLIT_METHODS:
            raise RuntimeError(f'ERROR: meanEddySplit: method must be one of {", ".join(self._SPLIT_METHODS)}, got {method!r}')
        idx, w, wtotal = self._step_table('meanEddySplit', steps, select, weights)
        call = getattr(self, method)
        lookahead = method != 'computeTracerFlux'      # the one product without prefetch_next
        total = None
        for j, t in enumerate(idx):
            if lookahead:
                rows = call(t, prefetch_next=idx[j + 1] if j + 1 < len(idx) else -1, **kw)
            else:
                rows = call(t, **kw)
            wj = numpy.float64(1.0 if w is None else w[j])
            terms = [wj * numpy.asarray(r, dtype=numpy.float64) for r in rows]
            total = terms if total is None else [a + b for a, b in zip(total, terms)]
        total = tuple(a / numpy.float64(wtotal) for a in total)
        if select is None and weights is None:
            meanField = self.timeMean(steps, thicknessWeighted)
        else:
            meanField = self.timeMean(steps, thicknessWeighted, select=select, weights=weights)
        mean = tuple(numpy.array(r, dtype=numpy.float64) for r in getattr(meanField, method)(0, **kw))
        return dict(total=total, mean=mean, eddy=tuple(a - b for a, b in zip(total, mean)), meanField=meanField)

    def meanEddyTracerTransport(self, steps=None, thicknessWeighted=False, select=None, weights=None):
        """The mean tracer transport of the steps [t0, t1) (steps=None: all; setTracer first) split in time, for the transect
        totals: 'total' = the float64 mean over the steps of the computeTracerFlux totals; 'mean' = computeTracerFlux(0) of
        timeMean(steps), the transport of the mean tracer by the mean flow; 'eddy' = total - mean, the part <u' tau'> carried
        by the correlation of the fluctuations; 'meanField' = that Field, for its profile, class and decomposition calls.
        thicknessWeighted=True (a time-varying cell thickness: z* / variable-volume output) is passed on to timeMean: 'total'
        is computed with the thickness of every step as before, 'mean' is the transport of the time-mean tracer by the
        time-mean VOLUME FLUX (mean thickness x thickness-weighted mean velocity), and 'eddy' is everything else -- the
        correlation of the tracer with the volume flux, which includes the tracer-thickness covariance, because there is no
        e3t to weight the tracer mean with.
        select / weights (timeMean): the steps of a strided or irregular selection and their weights (step lengths); this is
        then meanEddySplit('computeTracerFlux', ...) reduced to the transect totals."""
        self._sigma_refused('meanEddyTracerTransport')
        if getattr(self, '_tracer', None) is None:
            raise RuntimeError('ERROR: call setTracer first')
        if select is not None or weights is not None:
            d = self.meanEddySplit('computeTracerFlux', steps, select, weights, thicknessWeighted)
            return dict(total=d['total'][0], mean=d['mean'][0], eddy=d['eddy'][0], meanField=d['meanField'])
        t0, t1 = self._step_range(steps)
        if (t0, t1) == (0, self.nt):
            rows = self.computeTracerAll()[0]
        else:
            rows = numpy.array([self.computeTracerFlux(t)[0] for t in range(t0, t1)])
        total = numpy.asarray(rows, dtype=numpy.float64).sum(axis=0) / float(t1 - t0)
        meanField = self.timeMean(steps, thicknessWeighted)
        mean = numpy.array(meanField.computeTracerFlux(0)[0], dtype=numpy.float64)
        return dict(total=total, mean=mean, eddy=total - mean, meanField=meanField)

    def computeClassTracerTransport(self, tIndex, out=None, prefetch_next=None):
        """Transport of the tracer of setTracer (reference subtracted) of time step tIndex, binned by the class of each U / V
        face (setTracer and setClassEdges first): (nedges+2, ntransect) totals and (nedges+2, nseg) per-segment sums, rows as in
        computeClassTransport.  The class field is the tracer of setClassTracer when one is set (heat by density class), else
        the carried tracer itself (heat by temperature class).  Every per-level term of computeTracerProfile goes to the row
        of its face, so the rows add up to the computeTracerFlux row (up to rounding); a face whose carried tracer is missing
        on both sides adds nothing.  Levels this rank does not own (slab_range) contribute nothing.  Leaves everything else
        as it is.  `out`: as in computeClassTransport."""
        edges = getattr(self, '_class_edges', None)
        if edges is None:
            raise RuntimeError('ERROR: call setClassEdges first')
        rows = self._product('nf_field_compute_class_tracer_transport', tIndex, (edges.size + 2,), out=out,
                             prefetch_next=prefetch_next)
        return self._split_rows(rows)

    def setClassEdges(self, edges):
        """Class edges e[0] < ... < e[n-1] (2 <= n <= 1025, finite) for computeClassTransport and computeClassTracerTransport:
        the classes of the tracer of setTracer (potential density, temperature, salinity) -- or of setClassTracer, when one is
        set -- that the transport is binned by."""
        e = numpy.array(edges, dtype=numpy.float64).reshape(-1)
        check(lib.nf_field_set_class_edges(ctypes.byref(self._h), _lib.dptr(e), int(e.size)))
        self._class_edges = e

    def computeClassTransport(self, tIndex, out=None, prefetch_next=None):
        """Volume transport of time step tIndex binned by the class of the tracer at each U / V face (setTracer and
        setClassEdges first): (nedges+2, ntransect) totals and (nedges+2, nseg) per-segment sums.  Row 0: class value
        x < e[0]; row k: e[k-1] <= x < e[k]; row nedges: x >= e[nedges-1]; row nedges+1: faces without a class value (the
        tracer missing on both sides).  The class field is the tracer of setClassTracer when one is set, else the tracer of
        setTracer.  The class value of a face is the mean of the class field in the two cells beside it (the
        present one when only one has a value); the tracer's reference is NOT used for it.  Every per-level term of
        computeFluxProfile goes to the row of its face, so the rows add up to the computeFlux row (up to rounding).  Levels
        this rank does not own (slab_range) contribute nothing.  Leaves the resident edge fluxes, the running max, the row of
        the last computeFlux and the tracer rows as they are.  `out`: optional contiguous float64 torch CUDA tensor
        (nedges+2, row_length) that receives the raw rows in HBM (for nemoflux_amd.dist.reduce_rows)."""
        edges = getattr(self, '_class_edges', None)
        if edges is None:
            raise RuntimeError('ERROR: call setClassEdges first')
        rows = self._product('nf_field_compute_class_transport', tIndex, (edges.size + 2,), out=out,
                             prefetch_next=prefetch_next)
        return self._split_rows(rows)

    def computeClassRemap(self, tIndex, carry=False, out=None, prefetch_next=None):
        """Class transport of time step tIndex by conservative (piecewise-linear) remapping (setTracer and setClassEdges
        first): (nedges+2, ntransect) totals and (nedges+2, nseg) per-segment sums, rows, class field and terms as in
        computeClassTransport (carry=False) or computeClassTracerTransport (carry=True).  Instead of going whole to the class
        of its face, a level's term is spread uniformly in class space over the interval between the class field's values
        at the layer's upper and lower interface -- the mean of the face's values at this level and at the level above /
        below, the level's own value where there is no such level or the face has no value there -- and every class gets the
        share of the interval that lies in it: xgcm's transform(method='conservative').  With many class edges and few levels
        the rows are then a smooth function of the class instead of a comb.  The rows add up to those of the step rule; a
        layer that lies inside one class goes to it whole; a face without a class value goes to row nedges+1; a non-finite
        interface value falls back to the step rule for that term.  Levels this rank does not own (slab_range) contribute
        nothing, but the class field is read one level beyond them.  The rows go into classStreamfunction and timeMean
        Fields as those of the step forms do.  Raises while a cell thickness is set.  Leaves everything else as it is.
        `out`: as in computeClassTransport."""
        edges = getattr(self, '_class_edges', None)
        if edges is None:
            raise RuntimeError('ERROR: call setClassEdges first')
        rows = self._product('nf_field_compute_class_remap', tIndex, (edges.size + 2,), carry=bool(carry), out=out,
                             prefetch_next=prefetch_next)
        return self._split_rows(rows)

    def setDepthEdges(self, edges, top=0.0):
        """Depth edges e[0] < ... < e[n-1] (2 <= n <= 1025, finite; the units of the thicknesses) for computeDepthTransport,
        and `top`, the depth of the upper interface of level 0 (finite).  A set of its own: setClassEdges and
        setJointClassEdges do not see it."""
        e = numpy.array(edges, dtype=numpy.float64).reshape(-1)
        check(lib.nf_field_set_depth_edges(ctypes.byref(self._h), _lib.dptr(e), int(e.size), float(top)))
        self._depth_edges = (e, float(top))

    def computeDepthTransport(self, tIndex, carry=False, out=None, prefetch_next=None):
        """Transport of time step tIndex in true-depth bins (setDepthEdges first): (nedges+2, ntransect) totals and
        (nedges+2, nseg) per-segment sums.  Row 0: depth < e[0]; row k: e[k-1] <= depth < e[k]; row nedges: depth >=
        e[nedges-1]; row nedges+1: terms of a face whose interface depth is not finite (exactly +0.0 otherwise).  Every
        per-level term of computeFluxProfile (carry=True, setTracer first: of computeTracerProfile -- and with a cell
        thickness, which that call refuses, the same term with the thickness at the face) is spread uniformly in depth over
        the layer at its own face, [D_z, D_z+1] with D_0 = top and D_z+1 = D_z + h_z: h_z is the cell thickness at the face
        when one is set (setCellThickness: partial steps, z*, terrain-following levels), else thickness[z]; every bin gets
        the share of the layer that lies in it.  The rows add up to the sum over z of the profile rows (up to rounding);
        with the per-level thickness and edges at the level interfaces they are the profile rows bit for bit.  Levels this
        rank does not own (slab_range) contribute nothing, but the depths are summed from level 0: the thickness is read
        above the owned levels too.  The rows go into classStreamfunction as they are: the overturning streamfunction in
        depth.  Leaves everything else as it is.  `out`: as in computeClassTransport."""
        edges = getattr(self, '_depth_edges', None)
        if edges is None:
            raise RuntimeError('ERROR: call setDepthEdges first')
        rows = self._product('nf_field_compute_depth_transport', tIndex, (edges[0].size + 2,), carry=bool(carry),
                             tracer=carry, out=out, prefetch_next=prefetch_next)
        return self._split_rows(rows)

    def setDepthSurfaces(self, surfaces, top=0.0, fill_value=None, missing_value=None, wrapX=True):
        """Surfaces that bound the layers of computeSurfaceTransport: a list of 1 to 8 fields at T-points whose values are
        depths, positive downward, in the units of the thicknesses and measured from the origin of `top`, the depth of the
        upper interface of level 0 (finite) -- the mixed-layer depth, the depth of an isotherm, an ice-shelf draft, the column
        depth minus 200.  Each item is a host array of shape (ny, nx), (1, ny, nx) (static) or (nt, ny, nx), a torch CUDA
        tensor or a DeviceArray of such a shape (used in place), or a (path, name) pair read with nemoflux_amd.io, its CF
        markers decoded: a time-varying one, one step at a time.  All items are static or all vary in time, and all live on the
        host (files included) or all on the device.  A host array of another float dtype is cast to the dtype of uo / vo; a
        device array of another dtype raises.  fill_value / missing_value: the surfaces' own missing markers (the files' when
        not given; more than two distinct ones over the set raise); NaN always counts as missing.  wrapX: the east face of
        the last column takes column 0 as its neighbour.  A set of its own: setDepthEdges, setClassEdges and
        setJointClassEdges do not see it.  setDepthSurfaces(None) clears it.
        An item may also be a nemoflux_amd.surfaces.IsoDepth or MixedLayerDepth: surfaces derived on the GPU from a tracer --
        the depth of an isotherm or an isopycnal, the mixed-layer depth -- one time step at a time (nf_iso_depth).  Such an
        item counts as its number of values towards the limit of 8, varies in time and lives on the device: it may stand
        beside device arrays of (nt, ny, nx).  Its planes carry NaN where a column has no wet level."""
        from .surfaces import IsoDepth
        self._surfaces = None
        if surfaces is None:
            check(lib.nf_field_set_depth_surfaces(ctypes.byref(self._h), None, 0, 0, NF_F64, 0, numpy.nan, 0.0))
            return
        surfaces = list(surfaces)
        count = sum(s.m if isinstance(s, IsoDepth) else 1 for s in surfaces)
        if not 1 <= count <= 8:
            raise RuntimeError(f'ERROR: setDepthSurfaces needs a list of 1 to 8 surfaces, got {count}')
        if not numpy.isfinite(float(top)):
            raise RuntimeError(f'ERROR: setDepthSurfaces: top must be a finite number, got {top!r}')
        uv_dtype = self._uv_dtype
        markers, items, nts, homes, derived = [], [], [], [], []
        for k, s in enumerate(surfaces):
            if isinstance(s, IsoDepth):
                item = self._derived_surface(k, s, float(top))
                derived.append(item)
                for j in range(s.m):
                    items.append(_DerivedPlane(item, j))
                    nts.append(self.nt)
                    homes.append(True)
                continue
            s, own = _open_pair(s)
            for m in own:
                if m not in markers:
                    markers.append(m)
            shape = tuple(int(x) for x in s.shape)
            nt_s = 1 if len(shape) == 2 else (shape[0] if len(shape) == 3 else -1)
            if shape[-2:] != (self.ny, self.nx) or nt_s not in (1, self.nt):
                raise RuntimeError(f'ERROR: surface {k} has shape {shape}; need (ny, nx) = {(self.ny, self.nx)}, (1, ny, nx) or '
                                   f'(nt, ny, nx) = {(self.nt, self.ny, self.nx)}')
            if hasattr(s, 'read_step') and (nt_s == 1 or len(shape) == 2):     # a static file variable: read once
                s = numpy.stack([s.read_step(j) for j in range(shape[0])]) if len(shape) == 2 else s.read_step(0)
            dt, ptr, lazy = numpy.dtype(_native_dtype(s)), _lib.device_pointer(s), hasattr(s, 'read_step')
            if ptr is not None and dt != uv_dtype:
                raise RuntimeError(f'ERROR: surface {k} is {dt.name}, uo/vo are {uv_dtype.name}: only a host array of another '
                                   f'float dtype is cast')
            if dt.kind != 'f':
                raise RuntimeError(f'ERROR: surface {k} is {dt.name}: need a float array')
            if ptr is None and not lazy:
                s = _native(numpy.asarray(s, dtype=uv_dtype))
            items.append(s)
            nts.append(nt_s)
            homes.append(ptr is not None)
        if len(set(nts)) > 1:
            raise RuntimeError(f'ERROR: setDepthSurfaces: the surfaces have {nts} time steps: all static or all per time step')
        if len(set(homes)) > 1:
            raise RuntimeError('ERROR: setDepthSurfaces: the surfaces must all be host arrays (or files) or all be device arrays')
        fill, missing = _two_markers(markers, fill_value, missing_value, 'the surfaces carry', merge=True)
        slot = dict(items=items, nt=nts[0], on_dev=homes[0], step=-1, stage=None, top=float(top), wrapX=bool(wrapX), fill=fill,
                    missing=missing, derived=derived)
        bufs = [self._host_array((self.ny, self.nx), uv_dtype) if hasattr(s, 'read_step') else None for s in items]
        plane = self.ny * self.nx * uv_dtype.itemsize

        def stage_derived(t):
            """every IsoDepth computed into its buffer: its planes and the plain device arrays through a virtual (nt, ny, nx)
            base that the engine dereferences at step t"""
            for item in derived:
                item.run(t, item.out.ptr)
            return [s.item.out.ptr + (s.index - t) * plane if isinstance(s, _DerivedPlane) else _lib.device_pointer(s)
                    for s in items]

        def stage_files(t):
            """each file-backed surface into its pinned buffer, handed over through a virtual (nt, ny, nx) base"""
            for s, buf in zip(items, bufs):
                if buf is not None:
                    numpy.copyto(buf, s.read_step(t), casting='same_kind')
            return [s.ctypes.data if buf is None else buf.ctypes.data - t * plane for s, buf in zip(items, bufs)]

        if derived:
            slot['stage'] = stage_derived
        elif any(b is not None for b in bufs):
            slot['stage'] = stage_files
        else:
            self._set_surfaces(slot, [_lib.device_pointer(s) if slot['on_dev'] else s.ctypes.data for s in items])
        check(lib.nf_field_set_depth_surfaces_missing_value(ctypes.byref(self._h), missing))
        check(lib.nf_field_set_depth_surfaces_wrap(ctypes.byref(self._h), 1 if wrapX else 0))
        self._surfaces = slot

    def _set_surfaces(self, slot, ptrs):
        arr = (ctypes.c_void_p * len(ptrs))(*ptrs)
        check(lib.nf_field_set_depth_surfaces(ctypes.byref(self._h), arr, len(ptrs), slot['nt'], self._uv_code,
                                              1 if slot['on_dev'] else 0, slot['fill'], slot['top']))

    def _stage_surfaces(self, tIndex):
        """make step tIndex of surfaces that need work at every step (file-backed, derived) the one the engine reads"""
        slot = self._surfaces
        if slot.get('stage') is not None and slot['step'] != tIndex:
            self._set_surfaces(slot, slot['stage'](tIndex))
            slot['step'] = tIndex

    def _derived_surface(self, k, iso, top):
        """the producer of item k of setDepthSurfaces, an IsoDepth, once its tracer (or the thetao and so of its Sigma) and its
        e3t are found to fit this Field"""
        from .eos import Sigma
        uv_dtype = self._uv_dtype
        full = (self.nt, self.nz, self.ny, self.nx)
        sigma = isinstance(iso.tracer, Sigma)
        if not sigma:
            if self.getSizes(iso.shape) != full or len(iso.shape) not in (3, 4):
                raise RuntimeError(f'ERROR: surface {k}: the tracer of the IsoDepth has shape {iso.shape}; uo/vo have '
                                   f'(nt, nz, ny, nx) = {full}')
            if iso.dtype != uv_dtype:
                raise RuntimeError(f'ERROR: surface {k}: the tracer of the IsoDepth is {iso.dtype.name}, uo/vo are '
                                   f'{uv_dtype.name}')
        nt_e = None
        if iso.e3t is None and self.nz > 256:
            raise RuntimeError(f'ERROR: surface {k}: an IsoDepth without e3t uses the per-level thickness, which nf_iso_depth '
                               f'takes for at most 256 levels; this Field has {self.nz}: give e3t=')
        if iso.e3t is not None:
            shape = tuple(int(x) for x in iso.e3t.shape)
            nt_e = self.getSizes(shape)[0] if len(shape) in (3, 4) else -1
            if len(shape) not in (3, 4) or self.getSizes(shape)[1:] != full[1:] or nt_e not in (1, self.nt):
                raise RuntimeError(f'ERROR: surface {k}: the e3t of the IsoDepth has shape {shape}; need (nz, ny, nx) = '
                                   f'{full[1:]}, (1, nz, ny, nx) or (nt, nz, ny, nx) = {full}')
            dt = numpy.dtype(_native_dtype(iso.e3t))
            if dt != uv_dtype:
                raise RuntimeError(f'ERROR: surface {k}: the e3t of the IsoDepth is {dt.name}, uo/vo are {uv_dtype.name}')
        if sigma:
            self._check_sigma(iso.tracer, f'the Sigma of surface {k}')
        return IsoDepthProducer(self._layout(), iso, nt_e, self.thickness, top)      # everything fits: the buffers

    def getDepthSurfaces(self, tIndex):
        """The surfaces of setDepthSurfaces in force at time step tIndex as a host array (m, ny, nx) in the dtype of uo / vo,
        derived (IsoDepth, MixedLayerDepth: computed on the GPU for that step) or plain -- the mixed-layer depth that a section
        plot draws over the crossings.  Missing values are as the surfaces hold them; a derived surface has NaN where a column
        has no wet level."""
        slot = getattr(self, '_surfaces', None)
        if slot is None:
            raise RuntimeError('ERROR: call setDepthSurfaces first')
        tIndex = int(tIndex)
        if not 0 <= tIndex < self.nt:
            raise RuntimeError(f'ERROR: getDepthSurfaces: tIndex must be 0 .. {self.nt - 1}, got {tIndex}')
        uv_dtype = self._uv_dtype
        t = tIndex if slot['nt'] > 1 else 0
        return numpy.stack([numpy.asarray(self._surface_step_host(s, t), dtype=uv_dtype).reshape(self.ny, self.nx)
                            for s in slot['items']])

    def _derived_host(self, item, t):
        """the planes (m, ny, nx) of one derived item at step t on the host; the last step asked for is kept"""
        if item.host is None or item.host[0] != t:
            item.run(t, item.out.ptr)
            self._surfaces['step'] = -1       # the item's buffer no longer holds the step the engine was given
            check(lib.nf_synchronize())
            item.host = (t, item.out.download((item.iso.m, self.ny, self.nx), self._uv_dtype))
        return item.host[1]

    def _surface_step_host(self, s, t):
        """step t of one surface as a host array (ny, nx)"""
        import torch
        if isinstance(s, _DerivedPlane):
            return self._derived_host(s.item, t)[s.index]
        if hasattr(s, 'read_step'):
            return numpy.asarray(s.read_step(t))
        if isinstance(s, torch.Tensor):
            return s.reshape(-1, self.ny, self.nx)[t].cpu().numpy()
        if isinstance(s, _lib.DeviceArray):
            host = numpy.empty((self.ny, self.nx), s.dtype)
            check(lib.nf_memcpy_d2h(host.ctypes.data, s.ptr + t * host.nbytes, host.nbytes))
            return host
        return s.reshape(-1, self.ny, self.nx)[t]

    def _mean_surfaces(self, mean, table, t0, t1):
        """carry the surfaces to the Field of timeMean: a static set as it is (float64, where it lives), a time-varying one
        as the mean of its present values over the visited steps with their weights -- the tracer rule of timeMean: sum of
        w_j x over the steps where x is present / the sum of those w_j, float64 in step order; missing at every step: the
        first marker (NaN without one)"""
        slot = getattr(self, '_surfaces', None)
        if slot is None:
            return
        dt = self._uv_dtype
        with numpy.errstate(over='ignore'):
            marks = [float(dt.type(m)) for m in (slot['fill'], slot['missing']) if m == m]
        marks = [m for m in marks if m == m]
        if slot['nt'] == 1 and not slot.get('derived'):
            out = [self._as_float64(s) for s in slot['items']]
        else:
            idx, w = (list(range(t0, t1)), None) if table is None else table[:2]
            sums = [(numpy.zeros((self.ny, self.nx)), numpy.zeros((self.ny, self.nx))) for _ in slot['items']]
            for j, t in enumerate(idx):         # step by step: a derived item is computed once per step for all its planes
                for s, (num, den) in zip(slot['items'], sums):
                    x = self._surface_step_host(s, t)
                    ok = ~numpy.isnan(x)
                    for m in marks:
                        ok &= x != x.dtype.type(m)
                    wj = numpy.float64(1.0 if w is None else w[j])
                    num += numpy.where(ok, wj * numpy.where(ok, x, 0).astype(numpy.float64), 0.0)
                    den += numpy.where(ok, wj, 0.0)
            with numpy.errstate(invalid='ignore', divide='ignore'):
                out = [numpy.where(den > 0, num / den, marks[0] if marks else numpy.nan) for num, den in sums]
        mean.setDepthSurfaces(out, top=slot['top'], fill_value=marks[0] if marks else None,
                              missing_value=marks[1] if len(marks) > 1 else None, wrapX=slot['wrapX'])

    def computeSurfaceTransport(self, tIndex, carry=False, out=None, prefetch_next=None):
        """Transport of time step tIndex between the surfaces of setDepthSurfaces: (m+2, ntransect) totals and (m+2, nseg)
        per-segment sums.  Row 0: above surface 1; row k: between surfaces k and k+1; row m: below surface m; row m+1: the
        terms of a face where a surface has no finite value, or whose interface depth is not finite (exactly +0.0
        otherwise).  The terms, the interface depths of the layers and the spreading are those of computeDepthTransport
        (carry=True, setTracer first: the tracer's terms; with setCellThickness the depths are sums of the cell thicknesses
        at the face), but the edges are the face's own: the mean of each surface in the two cells beside the face (the
        present one when only one has a value), each raised to the surface before it, so that a surface that rises above
        the one before it bounds a layer of zero width there.  With surfaces that are constant over the grid the rows are
        those of computeDepthTransport with these edges, bit for bit.  The rows add up to the sum over z of the profile rows
        (up to rounding) and go into classStreamfunction as they are.  Levels this rank does not own (slab_range)
        contribute nothing, but the depths are summed from level 0.  Leaves everything else as it is.  `out`: as in
        computeClassTransport."""
        slot = getattr(self, '_surfaces', None)
        if slot is None:
            raise RuntimeError('ERROR: call setDepthSurfaces first')
        rows = self._product('nf_field_compute_surface_transport', tIndex, (len(slot['items']) + 2,), carry=bool(carry),
                             tracer=carry, surfaces=True, out=out, prefetch_next=prefetch_next)
        return self._split_rows(rows)

    def computeGrossClassTransport(self, tIndex, carry=False, out=None, prefetch_next=None):
        """Gross transports of time step tIndex in tracer classes (setTracer and setClassEdges first): (totals, segments) of
        shape (2, nedges+2, ntransect) and (2, nedges+2, nseg), part 0 = P, the inflow of every class (what goes through the
        section in the direction computeFlux counts positive), part 1 = N, its outflow (<= 0 in the volume form); rows and
        class field as in computeClassTransport.  Every term of computeGrossProfile goes to the row of its own face's class
        instead of its level: to P where the water term of its slot is > 0, to N where it is < 0.  carry=True: the terms of
        computeClassTracerTransport instead, split by the direction of the water at their slot.  Unlike computeClassTransport
        and computeClassTracerTransport this call takes a cell thickness (setCellThickness), so P + N is the class transport
        under partial steps and z* thicknesses -- on the Field of timeMean(thicknessWeighted=True) too; without one P + N is
        their rows up to rounding.  The parts go as they are into grossTransport (the sum over the classes),
        transportWeightedTracer (the mean tracer of a class's inflow) and classStreamfunction(P + N).  Levels this rank does
        not own (slab_range) contribute nothing.  Leaves the resident edge fluxes, the running max, the row of the last
        computeFlux and the tracer, class and joint rows as they are.  `out`: optional contiguous float64 torch CUDA tensor
        (2 * (nedges+2), row_length), P's rows then N's, that receives the raw rows in HBM (for
        nemoflux_amd.dist.reduce_rows)."""
        edges = getattr(self, '_class_edges', None)
        if edges is None:
            raise RuntimeError('ERROR: call setClassEdges first')
        nrows = edges.size + 2
        rows = self._product('nf_field_compute_gross_class_transport', tIndex, (2 * nrows,), carry=bool(carry), out=out,
                             prefetch_next=prefetch_next)
        return self._split_rows(rows.reshape(2, nrows, self._row_width))

    def computeGrossClassRemap(self, tIndex, carry=False, out=None, prefetch_next=None):
        """Gross transports of time step tIndex in tracer classes by conservative (piecewise-linear) remapping (setTracer and
        setClassEdges first): what computeGrossClassTransport returns -- (totals, segments) of shape (2, nedges+2, ntransect)
        and (2, nedges+2, nseg), part 0 = P, the inflow of every class, part 1 = N, its outflow -- with every term spread over
        the classes by the rule of computeClassRemap (the interval between the class field's values at the layer's upper and
        lower interface on the term's own face) instead of going whole to the class of its face.  The shares of a term go to
        P where the water term of its slot is > 0 and to N where it is < 0.  carry=True: the terms of
        computeClassTracerTransport, split by the direction of the water all the same.  The inflow and outflow of every class
        are then smooth functions of the class with hundreds of edges on 75 levels, where the step rule gives a comb.  Unlike
        computeClassRemap this call takes a cell thickness (setCellThickness): P + N is the remapped class transport -- a
        smooth MOC(sigma), heat by sigma -- under partial steps and z* thicknesses, on the Field of
        timeMean(thicknessWeighted=True) too; without one P + N is the rows of computeClassRemap up to rounding.  A class field
        that is constant in z gives the parts of computeGrossClassTransport bit for bit.  The parts go as they are into
        grossTransport, transportWeightedTracer and classStreamfunction(P + N).  Levels this rank does not own (slab_range)
        contribute nothing, but the class field is read one level beyond them.  Leaves everything else as it is.  `out`: as
        in computeGrossClassTransport."""
        edges = getattr(self, '_class_edges', None)
        if edges is None:
            raise RuntimeError('ERROR: call setClassEdges first')
        nrows = edges.size + 2
        rows = self._product('nf_field_compute_gross_class_remap', tIndex, (2 * nrows,), carry=bool(carry), out=out,
                             prefetch_next=prefetch_next)
        return self._split_rows(rows.reshape(2, nrows, self._row_width))

    def computeClassArea(self, tIndex, out=None, prefetch_next=None):
        """Section area of time step tIndex in tracer classes (setTracer and setClassEdges first): (totals, segments) of shape
        (2, nedges+2, ntransect) and (2, nedges+2, nseg), part 0 = A, the area of the section that every class occupies,
        part 1 = B, the area-weighted tracer of setTracer (reference subtracted) in it; rows and class field as in
        computeClassTransport.  Every term of computeAreaProfile -- |w| * th * arc over the faces that count (velocity present,
        tracer face value finite), and the same times (tracer face value - reference) -- goes to the row of its own face's
        class instead of its level, so the rows add up over the classes to the depth sums of computeAreaProfile (up to
        rounding).  th is thickness[z], or the cell thickness at the face when one is set (setCellThickness).  No Sverdrup
        scale.  With a class field of its own (setClassTracer, or a Sigma) row nedges+1 holds the counted faces without a
        class value; without one it is empty.  A goes into classInterfaceDepth (the depth axis of classStreamfunction), the
        pair into classMeanTracer (the mean theta of a sigma class) and into overturningGyre
        (decomposeTracerTransportByClass).  Levels this rank does not own (slab_range) contribute nothing.  Leaves the
        resident edge fluxes, the running max, the row of the last computeFlux and the tracer, class and joint rows as they
        are.  `out`: optional contiguous float64 torch CUDA tensor (2 * (nedges+2), row_length), A's rows then B's, that
        receives the raw rows in HBM (for nemoflux_amd.dist.reduce_rows)."""
        edges = getattr(self, '_class_edges', None)
        if edges is None:
            raise RuntimeError('ERROR: call setClassEdges first')
        nrows = edges.size + 2
        rows = self._product('nf_field_compute_class_area', tIndex, (2 * nrows,), out=out, prefetch_next=prefetch_next)
        return self._split_rows(rows.reshape(2, nrows, self._row_width))

    @staticmethod
    def classMeanTracer(areaParts, reference=0.0):
        """Area-weighted mean tracer of every class: B / A + reference from the parts (2, ...) = A, B of computeClassArea
        (totals or segments alike); `reference`: the reference of setTracer, which B has subtracted.  NaN where A is 0."""
        P = numpy.asarray(areaParts, dtype=numpy.float64)
        if P.ndim < 1 or P.shape[0] != 2:
            raise ValueError(f'classMeanTracer: the parts must have shape (2, ...), got {P.shape}')
        with numpy.errstate(divide='ignore', invalid='ignore'):
            return numpy.where(P[0] != 0.0, P[1] / P[0] + float(reference), numpy.nan)

    @staticmethod
    def classInterfaceDepth(classArea, areaProfile, bounds_depth):
        """Pseudo-depth of the class interfaces: the depth axis that classStreamfunction is drawn against.  Host only,
        float64, on rows that have been summed over all ranks first (the step is not linear).  classArea: A (nedges+2, n) of
        computeClassArea; areaProfile: A(z) (nz, n) of computeAreaProfile; bounds_depth (nz, 2), top then bottom of every
        level (a Field's bounds_depth) -- totals or segments alike.  Per column and edge k, with
            phi_k = (A[0] + ... + A[k]) / (A[0] + ... + A[nedges])      (the row of the faces without a class value left out)
        the result is the depth d above which the section has that fraction of its area: G(d) / G(inf) = phi_k, G the
        piecewise-linear area above d, level z filling linearly between its two bounds; where G is flat, the shallowest such
        d.  Returns (nedges, n), non-decreasing in k; NaN where either total is 0."""
        C = numpy.asarray(classArea, dtype=numpy.float64)
        Z = numpy.asarray(areaProfile, dtype=numpy.float64)
        bd = numpy.asarray(bounds_depth, dtype=numpy.float64)
        if C.ndim != 2 or C.shape[0] < 4 or Z.ndim != 2 or Z.shape[1] != C.shape[1] or bd.shape != (Z.shape[0], 2):
            raise ValueError(f'classInterfaceDepth: need classArea (nedges+2, n) with nedges >= 2, areaProfile (nz, n) and '
                             f'bounds_depth (nz, 2), got {C.shape}, {Z.shape}, {bd.shape}')
        top, bot = bd[:, 0], bd[:, 1]
        if not numpy.all(bot > top):
            raise ValueError('classInterfaceDepth: every level needs bounds_depth[z, 0] < bounds_depth[z, 1]')
        nedges, n = C.shape[0] - 2, C.shape[1]
        cum = numpy.cumsum(C[:nedges + 1], axis=0)             # cum[k] = A[0] + ... + A[k]; cum[nedges]: the class total
        b = numpy.unique(bd)                                   # the depths at which G changes slope
        G = numpy.zeros((b.size, n))                           # G at those depths, the levels added z ascending
        for z in range(Z.shape[0]):
            G += numpy.clip((b - top[z]) / (bot[z] - top[z]), 0.0, 1.0)[:, None] * Z[z][None, :]
        depth = numpy.full((nedges, n), numpy.nan)
        for c in range(n):
            if not (cum[nedges, c] > 0.0 and G[-1, c] > 0.0):
                continue
            g = (cum[:nedges, c] / cum[nedges, c]) * G[-1, c]
            i = numpy.minimum(numpy.searchsorted(G[:, c], g, side='left'), b.size - 1)   # the first depth with G >= g
            lo = numpy.maximum(i - 1, 0)
            rise = G[i, c] - G[lo, c]
            with numpy.errstate(divide='ignore', invalid='ignore'):
                f = numpy.where(rise > 0.0, (g - G[lo, c]) / rise, 1.0)
            depth[:, c] = numpy.where(i > 0, b[lo] + f * (b[i] - b[lo]), b[0])
        return depth

    def decomposeTracerTransportByClass(self, tIndex):
        """The tracer transport of time step tIndex and its throughflow, overturning and gyre parts with the classes of the
        class field in the place of the levels (setTracer and setClassEdges first), for the transect totals: the overturning
        part is what the diapycnal circulation carries, the gyre part what is carried along the classes.  overturningGyre
        with V = the class transport rows (P + N of computeGrossClassTransport when a cell thickness is set, else
        computeClassTransport), (A, B) of computeClassArea and H of computeTracerFlux; 'mean' is then (nedges+2, ntransect).
        On one rank only; sharded runs reduce the rows first (docs/MULTIGPU.md)."""
        if getattr(self, '_e3', None) is not None:
            P = self.computeGrossClassTransport(tIndex)[0]
            V = P[0] + P[1]
        else:
            V = self.computeClassTransport(tIndex)[0]
        AB = self.computeClassArea(tIndex)[0]
        H = self.computeTracerFlux(tIndex)[0]
        return self.overturningGyre(V, (AB[0], AB[1]), H)

    @staticmethod
    def classStreamfunction(rows):
        """Overturning streamfunction in class space from the rows of computeClassTransport or computeClassTracerTransport,
        or from P + N of computeGrossClassTransport (the one form that takes a cell thickness)
        (totals or segments, classes first): psi[k] = rows[0] + ... + rows[k], k = 0 .. nedges-1, the transport of the faces whose class value is below
        e[k].  The rows of computeDepthTransport give the overturning streamfunction in depth, the transport above e[k].
        Host only."""
        R = numpy.asarray(rows, dtype=numpy.float64)
        if R.ndim < 1 or R.shape[0] < 4:
            raise ValueError(f'classStreamfunction: need the nedges + 2 >= 4 rows of computeClassTransport, got shape {R.shape}')
        return numpy.cumsum(R[:R.shape[0] - 2], axis=0)

    def setJointClassEdges(self, edgesA, edgesB):
        """Class edges of the two axes of computeJointClassTransport: edgesA for the tracer of setTracer, edgesB for the tracer
        of setClassTracer, each finite, strictly increasing, 2 <= n <= 1025, with (nA + 2) * (nB + 2) <= 16384 joint rows.
        They are kept apart from setClassEdges: the 1-D class calls do not see them.  (None, None) clears them."""
        if edgesA is None and edgesB is None:
            check(lib.nf_field_set_joint_class_edges(ctypes.byref(self._h), None, 0, None, 0))
            self._joint_edges = None
            return
        if edgesA is None or edgesB is None:
            raise RuntimeError('ERROR: setJointClassEdges needs both edge sets (or None for both)')
        ea = numpy.array(edgesA, dtype=numpy.float64).reshape(-1)
        eb = numpy.array(edgesB, dtype=numpy.float64).reshape(-1)
        check(lib.nf_field_set_joint_class_edges(ctypes.byref(self._h), _lib.dptr(ea), int(ea.size), _lib.dptr(eb), int(eb.size)))
        self._joint_edges = (ea, eb)

    def computeJointClassTransport(self, tIndex, carry=False, out=None, prefetch_next=None):
        """Transport of time step tIndex in joint classes of two tracers (setTracer: axis A, setClassTracer: axis B,
        setJointClassEdges first): totals (nA+2, nB+2, ntransect) and per-segment sums (nA+2, nB+2, nseg) -- the volumetric
        T-S census of the sections.  Entry [ra, rb] holds the terms of the faces whose value of A lies in row ra of edgesA and
        whose value of B lies in row rb of edgesB, rows as in computeClassTransport (the last one of an axis: faces without a
        value of that tracer).  carry=False: the volume terms of computeClassTransport; carry=True: the transport of the
        tracer A (reference subtracted), the terms of computeClassTracerTransport.  Summed over rb the rows are those of the
        1-D call binned by A, summed over ra those binned by B (up to rounding).  Levels this rank does not own (slab_range)
        contribute nothing.  Leaves everything else as it is.  `out`: optional contiguous float64 torch CUDA tensor
        ((nA+2)*(nB+2), row_length) that receives the raw rows in HBM (for nemoflux_amd.dist.reduce_rows)."""
        edges = getattr(self, '_joint_edges', None)
        if edges is None:
            raise RuntimeError('ERROR: call setJointClassEdges first')
        na, nb = edges[0].size + 2, edges[1].size + 2
        rows = self._product('nf_field_compute_joint_class_transport', tIndex, (na * nb,), carry=bool(carry), out=out,
                             prefetch_next=prefetch_next)
        tot, seg = self._split_rows(rows)
        return tot.reshape((na, nb) + tot.shape[1:]), seg.reshape((na, nb) + seg.shape[1:])

    @staticmethod
    def jointClassStreamfunction(rows, axis=0):
        """Streamfunction in the space of two tracers from the rows of computeJointClassTransport (totals or segments, the two
        class axes first): the cumulative sum along class axis `axis` (0: A, 1: B) over its rows 0 .. n-1 -- the `>= last
        edge` row and the no-value row of that axis are left out, as in classStreamfunction; the other axis is kept whole.
        Host only."""
        R = numpy.asarray(rows, dtype=numpy.float64)
        if axis not in (0, 1):
            raise ValueError(f'jointClassStreamfunction: axis must be 0 or 1, got {axis!r}')
        if R.ndim < 2 or R.shape[0] < 4 or R.shape[1] < 4:
            raise ValueError('jointClassStreamfunction: need the (nA + 2, nB + 2, ...) rows of computeJointClassTransport, '
                             f'got shape {R.shape}')
        keep = [slice(None)] * R.ndim
        keep[axis] = slice(0, R.shape[axis] - 2)
        return numpy.cumsum(R[tuple(keep)], axis=axis)

    def depthBandFlux(self, profile, ztop, zbot):
        """Flux between the depths ztop < zbot (the units of deptht_bounds) from a profile of computeFluxProfile or
        computeTracerProfile (totals or segments, levels first): level z contributes profile[z] * overlap([ztop, zbot], layer z) / thickness[z], exact
        because a level's flux is linear in its thickness; layers of zero thickness contribute nothing.  With a cell
        thickness set (setCellThickness) the levels are still selected, and cut, by the nominal deptht_bounds: a level
        inside the band enters whole with its per-cell thicknesses, a level cut by ztop or zbot with the nominal fraction."""
        ztop, zbot = float(ztop), float(zbot)
        if not ztop <= zbot:
            raise ValueError(f'depthBandFlux: need ztop <= zbot, got {ztop}, {zbot}')
        P = numpy.asarray(profile, dtype=numpy.float64)
        if P.shape[:1] != (self.nz,):
            raise ValueError(f'depthBandFlux: the profile must have {self.nz} levels first, got shape {P.shape}')
        return _band_sum(P, self.bounds_depth, ztop, zbot)

    def getFluxText(self):
        """field.py:98-109."""
        txt = ""
        for pli in self.plis:
            totalFlux = pli.getIntegral(self.integratedVelocity, mint.CELL_BY_CELL_DATA)
            txt += f"{totalFlux:4.3g}, "
        if self.sverdrup:
            txt += "(Sv) "
        else:
            txt += "(A m^2/s) "
        txt = re.sub(r',\s*\(', ' (', txt)
        return txt

    def getWeights(self):
        """(cell*4+edge, weight, global segment id) of the batched transect set."""
        n = ctypes.c_size_t()
        check(lib.nf_field_num_weights(ctypes.byref(self._h), ctypes.byref(n)))
        ce = numpy.empty(n.value, numpy.int64)
        w = numpy.empty(n.value, numpy.float64)
        sg = numpy.empty(n.value, numpy.int32)
        check(lib.nf_field_get_weights(ctypes.byref(self._h), ce.ctypes.data_as(_lib.c_int64_p), _lib.dptr(w),
                                       sg.ctypes.data_as(_lib.c_int_p)))
        return ce, w, sg

    def getCoverage(self):
        """Per transect: the fraction of each of its target segments that lies inside cells of the grid (1 = inside, each
        point counted once; less = part of the line is outside the grid and contributes no flux)."""
        cov = numpy.zeros(max(self._nseg, 1), numpy.float64)
        check(lib.nf_field_get_coverage(ctypes.byref(self._h), _lib.dptr(cov)))
        return [cov[self._tr_off[i]:self._tr_off[i + 1]].copy() for i in range(len(self.plis))]

    def getEdgeWeights(self):
        """(element of [eU | eV], weight, global segment id): the weights folded onto the unique edges of the two signed
        planes, which is what the on-device reduction gathers (one value per entry)."""
        n = ctypes.c_size_t()
        check(lib.nf_field_num_edge_weights(ctypes.byref(self._h), ctypes.byref(n)))
        el = numpy.empty(n.value, numpy.int32)
        sg = numpy.empty(n.value, numpy.int32)
        w = numpy.empty(n.value, numpy.float64)
        check(lib.nf_field_get_edge_weights(ctypes.byref(self._h), el.ctypes.data_as(_lib.c_int_p),
                                            sg.ctypes.data_as(_lib.c_int_p), _lib.dptr(w)))
        return el, w, sg

    # timing hooks for bench.py
    def enableKernelTiming(self, on=True, reserve=0):
        """reserve: number of launches whose events are created now, outside the timed region"""
        check(lib.nf_field_timing(ctypes.byref(self._h), max(1, int(reserve)) if on else 0))

    def readKernelTiming(self, split=False):
        """(launches, total ms) of the timed steps since enableKernelTiming; split=True appends the flux-kernel and the
        expansion-kernel shares of that total."""
        n, ms = ctypes.c_long(), ctypes.c_double()
        check(lib.nf_field_timing_read(ctypes.byref(self._h), ctypes.byref(n), ctypes.byref(ms)))
        if not split:
            return n.value, ms.value
        a, b = ctypes.c_double(), ctypes.c_double()
        check(lib.nf_field_timing_split(ctypes.byref(self._h), ctypes.byref(a), ctypes.byref(b)))
        return n.value, ms.value, a.value, b.value

    def readTransectTiming(self):
        """ms spent in the transect reductions behind the launches of the last readKernelTiming"""
        k3 = ctypes.c_double()
        check(lib.nf_field_timing_k3(ctypes.byref(self._h), ctypes.byref(k3)))
        return k3.value
