"""A sparse float64 / long-double reference of the transports with per-cell layer thicknesses (nf_field_set_cell_thickness),
for any grid size: the definition of include/nemoflux_amd.h restated in numpy over the cells the weight entries touch.  It uses
the entry / face bookkeeping and the two-stage summation of tests/resolved_reference.py and shares no code with the product.

Per level z and entry (cell c, slot, weight w, segment), with `a` the cell whose face the slot is (east, north: c; west: the
west cell; south: the south cell):

    volume term  w * (+fixth(e3u[t', z, a]) * fixed(uo[t, z, a]) * arcE[a])   east and west slots
                 w * (-fixth(e3v[t', z, a]) * fixed(vo[t, z, a]) * arcN[a])   north and south slots
    tracer term  the same with fixed(.) * tf, tf the carried tracer's face value minus the reference (0 without a value)

each times 6.371 in Sverdrup mode.  fixth(x) = 0 where x is NaN or one of the thickness's markers (compared in its dtype), else
x in float64; fixed likewise with the markers of uo / vo.  t' = t for a time-varying thickness, 0 for a static one: the caller's
`values` callback decides what it hands out for 'e3u' and 'e3v'.  Sums and their error: as in resolved_reference.
"""
import concurrent.futures

import numpy

from resolved_reference import ACC, ResolvedReference, _face, _present


class CellThickReference(ResolvedReference):
    """ResolvedReference with the thickness read at the face.  thick_markers: the markers of e3u / e3v (NaN = unused)."""

    def __init__(self, *a, thick_markers=(), **kw):
        super().__init__(*a, **kw)
        self.thick_markers = tuple(thick_markers)

    def step(self, values, threads=1, tracer=True):
        """values(name, z, cells) -> the raw values of 'uo', 'vo', 'e3u', 'e3v' and (tracer=True) 'tracer' of level z at the
        flat cell indices `cells`, in the array's dtype.  Returns (want, mag) pairs of [segments | transects] rows: 'volume'
        and 'tracer' (row_length,), 'volume_profile' (nz, row_length)."""
        nz, nseg = self.nz, self.nseg
        prof = numpy.zeros((nz, nseg, 4), ACC)   # last axis: volume, sum |volume terms|, tracer, sum |tracer terms|

        def level(z):
            fx = {}
            for name, markers in (('uo', self.uv_markers), ('vo', self.uv_markers), ('e3u', self.thick_markers),
                                  ('e3v', self.thick_markers)):
                x = values(name, z, self.cells)
                fx[name] = numpy.where(_present(x, markers), x.astype(numpy.float64), 0.0)
            vel = numpy.where(self.f_is_u, fx['uo'][self.ia], fx['vo'][self.ia])
            th = numpy.where(self.f_is_u, fx['e3u'][self.ia], fx['e3v'][self.ia])
            dv = (th * vel) * self.f_arc
            dt = None
            if tracer:
                tau = values('tracer', z, self.cells)
                has_t, xt = _face(tau[self.ia], tau[self.ib], self.f_has_b, self.tracer_markers)
                with numpy.errstate(invalid='ignore'):
                    tf = numpy.where(has_t, numpy.where(has_t, xt, 0.0) - self.reference, 0.0)
                dt = (th * (vel * tf)) * self.f_arc
            if self.scale is not None:
                dv, dt = dv * self.scale, None if dt is None else dt * self.scale
            prof[z][self.useg] = self._term_sums(self.w, self.face_of, dv, dt, self.seg_starts)

        if threads > 1:
            with concurrent.futures.ThreadPoolExecutor(threads) as pool:
                list(pool.map(level, range(nz)))
        else:
            for z in range(nz):
                level(z)

        def pair(a, q):
            return self._with_totals(a[..., q]), self._with_totals(a[..., q + 1])

        sums = prof.sum(axis=0, dtype=ACC)
        return {'volume': pair(sums, 0), 'tracer': pair(sums, 2), 'volume_profile': pair(prof, 0)}


def array_values(arrays, t):
    """the `values` callback for host arrays {'uo': (nt, nz, ny, nx), ..., 'e3u': (nt or 1, nz, ny, nx), ...} at step t: an
    array with one step is static"""
    def values(name, z, cells):
        a = arrays[name]
        return a[t if a.shape[0] > 1 else 0, z].reshape(-1)[cells]
    return values
