"""A sparse float64 / long-double reference of the section area and the area-weighted tracer of one time step
(nf_field_compute_area_profile), for any grid size: the definition of include/nemoflux_amd.h restated in numpy over the cells
the weight entries touch.  It uses the entry / face bookkeeping and the summation of tests/resolved_reference.py, through
tests/cellthick_reference.py, and shares no code with the product.

Per level z and entry (cell c, slot, weight w, segment), with `a` the cell whose face the slot is (east, north: c; west: the
west cell; south: the south cell; the south entries of row 0 are dropped):

    the face counts   the velocity at the face (uo[t, z, a] for east / west slots, vo[t, z, a] for north / south slots) is
                      present, and the carried tracer has a face value x (0.5 (a + b), the present one, or none) that is finite
    area term         |w| * (th * arc)           th = thickness[z], or fixth(e3u[t', z, a]) / fixth(e3v[t', z, a]);  arc > 0
    tracer term       (|w| * (th * arc)) * (x - reference)

both 0 for a face that does not count.  No Sverdrup scale.  Terms are formed in float64 and summed in long double per
(level, segment), the transect columns from the segments; `mag` is the sum of the absolute values of the terms.
"""
import concurrent.futures

import numpy

from cellthick_reference import CellThickReference, array_values  # noqa: F401  (array_values: for the callers)
from resolved_reference import ACC, _face, _group_sums, _present


class SectionReference(CellThickReference):
    """CellThickReference with the two rows of the area profile.  cell_thickness=True: the thickness is read at the face
    ('e3u', 'e3v' of the callback, markers thick_markers); otherwise `thickness` (nz,) is used."""

    def __init__(self, *a, cell_thickness=False, **kw):
        super().__init__(*a, **kw)
        self.cell_thickness = bool(cell_thickness)
        self.f_abs_arc = numpy.abs(self.f_arc)

    def area_step(self, values, threads=1):
        """values(name, z, cells) -> the raw values of 'uo', 'vo', 'tracer' (and 'e3u', 'e3v' with cell_thickness) of level z
        at the flat cell indices `cells`, in the array's dtype.  Returns {'area_profile': (want, mag), 'tracer_area_profile':
        (want, mag)}, each of shape (nz, row_length), rows [segments | transects]."""
        nz, nseg = self.nz, self.nseg
        prof = numpy.zeros((nz, nseg, 4), ACC)   # last axis: area, sum |area terms|, tracer, sum |tracer terms|
        aw = numpy.abs(self.w)

        def level(z):
            uo, vo = values('uo', z, self.cells), values('vo', z, self.cells)
            has_v = numpy.where(self.f_is_u, _present(uo, self.uv_markers)[self.ia], _present(vo, self.uv_markers)[self.ia])
            tau = values('tracer', z, self.cells)
            has_t, xt = _face(tau[self.ia], tau[self.ib], self.f_has_b, self.tracer_markers)
            counts = has_v & has_t & numpy.isfinite(numpy.where(has_t, xt, 0.0))
            if self.cell_thickness:
                e3u, e3v = values('e3u', z, self.cells), values('e3v', z, self.cells)
                fu = numpy.where(_present(e3u, self.thick_markers), e3u.astype(numpy.float64), 0.0)
                fv = numpy.where(_present(e3v, self.thick_markers), e3v.astype(numpy.float64), 0.0)
                th = numpy.where(self.f_is_u, fu[self.ia], fv[self.ia])
            else:
                th = self.thickness[z]
            da = numpy.where(counts, th * self.f_abs_arc, 0.0)          # per face: th * arc
            dx = numpy.where(counts, xt, self.reference) - self.reference
            alpha = aw * da[self.face_of]                                # per entry
            beta = alpha * dx[self.face_of]
            out = numpy.zeros((self.seg_starts.size, 4), ACC)
            for q, t in ((0, alpha), (2, beta)):
                out[:, q], out[:, q + 1] = _group_sums(t, self.seg_starts), _group_sums(numpy.abs(t), self.seg_starts)
            prof[z][self.useg] = out

        if threads > 1:
            with concurrent.futures.ThreadPoolExecutor(threads) as pool:
                list(pool.map(level, range(nz)))
        else:
            for z in range(nz):
                level(z)

        def pair(q):
            return self._with_totals(prof[..., q]), self._with_totals(prof[..., q + 1])

        return {'area_profile': pair(0), 'tracer_area_profile': pair(2)}
