"""The reference of the section area and the area-weighted tracer of one time step (nf_field_compute_area_profile), for any
grid size.  Entries, faces, presence, face values, the thickness th and the summation are those of
tests/resolved_reference.py; its own are the rule by which a face counts and the terms, which carry |w| and no velocity:

    the face counts   the velocity at the face (uo[t, z, a] for east / west slots, vo[t, z, a] for north / south slots) is
                      present, and the carried tracer has a face value x that is finite
    area term         |w| * (th * arc)           arc > 0
    tracer term       (|w| * (th * arc)) * (x - reference)

both 0 for a face that does not count.  No Sverdrup scale.  Terms are summed per (level, segment), the transect columns from
the segments; `mag` is the sum of the absolute values of the terms.
"""
import numpy

from resolved_reference import ACC, ResolvedReference, _present, _term_sums, array_values  # noqa: F401  (for the callers)


class SectionReference(ResolvedReference):
    """ResolvedReference with the two rows of the area profile."""

    def area_step(self, values, threads=1):
        """values(name, z, cells): as in ResolvedReference.step, 'uo', 'vo', 'tracer' (and 'e3u', 'e3v' with cell_thickness).
        Returns {'area_profile': (want, mag), 'tracer_area_profile': (want, mag)}, each of shape (nz, row_length), rows
        [segments | transects]."""
        prof = numpy.zeros((self.nz, self.nseg, 4), ACC)   # last axis: area, sum |area terms|, tracer, sum |tracer terms|
        aw, abs_arc = numpy.abs(self.w), numpy.abs(self.f_arc)

        def level(z):
            uo, vo = values('uo', z, self.cells), values('vo', z, self.cells)
            has_v = numpy.where(self.f_is_u, _present(uo, self.uv_markers)[self.ia], _present(vo, self.uv_markers)[self.ia])
            has_t, xt = self._face_values(values, z, 'tracer', self.tracer_markers)
            counts = has_v & has_t & numpy.isfinite(numpy.where(has_t, xt, 0.0))
            da = numpy.where(counts, self._thick(values, z) * abs_arc, 0.0)          # per face: th * arc
            dx = numpy.where(counts, xt, self.reference) - self.reference
            alpha = aw * da[self.face_of]                                              # per entry
            prof[z][self.useg] = _term_sums([alpha, alpha * dx[self.face_of]], self.seg_starts)

        self._each_level(level, threads)
        return {'area_profile': self._pair(prof, 0), 'tracer_area_profile': self._pair(prof, 2)}
