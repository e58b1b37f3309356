"""The reference of the section area in tracer classes of one time step (nf_field_compute_class_area), for any grid size: the
area term and the tracer term of tests/section_reference.py in the class rows of tests/resolved_reference.py.

    A[r] = sum of the area terms of the entries whose face counts and has class row r,    B[r] = the same of the tracer terms

The callback serves 'uo', 'vo' (read for their presence alone), 'tracer' (the carried tracer; markers tracer_markers), 'class'
(the class field: its markers are class_markers; the same array as 'tracer' when the tracer is binned by itself) and 'e3u',
'e3v' with cell thicknesses.  A face that does not count is in no row.  Terms are summed per (level, part, row, segment), then
the levels, then the transect columns from the segments.  `mag` is the sum of the absolute values of the terms of the value.
"""
import threading

import numpy

from resolved_reference import ACC, _present
from section_reference import SectionReference


class ClassAreaReference(SectionReference):
    """SectionReference with the rows of the class area."""

    def _area_terms(self, values, z):
        """per entry: whether its face counts, the area term and the tracer term (the rule and the terms of area_step)"""
        uo, vo = values('uo', z, self.cells), values('vo', z, self.cells)
        has_v = numpy.where(self.f_is_u, _present(uo, self.uv_markers)[self.ia], _present(vo, self.uv_markers)[self.ia])
        has_t, xt = self._face_values(values, z, 'tracer', self.tracer_markers)
        counts = has_v & has_t & numpy.isfinite(numpy.where(has_t, xt, 0.0))
        da = numpy.where(counts, self._thick(values, z) * numpy.abs(self.f_arc), 0.0)      # per face: th * arc
        dx = numpy.where(counts, xt, self.reference) - self.reference
        alpha = numpy.abs(self.w) * da[self.face_of]                                          # per entry
        return counts[self.face_of], alpha, alpha * dx[self.face_of]

    def class_area_step(self, values, edges, threads=1):
        """values(name, z, cells): as in ResolvedReference.step.  Returns (want, mag) of shape (2, len(edges) + 2, row_length):
        A then B, rows [segments | transects]."""
        edges = numpy.asarray(edges, dtype=numpy.float64)
        nrows = edges.size + 2
        acc = numpy.zeros((nrows * self.nseg, 4), ACC)     # last axis: A, sum |area terms|, B, sum |tracer terms|
        lock = threading.Lock()

        def level(z):
            counts, alpha, beta = self._area_terms(values, z)
            live = numpy.flatnonzero(counts)                                   # only these are binned
            row = self._class_rows(values, z, edges)[self.face_of[live]]
            keys, sums = self._bin(row, [alpha, beta], nrows, sel=live)
            with lock:
                acc[keys] += sums

        self._each_level(level, threads)
        acc = acc.reshape(nrows, self.nseg, 4)
        (a, am), (b, bm) = self._pair(acc, 0), self._pair(acc, 2)
        return numpy.stack([a, b]), numpy.stack([am, bm])
