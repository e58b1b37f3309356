"""The reference of the transport in joint classes of two tracers, for any grid size ("Transport in joint
classes of two tracers"): the volume and tracer terms, the class row and the summation of tests/resolved_reference.py, with
its own row

    row          ra * (nB + 2) + rb; ra = the class row of the raw face value of A among the edges of A, rb the same for B
                 with its own markers and edges

A is the carried tracer.  A value of a joint row, segment is the sum of its terms, `mag` the sum of their absolute values; a
transect's value is the sum of its segments.  The entries of one (level, row, segment) are summed first, then the levels.
"""
import numpy

from resolved_reference import ACC, ResolvedReference, class_rows


class JointClassReference(ResolvedReference):
    """ResolvedReference's constructor: tracer_markers are A's (the carried tracer), class_markers are B's."""

    def joint(self, values, edges_a, edges_b):
        """values(name, z, cells): as in ResolvedReference.step, 'tracer' = A, 'class' = B.  Returns {'volume': (want, mag),
        'tracer': (want, mag)}, every array ((nA + 2) * (nB + 2), row_length) = [segments | transects] per joint row."""
        ea, eb = numpy.asarray(edges_a, dtype=numpy.float64), numpy.asarray(edges_b, dtype=numpy.float64)
        nrows = (ea.size + 2) * (eb.size + 2)
        acc = numpy.zeros((nrows * self.nseg, 4), ACC)    # last axis: volume, sum |volume terms|, tracer, sum |tracer terms|

        def level(z):
            dv, dt, has_a, xa = self._factors(values, z)
            row = class_rows(has_a, xa, ea) * (eb.size + 2) + self._class_rows(values, z, eb)
            keys, sums = self._bin(row[self.face_of], [self._entries(dv), self._entries(dt)], nrows)
            acc[keys] += sums

        with numpy.errstate(invalid='ignore', over='ignore'):    # an infinite A makes its carried terms infinite or NaN
            self._each_level(level)
            acc = acc.reshape(nrows, self.nseg, 4)
            return {'volume': self._pair(acc, 0), 'tracer': self._pair(acc, 2)}
