"""The reference of the gross transports in tracer classes of one time step (nf_field_compute_gross_class_transport), for any
grid size: the terms q and c of tests/gross_reference.py in the class rows of tests/resolved_reference.py.

    P[r] = sum of c over the entries of row r with q > 0,    N[r] = sum of c over those with q < 0;    q == 0: in neither.

The callback serves 'uo', 'vo', 'class' (the class field: its markers are class_markers), 'tracer' (the carried tracer, with
tracer=True; markers tracer_markers) and 'e3u', 'e3v' with cell thicknesses.  Terms are summed per (level, part, row, segment),
then the levels, then the transect columns from the segments.  `mag` is the sum of |c| over the entries of the value;
min_abs_q the smallest non-zero |q| met.
"""
import threading

import numpy

from gross_reference import GrossReference
from resolved_reference import ACC


class GrossClassReference(GrossReference):
    """GrossReference with the rows of the gross class transport."""

    def gross_class_step(self, values, edges, tracer=True, threads=1):
        """Returns {'volume': (want, mag), 'carried': (want, mag) (tracer=True), 'min_abs_q': float}; want and mag have shape
        (2, len(edges) + 2, row_length): P then N, rows [segments | transects]."""
        edges = numpy.asarray(edges, dtype=numpy.float64)
        nrows = edges.size + 2
        acc = numpy.zeros((2 * nrows * self.nseg, 4 if tracer else 2), ACC)
        min_q = [numpy.inf] * self.nz
        lock = threading.Lock()

        def level(z):
            q, cs, min_q[z] = self._gross_terms(values, z, tracer)
            live = numpy.flatnonzero(q != 0)                                   # only these are binned
            r = self._class_rows(values, z, edges)
            row = numpy.where(q[live] < 0, nrows, 0) + r[self.face_of[live]]   # part * (n + 2) + r
            keys, sums = self._bin(row, cs, 2 * nrows, sel=live)
            with lock:
                acc[keys] += sums

        self._each_level(level, threads)
        return self._gross_result(acc.reshape(2, nrows, self.nseg, -1), min_q)
