"""A sparse float64 / long-double restatement of the transport in joint classes of two tracers, for any grid size.

It restates DESIGN.md section 4 ("Transport in joint classes of two tracers") from the weight entries alone and shares no
code with the product.  It re-uses the constructor of resolved_reference.ResolvedReference (the entries, their faces and the
cells whose values are needed) and its helpers _face / _present / _group_sums; the binning below is its own.

Per level z and entry (cell, slot, weight w, segment) whose face has the first cell a and the second cell b:

    volume term  w * (+th_z * fixed(uo[a]) * arcE[a])  (east, west slots);  w * (-th_z * fixed(vo[a]) * arcN[a])  (north, south)
    tracer term  the same with fixed(.) * tf, tf = face value of A - reference (0 when the face has no value of A)
    row          ra * (nB + 2) + rb; ra = the number of edges of A <= the raw face value of A (no value, or NaN: nA + 1),
                 rb the same for B with its own markers and edges

each term times 6.371 in Sverdrup mode; row 0's south entries carry nothing.  A value of a joint row, segment is the sum of its
terms, `mag` the sum of their absolute values; a transect's value is the sum of its segments.  Summation as in
resolved_reference: the entries of one (level, row, segment) in long double, then the levels -- its docstring derives the
error, well inside 1e-12 x mag.
"""
import numpy

from resolved_reference import ACC, ResolvedReference, _face, _group_sums, _present


def _rows_of(has, x, edges):
    """1-D class row of the face values x (has: the face has a value): edges <= x, or len(edges) + 1"""
    classed = has & ~numpy.isnan(x)
    return numpy.where(classed, numpy.searchsorted(edges, numpy.where(classed, x, 0.0), side='right'), edges.size + 1)


class JointClassReference(ResolvedReference):
    """ResolvedReference's constructor: tracer_markers are A's (the carried tracer), class_markers are B's."""

    def joint(self, values, edges_a, edges_b):
        """values(name, z, cells): as in ResolvedReference.step, 'tracer' = A, 'class' = B.  Returns {'volume': (want, mag),
        'tracer': (want, mag)}, every array ((nA + 2) * (nB + 2), row_length) = [segments | transects] per joint row."""
        ea, eb = numpy.asarray(edges_a, dtype=numpy.float64), numpy.asarray(edges_b, dtype=numpy.float64)
        nrows, nseg = (ea.size + 2) * (eb.size + 2), self.nseg
        acc = numpy.zeros((nrows * nseg, 4), ACC)    # last axis: volume, sum |volume terms|, tracer, sum |tracer terms|
        for z in range(self.nz):
            uo, vo = values('uo', z, self.cells), values('vo', z, self.cells)
            A, B = values('tracer', z, self.cells), values('class', z, self.cells)
            fixed_u = numpy.where(_present(uo, self.uv_markers), uo.astype(numpy.float64), 0.0)
            fixed_v = numpy.where(_present(vo, self.uv_markers), vo.astype(numpy.float64), 0.0)
            vel = numpy.where(self.f_is_u, fixed_u[self.ia], fixed_v[self.ia])
            has_a, xa = _face(A[self.ia], A[self.ib], self.f_has_b, self.tracer_markers)
            has_b, xb = _face(B[self.ia], B[self.ib], self.f_has_b, self.class_markers)
            with numpy.errstate(invalid='ignore'):
                tf = numpy.where(has_a, numpy.where(has_a, xa, 0.0) - self.reference, 0.0)
            th = self.thickness[z]
            with numpy.errstate(invalid='ignore', over='ignore'):    # an infinite A makes its carried terms infinite or NaN
                dv, dt = (th * vel) * self.f_arc, (th * (vel * tf)) * self.f_arc
                if self.scale is not None:
                    dv, dt = dv * self.scale, dt * self.scale
            row_face = _rows_of(has_a, xa, ea) * (eb.size + 2) + _rows_of(has_b, xb, eb)
            if self.w.size == 0:
                continue
            key = row_face[self.face_of] * nseg + self.seg
            order = numpy.argsort(key, kind='stable')
            key, w, face_of = key[order], self.w[order], self.face_of[order]
            starts = numpy.flatnonzero(numpy.concatenate([[True], key[1:] != key[:-1]]))
            sums = numpy.zeros((starts.size, 4), ACC)
            with numpy.errstate(invalid='ignore', over='ignore'):
                for q, d in ((0, dv), (2, dt)):
                    t = w * d[face_of]
                    sums[:, q], sums[:, q + 1] = _group_sums(t, starts), _group_sums(numpy.abs(t), starts)
                acc[key[starts]] += sums
        acc = acc.reshape(nrows, nseg, 4)
        with numpy.errstate(invalid='ignore', over='ignore'):
            return self._rows(acc)

    def _rows(self, acc):
        return {'volume': (self._with_totals(acc[..., 0]), self._with_totals(acc[..., 1])),
                'tracer': (self._with_totals(acc[..., 2]), self._with_totals(acc[..., 3]))}
