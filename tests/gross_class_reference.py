"""A sparse float64 / long-double reference of the gross transports in tracer classes of one time step
(nf_field_compute_gross_class_transport), for any grid size: the definition of include/nemoflux_amd.h restated in numpy over
the cells the weight entries touch.  It uses the entry / face bookkeeping, the face rule and the summation of
tests/resolved_reference.py and the terms of tests/gross_reference.py, and shares no code with the product.

Per level z and entry (cell c, slot, weight w, segment), with the face of the slot as in tests/resolved_reference.py:

    water term    q = w * ((th * fixed(vel)) * arc)             as in tests/gross_reference.py (th: scalar or at the face)
    carried term  c = q                                         (volume form)
                  c = w * ((th * (fixed(vel) * tf)) * arc)      (carried form; tf = the carried tracer's face value - reference)
    row           r = the number of class edges <= the class field's raw face value; n + 1 for a face without a class value
                      (or with NaN from +inf beside -inf)

    P[r] = sum of c over the entries of row r with q > 0,    N[r] = sum of c over those with q < 0;    q == 0: in neither.

The callback serves 'uo', 'vo', 'class' (the class field: its markers are class_markers), 'tracer' (the carried tracer, with
tracer=True; markers tracer_markers) and 'e3u', 'e3v' with cell thicknesses.  Terms are formed in float64 and summed in long
double: a level's entries of one (part, row, segment), then the levels, then the transect columns from the segments.  `mag` is
the sum of |c| over the entries of the value; min_abs_q the smallest non-zero |q| met.
"""
import concurrent.futures
import threading

import numpy

from gross_reference import GrossReference
from resolved_reference import ACC, _face, _group_sums, _present


class GrossClassReference(GrossReference):
    """GrossReference with the rows of the gross class transport."""

    def gross_class_step(self, values, edges, tracer=True, threads=1):
        """Returns {'volume': (want, mag), 'carried': (want, mag) (tracer=True), 'min_abs_q': float}; want and mag have shape
        (2, len(edges) + 2, row_length): P then N, rows [segments | transects]."""
        edges = numpy.asarray(edges, dtype=numpy.float64)
        nrows, nseg = edges.size + 2, self.nseg
        forms = ('volume', 'carried') if tracer else ('volume',)
        acc = {nm: numpy.zeros((2 * nrows * nseg, 2), ACC) for nm in forms}    # last axis: the sum, the sum of |terms|
        min_q = [numpy.inf] * self.nz
        lock = threading.Lock()

        def level(z):
            uo, vo = values('uo', z, self.cells), values('vo', z, self.cells)
            fu = numpy.where(_present(uo, self.uv_markers), uo.astype(numpy.float64), 0.0)
            fv = numpy.where(_present(vo, self.uv_markers), vo.astype(numpy.float64), 0.0)
            vel = numpy.where(self.f_is_u, fu[self.ia], fv[self.ia])
            if self.cell_thickness:
                e3u, e3v = values('e3u', z, self.cells), values('e3v', z, self.cells)
                tu = numpy.where(_present(e3u, self.thick_markers), e3u.astype(numpy.float64), 0.0)
                tv = numpy.where(_present(e3v, self.thick_markers), e3v.astype(numpy.float64), 0.0)
                th = numpy.where(self.f_is_u, tu[self.ia], tv[self.ia])
            else:
                th = self.thickness[z]
            d = {'volume': (th * vel) * self.f_arc}
            if tracer:
                tau = values('tracer', z, self.cells)
                has_t, xt = _face(tau[self.ia], tau[self.ib], self.f_has_b, self.tracer_markers)
                with numpy.errstate(invalid='ignore'):
                    tf = numpy.where(has_t, numpy.where(has_t, xt, 0.0) - self.reference, 0.0)
                d['carried'] = (th * (vel * tf)) * self.f_arc
            if self.scale is not None:
                d = {nm: x * self.scale for nm, x in d.items()}
            sig = values('class', z, self.cells)
            has_s, xs = _face(sig[self.ia], sig[self.ib], self.f_has_b, self.class_markers)
            classed = has_s & ~numpy.isnan(xs)
            r_face = numpy.where(classed, numpy.searchsorted(edges, numpy.where(classed, xs, 0.0), side='right'), edges.size + 1)
            q = self.w * d['volume'][self.face_of]                            # per entry
            live = numpy.flatnonzero(q != 0)
            if not live.size:
                return
            min_q[z] = float(numpy.abs(q[live]).min())
            row = numpy.where(q[live] < 0, nrows, 0) + r_face[self.face_of[live]]          # part * (n + 2) + r
            # the entries are in segment order: a stable sort by row leaves every (row, segment) group contiguous
            order = numpy.argsort(row, kind='stable')
            live, key = live[order], row[order] * nseg + self.seg[live[order]]
            starts = numpy.flatnonzero(numpy.concatenate([[True], key[1:] != key[:-1]]))
            for nm in forms:
                c = q[live] if nm == 'volume' else (self.w * d[nm][self.face_of])[live]
                sums = numpy.zeros((starts.size, 2), ACC)
                sums[:, 0], sums[:, 1] = _group_sums(c, starts), _group_sums(numpy.abs(c), starts)
                with lock:
                    acc[nm][key[starts]] += sums                              # key[starts] has no repeats

        if threads > 1:
            with concurrent.futures.ThreadPoolExecutor(threads) as pool:
                list(pool.map(level, range(self.nz)))
        else:
            for z in range(self.nz):
                level(z)
        res = {}
        for nm in forms:
            a = acc[nm].reshape(2, nrows, nseg, 2)
            res[nm] = (self._with_totals(a[..., 0]), self._with_totals(a[..., 1]))
        res['min_abs_q'] = min(min_q)
        return res
