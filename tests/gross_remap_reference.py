"""The reference of the remapped gross class transports of one time step (nf_field_compute_gross_class_remap), for any grid
size: the terms q and c and the sign rule of tests/gross_class_reference.py (gross_reference._gross_terms), the thickness rule of
tests/cellthick_reference.py where a cell thickness is set (resolved_reference with cell_thickness=True, which is all that
module is), and the interval and share rule of tests/class_remap_reference.py (face_intervals, shares), restated from the weight
entries alone.

    per level z and entry:  q the water term, c = q (volume form) or the tracer term (carried form)
    c is spread over the class rows by shares() of the interval between the class field's interface values on the entry's own
    face (levels z - 1 and z + 1 of the array); the shares go to the rows of P where q > 0, of N where q < 0; q == 0: to neither.

The shares  c * fraction  are formed in float64 exactly as stated and summed like the terms of resolved_reference: per (level,
part, row, segment) in long double, then the levels, then the transect columns from the segments.  `mag` is the sum of |share|
over the shares of a value; min_abs_q the smallest non-zero |q| met.

remap_lattice / GPU_*: the inputs of tests/test_gpu_gross_remap.py, made here so that tests/test_gross_remap_cpu.py can say
without a GPU which branches they take.
"""
import threading

import numpy

from class_remap_reference import face_intervals, shares
from gross_reference import GrossReference
from resolved_reference import ACC, _group_sums, _term_sums

# the class-field lattice of tests/test_gpu_class_remap.py (its _lattice, restated: the GPU test holds the two equal), its
# markers and its edge sets
GPU_EDGES = {2: numpy.array([10., 20.]), 3: numpy.array([8., 16., 24.]), 16: 2. * numpy.arange(16), 1025: numpy.arange(1025) / 32.}
GPU_LINES = ["(-100,-80),(100,-80),(0,80)", "(-100,-80),(100,-80),(0,80),(-100,-80)", "(150,-30),(179.5,-20),(179.9,10),(175,40)"]
SFILL, SMISSING = -8888., 5.e15


def remap_lattice(real, shape, own, tracer_marks):
    """values on a 2^-10 lattice in [-2, 32] that grow with z; columns that are constant in z (lo == hi); values on an edge of
    every edge set; NaN and both markers -- the tracer's (own = False: the field is carried too) or its own with +-inf as well"""
    nt, nz, ny, nx = shape
    rng = numpy.random.default_rng(17 + own)
    dt = numpy.dtype(real).type
    x = rng.integers(0, 6 * 1024, shape) / 1024. + 4.5 * numpy.arange(nz)[None, :, None, None] - 2.
    x = numpy.clip(x, -2., 32.).astype(real)
    x[:, :, ::3, ::4] = x[:, 3:4, ::3, ::4]
    x[rng.random(shape) < 0.05] = dt(16.)
    marks = (SFILL, SMISSING, numpy.inf, -numpy.inf) if own else tuple(tracer_marks)
    for m in marks + (numpy.nan,):
        x[rng.random(shape) < 0.03] = dt(m)
    x[:, :, 12:15, 40:50] = dt(marks[0])
    return x


class GrossRemapReference(GrossReference):
    """GrossReference with the rows of the remapped gross class transport."""

    def gross_remap_step(self, values, edges, tracer=True, threads=1, levels=None):
        """values: the callback of ResolvedReference.step ('uo', 'vo', 'class', 'tracer' with tracer=True, 'e3u' / 'e3v' with
        cell_thickness).  levels = (z0, z1): the terms of the levels [z0, z1) only, a rank's rows under a slab range; the
        interface values still come from the levels z - 1 and z + 1 of the array.  Returns {'volume': (want, mag), 'carried': (want, mag) (tracer=True), 'min_abs_q': the smallest
        non-zero |q|, 'spread_terms' / 'flat_terms' / 'on_edge': how many live terms (q != 0) were spread over more than one
        row / had lo == hi with a class value / had an interface value exactly on an edge, 'fraction_error': the largest |sum
        of a spread term's fractions - 1|, 'signs': per segment whether it has a term with q > 0 and one with q < 0, (2, nseg)};
        want and mag have shape (2, len(edges) + 2, row_length): P then N, rows [segments | transects]."""
        edges = numpy.asarray(edges, dtype=numpy.float64)
        nrows, nseg = edges.size + 2, self.nseg
        acc = numpy.zeros((2 * nrows * nseg, 4 if tracer else 2), ACC)
        min_q = [numpy.inf] * self.nz
        stats = [None] * self.nz
        signs = numpy.zeros((2, nseg), bool)
        lock = threading.Lock()

        def level(z):
            if levels is not None and not levels[0] <= z < levels[1]:          # not owned: no term, but its class field is read
                stats[z] = (0, 0, 0, 0.0)
                return
            q, cs, min_q[z] = self._gross_terms(values, z, tracer)
            live = numpy.flatnonzero((q > 0) | (q < 0))                        # only these are spread
            at = lambda zz: self._face_values(values, zz, 'class', self.class_markers)   # noqa: E731
            classed, lo, hi = face_intervals(at(z), at(z - 1) if z > 0 else None, at(z + 1) if z < self.nz - 1 else None)
            fo = self.face_of[live]
            ent, row, frac = shares(classed[fo], lo[fo], hi[fo], edges)
            e = live[ent]                                                      # the entry of every share
            key = (numpy.where(q[e] < 0, nrows, 0) + row) * nseg + self.seg[e]   # (part * (n + 2) + row, segment)
            order = numpy.argsort(key, kind='stable')
            key = key[order]
            starts = numpy.flatnonzero(numpy.concatenate([[True], key[1:] != key[:-1]])) if key.size else numpy.zeros(0, int)
            sums = _term_sums([c[e] * frac for c in cs], starts, order)
            count = numpy.bincount(ent, minlength=live.size)
            # the fractions of a term summed in long double (a term's shares are contiguous: ent ascends), so that what is
            # held to 1 is the fractions and not the rounding of adding up to ~200 of them
            fsum = numpy.zeros(live.size)
            if ent.size:
                first = numpy.flatnonzero(numpy.concatenate([[True], ent[1:] != ent[:-1]]))
                fsum[ent[first]] = _group_sums(frac, first).astype(numpy.float64)
            spread = count > 1
            on_edge = classed[fo] & (numpy.isin(lo[fo], edges) | numpy.isin(hi[fo], edges))
            stats[z] = (int(spread.sum()), int((classed[fo] & (lo[fo] == hi[fo])).sum()), int(on_edge.sum()),
                        float(numpy.abs(fsum[spread] - 1.0).max()) if spread.any() else 0.0)
            with lock:
                acc[key[starts]] += sums
                signs[0, self.seg[live[q[live] > 0]]] = True
                signs[1, self.seg[live[q[live] < 0]]] = True

        self._each_level(level, threads)
        out = self._gross_result(acc.reshape(2, nrows, nseg, -1), min_q)
        out['spread_terms'] = sum(s[0] for s in stats)
        out['flat_terms'] = sum(s[1] for s in stats)
        out['on_edge'] = sum(s[2] for s in stats)
        out['fraction_error'] = max(s[3] for s in stats)
        out['signs'] = signs
        return out
