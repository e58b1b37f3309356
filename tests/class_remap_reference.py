"""The reference of the conservative (piecewise-linear) remapping of the class transport of one time step
(nf_field_compute_class_remap), for any grid size: the terms of tests/resolved_reference.py (_factors, _entries) spread over the
class rows by the definition below, restated from the weight entries alone.

A term t is one entry (weight slot of one record) at one level z; f_z is the class field's face value there (face rule and
markers of resolved_reference; class_markers).

    no class value at z, or NaN                      the whole term to row n + 1
    g_up = 0.5 (f_{z-1} + f_z)   where z > 0 and the face has a class value at level z - 1, else f_z
    g_dn = 0.5 (f_{z+1} + f_z)   where z < nz - 1 and it has one at level z + 1, else f_z
    g_up, g_dn or g_dn - g_up not finite             the whole term to row(f_z)               (the step rule)
    lo = min(g_up, g_dn), hi = max(g_up, g_dn);  lo == hi:  the whole term to row(lo)
    else every row j from row(lo) to row(hi):  left = lo in row(lo) else e[j-1],  right = hi in row(hi) else e[j];
         the share  t * ((right - left) / (hi - lo))  in float64, in that order;  nothing where right == left

row(x): the number of edges <= x.  The shares are formed in float64 exactly as stated -- they are the definition -- and summed
like the terms of resolved_reference: per (level, row, segment) in long double, then the levels, then the transect columns from
the segments.  `mag` is the sum of |share| over the shares of a value.
"""
import threading

import numpy

from resolved_reference import ACC, ResolvedReference, _term_sums


def face_intervals(cur, up, dn):
    """cur, up, dn: (has, value) of the faces at level z, z - 1 and z + 1 (None: there is no such level).  Returns (classed,
    lo, hi): classed False -- no class value; lo == hi -- the whole term to row(lo) (f_z itself under the step rule)."""
    has, f = cur
    classed = has & ~numpy.isnan(f)
    f = numpy.where(classed, f, 0.0)
    with numpy.errstate(invalid='ignore', over='ignore'):
        gu = f if up is None else numpy.where(up[0], 0.5 * (up[1] + f), f)
        gd = f if dn is None else numpy.where(dn[0], 0.5 * (dn[1] + f), f)
        fin = numpy.isfinite(gu) & numpy.isfinite(gd) & numpy.isfinite(gd - gu)
        lo = numpy.where(fin, numpy.minimum(gu, gd), f)
        hi = numpy.where(fin, numpy.maximum(gu, gd), f)
    return classed, lo, hi


def shares(classed, lo, hi, edges):
    """per term (classed, lo, hi) -> the (term index, row, fraction) of every share, terms ascending and rows ascending inside
    a term; fraction is exactly 1.0 for a term that goes whole to one row"""
    n = edges.size
    jlo = numpy.where(classed, numpy.searchsorted(edges, lo, side='right'), n + 1)
    jhi = numpy.where(classed, numpy.searchsorted(edges, hi, side='right'), n + 1)
    cnt = jhi - jlo + 1
    first = numpy.cumsum(cnt) - cnt
    ent = numpy.repeat(numpy.arange(cnt.size), cnt)
    j = jlo[ent] + numpy.arange(ent.size) - first[ent]
    whole = (lo == hi)[ent] | ~classed[ent]
    left = numpy.where(j == jlo[ent], lo[ent], edges[numpy.clip(j - 1, 0, n - 1)])
    right = numpy.where(j == jhi[ent], hi[ent], edges[numpy.clip(j, 0, n - 1)])
    with numpy.errstate(invalid='ignore', divide='ignore'):
        frac = numpy.where(whole, 1.0, (right - left) / (hi - lo)[ent])
    keep = whole | (right != left)
    return ent[keep], j[keep], frac[keep]


class ClassRemapReference(ResolvedReference):
    """ResolvedReference with the rows of the remapped class transport."""

    def remap_step(self, values, edges, tracer=True, threads=1):
        """values: the callback of ResolvedReference.step ('uo', 'vo', 'class', and 'tracer' with tracer=True).  Returns
        {'volume': (want, mag), 'carried': (want, mag) (tracer=True), 'rows_per_term': the mean number of rows a classed term
        with a non-zero volume value reaches, 'spread_terms': how many terms were spread over more than one row,
        'fraction_error': the largest |sum of a spread term's fractions - 1|}; want and mag have shape (len(edges) + 2,
        row_length), rows [segments | transects]."""
        edges = numpy.asarray(edges, dtype=numpy.float64)
        nrows, nseg = edges.size + 2, self.nseg
        acc = numpy.zeros((nrows * nseg, 4 if tracer else 2), ACC)
        stats = [None] * self.nz
        lock = threading.Lock()

        def level(z):
            dv, dt = self._factors(values, z, tracer)[:2]
            tv, tt = self._entries(dv), self._entries(dt)
            at = lambda zz: self._face_values(values, zz, 'class', self.class_markers)   # noqa: E731
            classed, lo, hi = face_intervals(at(z), at(z - 1) if z > 0 else None, at(z + 1) if z < self.nz - 1 else None)
            ent, row, frac = shares(classed[self.face_of], lo[self.face_of], hi[self.face_of], edges)
            key = row * nseg + self.seg[ent]
            order = numpy.argsort(key, kind='stable')
            key = key[order]
            starts = numpy.flatnonzero(numpy.concatenate([[True], key[1:] != key[:-1]])) if key.size else numpy.zeros(0, int)
            sums = _term_sums([tv[ent] * frac, None if tt is None else tt[ent] * frac], starts, order)[:, :acc.shape[1]]
            count = numpy.bincount(ent, minlength=tv.size)
            fsum = numpy.bincount(ent, weights=frac, minlength=tv.size)
            spread = count > 1
            live = classed[self.face_of] & (tv != 0)
            stats[z] = (int(count[live].sum()), int(live.sum()), int(spread.sum()),
                        float(numpy.abs(fsum[spread] - 1.0).max()) if spread.any() else 0.0)
            with lock:
                acc[key[starts]] += sums

        self._each_level(level, threads)
        acc = acc.reshape(nrows, nseg, -1)
        out = {'volume': self._pair(acc, 0)}
        if tracer:
            out['carried'] = self._pair(acc, 2)
        reached, live = sum(s[0] for s in stats), sum(s[1] for s in stats)
        out['rows_per_term'] = reached / max(live, 1)
        out['spread_terms'] = sum(s[2] for s in stats)
        out['fraction_error'] = max(s[3] for s in stats)
        return out
