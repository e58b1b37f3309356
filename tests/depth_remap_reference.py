"""The reference of the transports in true-depth bins of one time step (nf_field_compute_depth_transport), for any grid size:
the terms of tests/resolved_reference.py (_factors, _entries; cell_thickness=True where a cell thickness is set) spread over
the depth rows by the definition below, restated from the weight entries alone.

A term t is one entry (weight slot of one record) at one level z.  The interface depths of its face run over ALL levels:

    D_0 = top,   D_{z+1} = D_z + h_z      one float64 addition per level, z ascending (a sequential loop: it is the definition)
    h_z = fixed(e3u[a]) / fixed(e3v[a]) at the face with a cell thickness, else thickness[z]

    D_z, D_{z+1} or D_{z+1} - D_z not finite         the whole term to row n + 1
    lo = min, hi = max of the two;  lo == hi:        the whole term to row(lo)
    else every row j from row(lo) to row(hi):  left = lo in row(lo) else e[j-1],  right = hi in row(hi) else e[j];
         the share  t * ((right - left) / (hi - lo))  in float64, in that order;  nothing where right == left

row(x): the number of edges <= x -- shares() of tests/class_remap_reference.py.  The shares are summed like the terms of
resolved_reference: per (level, row, segment) in long double, then the levels, then the transect columns from the segments.
`mag` is the sum of |share| over the shares of a value.
"""
import concurrent.futures
import threading

import numpy

from class_remap_reference import shares
from gross_reference import THFILL, THMISSING   # the thickness markers of the sibling tests
from resolved_reference import ACC, ResolvedReference, _term_sums


# the shapes and seeds of the inputs of tests/test_gpu_depth_remap.py (checked without a GPU in tests/test_depth_remap_cpu.py)
GPU_E3_SEED = 83
# its scalar thickness: multiples of 1/8 that float32 holds; the running sums 2.5, 5.5, 8, 10, 13.5, 16.5, 20.5 hit an edge of every
# edge set below (8, 10) and a layer straddles one of every set (16, 20)
GPU_TH = numpy.array([2.5, 3.0, 2.5, 2.0, 3.5, 3.0, 4.0])
EDGES = {2: numpy.array([10., 20.]), 3: numpy.array([8., 16., 24.]), 16: 2. * numpy.arange(16), 1025: numpy.arange(1025) / 32.}


def depth_thickness(real, shape, seed):
    """e3u, e3v of `shape` (1 or nt, nz, ny, nx) on the lattice of the multiples of 1/8 in [0.25, 4]: every running sum is
    exact in float64 and interface depths land exactly on edges that are multiples of 1/32; exactly 0, both markers and NaN
    scattered; no infinity"""
    rng = numpy.random.default_rng(seed)
    dt = numpy.dtype(real).type
    out = []
    for k in range(2):
        a = (rng.integers(2, 33, shape) / 8.).astype(real)
        for m in (0.0, THFILL, THMISSING, numpy.nan):
            a[rng.random(shape) < 0.03] = dt(m)
        out.append(a)
    return out


def depth_intervals(a, b):
    """a, b: the interface depths D_z, D_{z+1} of the terms.  Returns (binned, lo, hi) for shares(): binned False -- a depth or
    the difference is not finite, the whole term to row n + 1; lo == hi -- the whole term to row(lo)"""
    a, b = numpy.asarray(a, dtype=numpy.float64), numpy.asarray(b, dtype=numpy.float64)
    with numpy.errstate(invalid='ignore', over='ignore'):
        fin = numpy.isfinite(a) & numpy.isfinite(b) & numpy.isfinite(b - a)
    return fin, numpy.where(fin, numpy.minimum(a, b), 0.0), numpy.where(fin, numpy.maximum(a, b), 0.0)


class DepthRemapReference(ResolvedReference):
    """ResolvedReference with the rows of the transports in depth bins."""

    def interface_depths(self, values, top=0.0):
        """(nz + 1, faces): D_z of every face, by the sequential float64 loop of the definition"""
        D = numpy.empty((self.nz + 1, self.fa.size), numpy.float64)
        D[0] = numpy.float64(top)
        with numpy.errstate(invalid='ignore', over='ignore'):
            for z in range(self.nz):
                D[z + 1] = D[z] + self._thick(values, z)
        return D

    def depth_step(self, values, edges, top=0.0, tracer=True, levels=None, threads=1):
        """values: the callback of ResolvedReference.step ('uo', 'vo', 'e3u' / 'e3v' with cell_thickness, and 'tracer' with
        tracer=True).  levels = (z0, z1): the terms of those levels only (a rank's slab); the depths are summed from level 0
        all the same; with `threads` > 1 `values` is called from those threads.  Returns {'volume': (want, mag), 'carried': (want, mag) (tracer=True), 'spread_terms': the terms spread
        over more than one row, 'flat_terms': the terms with lo == hi, 'on_edge': the interface depths (faces x levels 1 ..
        nz) that are exactly an edge, 'fraction_error': the largest |sum of a spread term's fractions - 1|}; want and mag have
        shape (len(edges) + 2, row_length), rows [segments | transects]."""
        edges = numpy.asarray(edges, dtype=numpy.float64)
        nrows, nseg = edges.size + 2, self.nseg
        acc = numpy.zeros((nrows * nseg, 4 if tracer else 2), ACC)
        D = self.interface_depths(values, top)
        z0, z1 = (0, self.nz) if levels is None else levels
        stats = {}
        lock = threading.Lock()

        def level(z):
            dv, dt = self._factors(values, z, tracer)[:2]
            tv, tt = self._entries(dv), self._entries(dt)
            fin, lo, hi = depth_intervals(D[z], D[z + 1])
            ent, row, frac = shares(fin[self.face_of], lo[self.face_of], hi[self.face_of], edges)
            key = row * nseg + self.seg[ent]
            order = numpy.argsort(key, kind='stable')
            key = key[order]
            starts = numpy.flatnonzero(numpy.concatenate([[True], key[1:] != key[:-1]])) if key.size else numpy.zeros(0, int)
            sums = _term_sums([tv[ent] * frac, None if tt is None else tt[ent] * frac], starts, order)[:, :acc.shape[1]]
            count = numpy.bincount(ent, minlength=tv.size)
            # the shares of a term are contiguous (shares(): terms ascending): their fractions are added in ACC
            fsum = numpy.zeros(tv.size, ACC)
            if ent.size:
                first = numpy.flatnonzero(numpy.concatenate([[True], ent[1:] != ent[:-1]]))
                fsum[ent[first]] = numpy.add.reduceat(frac.astype(ACC), first)
            spread = count > 1
            stats[z] = (int(spread.sum()), int((fin & (lo == hi))[self.face_of].sum()),
                        float(numpy.abs(fsum[spread] - 1.0).max()) if spread.any() else 0.0)
            with lock:
                acc[key[starts]] += sums

        # the levels are independent once the depths are known: `threads` > 1 works on that many at a time
        if threads > 1:
            with concurrent.futures.ThreadPoolExecutor(threads) as pool:
                list(pool.map(level, range(z0, z1)))
        else:
            for z in range(z0, z1):
                level(z)
        spread_terms, flat_terms = (sum(x[k] for x in stats.values()) for k in (0, 1))
        fraction_error = max([x[2] for x in stats.values()], default=0.0)
        acc = acc.reshape(nrows, nseg, -1)
        out = {'volume': self._pair(acc, 0)}
        if tracer:
            out['carried'] = self._pair(acc, 2)
        out['spread_terms'], out['flat_terms'], out['fraction_error'] = spread_terms, flat_terms, fraction_error
        out['on_edge'] = int(numpy.isin(D[1:], edges).sum())
        return out
