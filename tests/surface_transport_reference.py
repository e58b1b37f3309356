"""The reference of the transports between surfaces of one time step (nf_field_compute_surface_transport), for any grid size:
the terms of tests/resolved_reference.py (_factors, _entries; cell_thickness=True where a cell thickness is set) and the
interface depths of tests/depth_remap_reference.py (the sequential loop of DepthRemapReference.interface_depths), spread over the
rows by the definition below with one edge set PER FACE, restated from the weight entries alone.

The m surfaces are 2-D fields at T-points.  A surface's value at a face is the class-field rule of resolved_reference._face with
the surfaces' own markers and wrap: 0.5 (a + b), the present one, or none.  With x_1 .. x_m the face values of a face:

    any x_k without a value or not finite            every term of the face whole to row m + 1, at every level
    else  e_1 = x_1,  e_k = max(e_{k-1}, x_k)        (non-decreasing: a surface above the one before it is taken at that one)

A term t is one entry at one level z, D_z and D_{z+1} the interface depths of its face:

    D_z, D_{z+1} or D_{z+1} - D_z not finite         the whole term to row m + 1
    lo = min, hi = max of the two;  lo == hi:        the whole term to row(lo)
    else every row j from row(lo) to row(hi):  left = lo in row(lo) else e_j,  right = hi in row(hi) else e_{j+1}  (1-based e);
         the share  t * ((right - left) / (hi - lo))  in float64, in that order;  nothing where right == left

row(x): the number of e_k <= x.  The shares are summed like the terms of resolved_reference: per (level, row, segment) in long
double, then the levels, then the transect columns from the segments.  `mag` is the sum of |share| over the shares of a value.
"""
import numpy

from depth_remap_reference import DepthRemapReference, depth_intervals
from resolved_reference import ACC, _face, _term_sums

# the surfaces' own markers in the tests: outside the range of the recipe, exact in float32
SFILL, SMISSING = -999., 1.0e20
GPU_SURFACE_SEED = 91
GPU_M = (1, 2, 3, 8)


def gpu_case(k, thick_index, nt=3):
    """case k of tests/test_gpu_surface_transport.py under thickness form `thick_index` (0 scalar, 1 static, 2 time-varying):
    (m, the time step, `top`, the steps of the surfaces) -- every m meets a static and a time-varying set, each step and both tops"""
    return GPU_M[k], k % nt, (0.0 if k % 2 == 0 else -1.5), (1 if (k + thick_index) % 2 == 0 else nt)


def surface_fields(real, shape, m, seed=GPU_SURFACE_SEED):
    """(shape[0], m, ny, nx) of dtype `real`, shape = (nt_s, ny, nx): surface k = 0 .. m - 1 is
    floor(8 * 0.75 * (24 / m) * k) / 8 + integers(0, 8 * 24 / m) / 8 -- all inside [0, 24], the depths of the sibling tests'
    columns; multiples of 1/8, so every face average is exact in float64 and lands on interface depths that are multiples of
    1/8; a surface's band overlaps the next one's by a quarter, so that one rises above the one before it here and there.  Each of
    the two markers and NaN is scattered with probability 0.02, +inf with 0.005."""
    rng = numpy.random.default_rng(seed)
    dt = numpy.dtype(real).type
    nt_s, ny, nx = shape
    out = numpy.empty((nt_s, m, ny, nx), real)
    for k in range(m):
        a = (numpy.floor(8. * 0.75 * (24. / m) * k) / 8. + rng.integers(0, int(8 * 24 / m), shape) / 8.).astype(real)
        for mark in (SFILL, SMISSING, numpy.nan):
            a[rng.random(shape) < 0.02] = dt(mark)
        a[rng.random(shape) < 0.005] = dt(numpy.inf)
        out[:, k] = a
    return out


def shares(binned, lo, hi, E):
    """per term (binned, lo, hi) and its own edges E[:, term] (m, terms; non-decreasing down a column) -> the (term index, row,
    fraction) of every share, terms ascending and rows ascending inside a term; fraction is exactly 1.0 for a term that goes
    whole to one row.  binned False: whole to row m + 1."""
    m = E.shape[0]
    jlo = numpy.where(binned, (E <= lo[None]).sum(axis=0), m + 1)
    jhi = numpy.where(binned, (E <= hi[None]).sum(axis=0), m + 1)
    cnt = jhi - jlo + 1
    first = numpy.cumsum(cnt) - cnt
    ent = numpy.repeat(numpy.arange(cnt.size), cnt)
    j = jlo[ent] + numpy.arange(ent.size) - first[ent]
    whole = (lo == hi)[ent] | ~binned[ent]
    left = numpy.where(j == jlo[ent], lo[ent], E[numpy.clip(j - 1, 0, m - 1), ent])
    right = numpy.where(j == jhi[ent], hi[ent], E[numpy.clip(j, 0, m - 1), ent])
    with numpy.errstate(invalid='ignore', divide='ignore'):
        frac = numpy.where(whole, 1.0, (right - left) / (hi - lo)[ent])
    keep = whole | (right != left)
    return ent[keep], j[keep], frac[keep]


class SurfaceReference(DepthRemapReference):
    """DepthRemapReference with the rows of the transports between surfaces.  surface_markers, surface_wrap: the surfaces' own
    markers and wrap rule; the other arguments are ResolvedReference's."""

    def __init__(self, cell_slot, weight, segment, arc, thickness, tr_off, nx, ny, surface_markers=(), surface_wrap=True, **kw):
        super().__init__(cell_slot, weight, segment, arc, thickness, tr_off, nx, ny, **kw)
        nx, ny = int(nx), int(ny)
        self.surface_markers = tuple(surface_markers)
        fj, fi = self.fa // nx, self.fa % nx
        self.s_has_b = numpy.where(self.f_is_u, (fi < nx - 1) | bool(surface_wrap), fj < ny - 1)

    def face_edges(self, values, m):
        """(ok, E, acted) per face: ok -- every surface has a finite value there; E (m, faces) -- the running max of the face
        values (0 where not ok); acted -- the running max changed a value"""
        X = numpy.zeros((m, self.fa.size))
        ok = numpy.ones(self.fa.size, bool)
        for k in range(m):
            x = values('surface', k, self.cells)
            has, f = _face(x[self.ia], x[self.ib], self.s_has_b, self.surface_markers)
            has = has & numpy.isfinite(numpy.where(has, f, 0.0))
            ok &= has
            X[k] = numpy.where(has, f, 0.0)
        X = numpy.where(ok[None], X, 0.0)
        E = numpy.maximum.accumulate(X, axis=0)
        return ok, E, ok & (E != X).any(axis=0)

    def surface_step(self, values, m, top=0.0, tracer=True, levels=None):
        """values: the callback of ResolvedReference.step ('uo', 'vo', 'e3u' / 'e3v' with cell_thickness, 'tracer' with
        tracer=True) that also serves ('surface', k, cells): surface k = 0 .. m - 1 at the flat cell indices.  levels =
        (z0, z1): the terms of those levels only; the depths are summed from level 0 all the same.  Returns {'volume': (want,
        mag), 'carried': (want, mag) (tracer=True)} of shape (m + 2, row_length), rows [segments | transects], and the counters
        'spread_terms' (terms spread over more than one row), 'flat_terms' (terms with lo == hi), 'on_edge' (interface depths,
        faces x levels 1 .. nz, exactly on an edge of their face), 'max_acted' (faces where the running max acted), 'unbinned'
        (faces sent to row m + 1 for want of an edge set), 'faces', 'fraction_error' (the largest |sum of a spread term's
        fractions - 1|)."""
        nrows, nseg = m + 2, self.nseg
        acc = numpy.zeros((nrows * nseg, 4 if tracer else 2), ACC)
        D = self.interface_depths(values, top)
        ok, E, acted = self.face_edges(values, m)
        Et = E[:, self.face_of]
        z0, z1 = (0, self.nz) if levels is None else levels
        spread_terms = flat_terms = 0
        fraction_error = 0.0
        for z in range(z0, z1):
            dv, dt = self._factors(values, z, tracer)[:2]
            tv, tt = self._entries(dv), self._entries(dt)
            fin, lo, hi = depth_intervals(D[z], D[z + 1])
            fin = fin & ok
            ent, row, frac = shares(fin[self.face_of], lo[self.face_of], hi[self.face_of], Et)
            key = row * nseg + self.seg[ent]
            order = numpy.argsort(key, kind='stable')
            key = key[order]
            starts = numpy.flatnonzero(numpy.concatenate([[True], key[1:] != key[:-1]])) if key.size else numpy.zeros(0, int)
            sums = _term_sums([tv[ent] * frac, None if tt is None else tt[ent] * frac], starts, order)[:, :acc.shape[1]]
            count = numpy.bincount(ent, minlength=tv.size)
            fsum = numpy.zeros(tv.size, ACC)
            if ent.size:
                first = numpy.flatnonzero(numpy.concatenate([[True], ent[1:] != ent[:-1]]))
                fsum[ent[first]] = numpy.add.reduceat(frac.astype(ACC), first)
            spread = count > 1
            spread_terms += int(spread.sum())
            flat_terms += int((fin & (lo == hi))[self.face_of].sum())
            if spread.any():
                fraction_error = max(fraction_error, float(numpy.abs(fsum[spread] - 1.0).max()))
            acc[key[starts]] += sums
        acc = acc.reshape(nrows, nseg, -1)
        out = {'volume': self._pair(acc, 0)}
        if tracer:
            out['carried'] = self._pair(acc, 2)
        out.update(spread_terms=spread_terms, flat_terms=flat_terms, fraction_error=fraction_error,
                   on_edge=int(((D[1:, None, :] == E[None]) & ok[None, None]).any(axis=1).sum()),
                   max_acted=int(acted.sum()), unbinned=int((~ok).sum()), faces=int(ok.size))
        return out


def surface_values(arrays, t):
    """the `values` callback of gross_reference.array_values extended by 'surface': arrays['surface'] is (nt_s, m, ny, nx) and
    the level argument of the callback is the surface's index"""
    def values(name, z, cells):
        a = arrays[name]
        return a[t if a.shape[0] > 1 else 0, z].reshape(-1)[cells]
    return values
