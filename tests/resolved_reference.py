"""A sparse float64 reference of the six resolved products of one time step, for any grid size.

It restates DESIGN.md section 4 ("Tracer transport", "Volume transport in tracer classes", "Depth- and class-resolved tracer
transports") from the weight entries alone and shares no code with the product.  It needs the raw values only *at the cells
the entries touch*, through a callback, so that it runs on the bench grid as on a toy one.  Written for clarity, not speed.

Definitions.  An entry is (cell c = (j, i), slot, weight w, segment).  Its face belongs to cell `a` and has a second cell `b`:

    east slot   a = c,              b = c + 1        (column nx - 1: column 0 of the row with `wrap`, else none)
    north slot  a = c,              b = c + nx       (last row: none)
    west slot   a = cw = west of c, b = c            (column 0: cw is column nx - 1 of the row; without `wrap` no b)
    south slot  a = cs = c - nx,    b = c            (row 0: the entry carries nothing)

A value is present when it is not NaN and differs from its array's markers, compared in the array's own dtype; from there on
everything is float64.  Face value: 0.5 (a + b), the present one, or none.  Per level z and entry

    volume term  w * (+th_z * fixed(uo[a]) * arcE[a])  for the east and west slots (fixed: 0 where uo is not present)
                 w * (-th_z * fixed(vo[a]) * arcN[a])  for the north and south slots
    tracer term  the same with fixed(.) * tf, tf = carried face value - reference (0 when the face has no carried value)

each times 6.371 in Sverdrup mode.  The row of a term is the number of class edges <= the class field's face value
(`searchsorted(side='right')`); a face without a class value, or with NaN from +inf beside -inf, goes to row nedges + 1.
Several edge sets are served at once: the terms are binned by the union of all edges, and a set's row is the sum of the
union rows between two of its edges.

Summation.  Every value is a sum of such terms; `mag` is the sum of their absolute values.  With an 80-bit numpy.longdouble
(eps 1.1e-19) the terms of a value are added in longdouble in two stages, a level's entries of one segment (the profiles) or
of one (row, segment) (the class rows) and then the levels (the rows and the class rows), so that no chain is longer than
E + nz additions, E = the entries of the longest segment: the summation error is at most (E + nz + S) x 1.1e-19 x mag with
S segments in a transect, i.e. below 2e-15 x mag for a 5400-record segment at 75 levels, plus the final rounding to float64
(1.1e-16 x |value|) and at most 6 roundings inside a term (6.7e-16 x mag).  That is three orders of magnitude inside the
1e-12 x mag bar of the GPU tests.  Where longdouble is no wider than 1e-18 the groups are summed pairwise by numpy.sum in
float64: about log2(E) x 1.1e-16 x mag, 2e-15 x mag at that size.
"""
import concurrent.futures
import threading

import numpy

EARTH_RADIUS_SV = 6371000.0 / 1.e6
_WIDE = numpy.finfo(numpy.longdouble).eps < 1e-18
ACC = numpy.longdouble if _WIDE else numpy.float64


def _group_sums(x, starts):
    """sums over the runs of rows of x that begin at `starts` (ascending, every run non-empty)"""
    if x.shape[0] == 0:
        return numpy.zeros((0,) + x.shape[1:], ACC)
    if _WIDE:
        return numpy.add.reduceat(x, starts, axis=0, dtype=ACC)
    ends = numpy.append(starts[1:], x.shape[0])
    return numpy.array([numpy.sum(x[s:e], axis=0) for s, e in zip(starts, ends)], dtype=ACC)


def _present(x, markers):
    ok = ~numpy.isnan(x)
    for m in markers:
        if m == m:
            ok &= x != x.dtype.type(m)
    return ok


def _face(a, b, has_b, markers):
    """(the face has a value, the value): 0.5 (a + b), the present one, or none"""
    pa, pb = _present(a, markers), has_b & _present(b, markers)
    a64, b64 = a.astype(numpy.float64), b.astype(numpy.float64)
    with numpy.errstate(invalid='ignore', over='ignore'):
        x = numpy.where(pa & pb, 0.5 * (a64 + b64), numpy.where(pa, a64, b64))
    return pa | pb, x


class ResolvedReference(object):
    """cell_slot, weight, segment: the entries of Field.getWeights() (cell x 4 + slot; slots south, east, north, west);
    arc: (ncell, 4) arc lengths (column 1 the east edge, column 2 the north edge); thickness: (nz,); tr_off: the first
    segment of every transect and the number of segments; the markers are pairs (or shorter) of floats, NaN = unused."""

    def __init__(self, cell_slot, weight, segment, arc, thickness, tr_off, nx, ny, uv_markers=(), tracer_markers=(),
                 class_markers=(), reference=0.0, wrap=True, sverdrup=False):
        ce = numpy.asarray(cell_slot, dtype=numpy.int64)
        nx, ny = int(nx), int(ny)
        # row 0's south slot carries nothing: those entries are dropped; the others go segment by segment, in their order
        kept = numpy.flatnonzero(~((ce % 4 == 0) & (ce // 4 < nx)))
        order = kept[numpy.argsort(numpy.asarray(segment)[kept], kind='stable')]
        ce = ce[order]
        self.w = numpy.asarray(weight, dtype=numpy.float64)[order]
        self.seg = numpy.asarray(segment, dtype=numpy.int64)[order]
        self.tr_off = numpy.asarray(tr_off, dtype=numpy.int64)
        self.nseg = int(self.tr_off[-1])
        self.row_length = self.nseg + self.tr_off.size - 1
        self.thickness = numpy.asarray(thickness, dtype=numpy.float64)
        self.nz = self.thickness.size
        self.uv_markers, self.tracer_markers, self.class_markers = tuple(uv_markers), tuple(tracer_markers), tuple(class_markers)
        self.reference = float(reference)
        self.scale = EARTH_RADIUS_SV if sverdrup else None
        c, slot = ce // 4, ce % 4
        j, i = c // nx, c % nx
        south, east, north, west = slot == 0, slot == 1, slot == 2, slot == 3
        a = numpy.select([south, west], [c - nx, numpy.where(i > 0, c - 1, c - 1 + nx)], c)   # the cell whose face the slot is
        # the entries of a slot pair (east of cw = west of c, north of cs = south of c) share their face: the terms' factors
        # are formed once per face (cell a, east or north) and level
        face, self.face_of = numpy.unique(2 * a + (east | west), return_inverse=True)
        self.face_of = self.face_of.reshape(-1)
        self.fa, self.f_is_u = face // 2, face % 2 == 1
        fj, fi = self.fa // nx, self.fa % nx
        east_of = numpy.where(fi < nx - 1, self.fa + 1, self.fa + 1 - nx)
        self.fb = numpy.where(self.f_is_u, east_of, numpy.minimum(self.fa + nx, nx * ny - 1))
        self.f_has_b = numpy.where(self.f_is_u, (fi < nx - 1) | bool(wrap), fj < ny - 1)
        arc = numpy.asarray(arc, dtype=numpy.float64).reshape(-1, 4)
        self.f_arc = numpy.where(self.f_is_u, arc[self.fa, 1], -arc[self.fa, 2])   # signed: +arcE for uo, -arcN for vo
        self.cells = numpy.unique(numpy.concatenate([self.fa, self.fb]))            # the cells whose values are needed
        self.ia, self.ib = numpy.searchsorted(self.cells, self.fa), numpy.searchsorted(self.cells, self.fb)
        self.useg, self.seg_starts = numpy.unique(self.seg, return_index=True)

    # ---- reductions ------------------------------------------------------------------------------------------------------
    def _with_totals(self, a):
        """(..., nseg) -> (..., row_length) in float64: [segments | transects]"""
        o = self.tr_off
        tot = [a[..., o[p]:o[p + 1]].sum(axis=-1, dtype=ACC)[..., None] for p in range(o.size - 1)]
        return numpy.concatenate([a] + tot, axis=-1).astype(numpy.float64)

    @staticmethod
    def _term_sums(w, face_of, dv, dt, starts):
        """the terms w * dv[face_of], w * dt[face_of] and their absolute values, each summed over the runs that begin at
        `starts`: (runs, 4) = volume, sum |volume terms|, tracer, sum |tracer terms|"""
        out = numpy.zeros((starts.size, 4), ACC)
        for q, d in ((0, dv), (2, dt)):
            if d is None:
                continue
            t = w * d[face_of]
            out[:, q], out[:, q + 1] = _group_sums(t, starts), _group_sums(numpy.abs(t), starts)
        return out

    # ---- one step ----------------------------------------------------------------------------------------------------------
    def step(self, values, edge_sets=(), threads=1, volume_classes=True):
        """values(name, z, cells) -> the raw values of 'uo', 'vo', 'tracer' (carried) or 'class' (class field) of level z at
        the flat cell indices `cells`, in the array's dtype.  Returns a dict of (want, mag) pairs of [segments | transects]
        rows: 'volume' and 'tracer' (row_length,), 'volume_profile' and 'tracer_profile' (nz, row_length), and for every k
        ('volume_classes', k) and ('tracer_classes', k), (len(edge_sets[k]) + 2, row_length).  The levels are independent
        until they are added up; `threads` > 1 works on that many at a time (`values` is then called from those threads).
        volume_classes=False leaves the 'volume_classes' rows out (they are not in the result)."""
        n, nseg, nz = self.w.size, self.nseg, self.nz
        edge_sets = [numpy.asarray(e, dtype=numpy.float64) for e in edge_sets]
        # last axis: volume, sum |volume terms|, tracer, sum |tracer terms|
        prof = numpy.zeros((nz, nseg, 4), ACC)
        # every set's row follows from the row among the union of all edges, so the terms are binned once per level
        union = numpy.unique(numpy.concatenate(edge_sets)) if edge_sets else numpy.zeros(0)
        fine = numpy.zeros(((union.size + 2) * nseg, 4), ACC)
        lock = threading.Lock()

        def level(z):
            uo, vo = values('uo', z, self.cells), values('vo', z, self.cells)
            tau, sig = values('tracer', z, self.cells), values('class', z, self.cells)
            fixed_u = numpy.where(_present(uo, self.uv_markers), uo.astype(numpy.float64), 0.0)
            fixed_v = numpy.where(_present(vo, self.uv_markers), vo.astype(numpy.float64), 0.0)
            vel = numpy.where(self.f_is_u, fixed_u[self.ia], fixed_v[self.ia])
            has_t, xt = _face(tau[self.ia], tau[self.ib], self.f_has_b, self.tracer_markers)
            with numpy.errstate(invalid='ignore'):
                tf = numpy.where(has_t, numpy.where(has_t, xt, 0.0) - self.reference, 0.0)
            th = self.thickness[z]
            dv, dt = (th * vel) * self.f_arc, (th * (vel * tf)) * self.f_arc
            if self.scale is not None:
                dv, dt = dv * self.scale, dt * self.scale
            prof[z][self.useg] = self._term_sums(self.w, self.face_of, dv, dt, self.seg_starts)
            if not edge_sets:
                return
            has_s, xs = _face(sig[self.ia], sig[self.ib], self.f_has_b, self.class_markers)
            classed = has_s & ~numpy.isnan(xs)
            r_face = numpy.where(classed, numpy.searchsorted(union, numpy.where(classed, xs, 0.0), side='right'), union.size + 1)
            # entries are in segment order: a stable sort by row leaves every (row, segment) group contiguous
            order = numpy.argsort(r_face.astype(numpy.int16)[self.face_of], kind='stable')
            face_of, seg = self.face_of[order], self.seg[order]
            key = r_face[face_of] * nseg + seg
            starts = numpy.flatnonzero(numpy.concatenate([[True], key[1:] != key[:-1]])) if n else numpy.zeros(0, int)
            sums = self._term_sums(self.w[order], face_of, dv if volume_classes else None, dt, starts)
            with lock:
                fine[key[starts]] += sums                                    # key[starts] has no repeats

        if threads > 1:
            with concurrent.futures.ThreadPoolExecutor(threads) as pool:
                list(pool.map(level, range(nz)))
        else:
            for z in range(nz):
                level(z)

        def pair(a, q):
            """columns q (values) and q + 1 (sum of |terms|) of a (..., nseg, 4) as [segments | transects] float64 rows"""
            return self._with_totals(a[..., q]), self._with_totals(a[..., q + 1])

        out = {}
        sums = prof.sum(axis=0, dtype=ACC)
        out['volume'], out['tracer'] = pair(sums, 0), pair(sums, 2)
        out['volume_profile'], out['tracer_profile'] = pair(prof, 0), pair(prof, 2)
        fine = fine.reshape(union.size + 2, nseg, 4)
        for k, e in enumerate(edge_sets):
            # union row q > 0 holds the values in [union[q - 1], union[q]): as many edges of e are <= them as are <= union[q - 1]
            row_of = numpy.concatenate([[0], numpy.searchsorted(e, union, side='right'), [e.size + 1]])
            acc = numpy.zeros((e.size + 2, nseg, 4), ACC)
            for q in range(union.size + 2):
                acc[row_of[q]] += fine[q]
            out['tracer_classes', k] = pair(acc, 2)
            if volume_classes:
                out['volume_classes', k] = pair(acc, 0)
        return out


def array_values(arrays, t):
    """the `values` callback for host arrays {'uo': (nt, nz, ny, nx), ...} at step t"""
    def values(name, z, cells):
        return arrays[name][t, z].reshape(-1)[cells]
    return values
