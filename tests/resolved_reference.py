"""A sparse float64 reference of the per-step transect products, for any grid size: the model that every *_reference module
of this directory is built from.

It restates DESIGN.md section 4 ("Tracer transport", "Volume transport in tracer classes", "Depth- and class-resolved tracer
transports") from the weight entries alone and shares no code with the product.  It needs the raw values only *at the cells
the entries touch*, through a callback, so that it runs on the bench grid as on a toy one.  Written for clarity, not speed.
ResolvedReference states every rule below once; the product classes (this one's `step`, section_reference, gross_reference,
gross_class_reference, joint_class_reference) add only what is their own.

Definitions.  An entry is (cell c = (j, i), slot, weight w, segment).  Its face belongs to cell `a` and has a second cell `b`:

    east slot   a = c,              b = c + 1        (column nx - 1: column 0 of the row with `wrap`, else none)
    north slot  a = c,              b = c + nx       (last row: none)
    west slot   a = cw = west of c, b = c            (column 0: cw is column nx - 1 of the row; without `wrap` no b)
    south slot  a = cs = c - nx,    b = c            (row 0: the entry carries nothing and is dropped)

A value is present when it is not NaN and differs from its array's markers, compared in the array's own dtype; from there on
everything is float64.  fixed(x): x where present, else 0.  Face value: 0.5 (a + b), the present one, or none.  Per level z
and entry

    volume term  w * ((th * fixed(uo[a])) * arcE[a])   for the east and west slots
                 w * ((th * fixed(vo[a])) * -arcN[a])  for the north and south slots
    tracer term  the same with fixed(.) * tf, tf = carried face value - reference (0 when the face has no carried value)

each times 6.371 in Sverdrup mode.  th is thickness[z], or with cell_thickness=True fixed(e3u[a]) for the east and west
slots, fixed(e3v[a]) for the others, with the markers thick_markers; whether the thickness varies in time is up to the
callback (array_values: an array with one step is static).  The class row of a term is the number of class edges <= the class
field's face value (`searchsorted(side='right')`); a face without a class value, or with NaN from +inf beside -inf, goes to
row nedges + 1.  `step` serves several edge sets at once: the terms are binned by the union of all edges, and a set's row is
the sum of the union rows between two of its edges.

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


def _term_sums(terms, starts, pick=None):
    """per-entry terms (None: all zero), optionally gathered at `pick`, summed over the runs that begin at `starts`:
    (runs, 2 len(terms)) = for every term its sum and the sum of its absolute values"""
    out = numpy.zeros((starts.size, 2 * len(terms)), ACC)
    for k, t in enumerate(terms):
        if t is not None:
            t = t if pick is None else t[pick]
            out[:, 2 * k], out[:, 2 * k + 1] = _group_sums(t, starts), _group_sums(numpy.abs(t), starts)
    return out


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


def class_rows(has, x, edges):
    """the class row of the face values x (has: the face has a value): the number of edges <= x, or len(edges) + 1"""
    classed = has & ~numpy.isnan(x)
    return numpy.where(classed, numpy.searchsorted(edges, numpy.where(classed, x, 0.0), side='right'), edges.size + 1)


class ResolvedReference(object):
    """cell_slot, weight, segment: the entries of Field.getWeights() (cell x 4 + slot; slots south, east, north, west);
    arc: (ncell, 4) arc lengths (column 1 the east edge, column 2 the north edge); thickness: (nz,); tr_off: the first
    segment of every transect and the number of segments; the markers are pairs (or shorter) of floats, NaN = unused.
    cell_thickness=True: the thickness is read at the face ('e3u', 'e3v' of the callback, markers thick_markers) and
    `thickness` gives the number of levels only."""

    def __init__(self, cell_slot, weight, segment, arc, thickness, tr_off, nx, ny, uv_markers=(), tracer_markers=(),
                 class_markers=(), reference=0.0, wrap=True, sverdrup=False, thick_markers=(), cell_thickness=False):
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
        self.thick_markers, self.cell_thickness = tuple(thick_markers), bool(cell_thickness)
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

    # ---- the rules of the model, per level: values per face ------------------------------------------------------------------
    def _fixed(self, values, z, u_name, v_name, markers):
        """fixed(u_name[a]) for the east faces, fixed(v_name[a]) for the north faces"""
        def fixed(name):
            x = values(name, z, self.cells)
            return numpy.where(_present(x, markers), x.astype(numpy.float64), 0.0)[self.ia]
        return numpy.where(self.f_is_u, fixed(u_name), fixed(v_name))

    def _thick(self, values, z):
        return self._fixed(values, z, 'e3u', 'e3v', self.thick_markers) if self.cell_thickness else self.thickness[z]

    def _face_values(self, values, z, name, markers):
        """(the face has a value, the value) of the field `name`"""
        x = values(name, z, self.cells)
        return _face(x[self.ia], x[self.ib], self.f_has_b, markers)

    def _class_rows(self, values, z, edges):
        return class_rows(*self._face_values(values, z, 'class', self.class_markers), edges)

    def _factors(self, values, z, tracer=True):
        """(dv, dt, has, x): a term is w * dv (volume) or w * dt (tracer) of its face; (has, x) is the carried tracer's
        face value.  tracer=False: dt, has and x are None and 'tracer' is not fetched."""
        vel, th = self._fixed(values, z, 'uo', 'vo', self.uv_markers), self._thick(values, z)
        dv, dt, has, x = (th * vel) * self.f_arc, None, None, None
        if tracer:
            has, x = self._face_values(values, z, 'tracer', self.tracer_markers)
            with numpy.errstate(invalid='ignore'):
                tf = numpy.where(has, numpy.where(has, x, 0.0) - self.reference, 0.0)
            dt = (th * (vel * tf)) * self.f_arc
        if self.scale is not None:
            dv, dt = dv * self.scale, None if dt is None else dt * self.scale
        return dv, dt, has, x

    def _entries(self, d):
        """per face -> per entry, times the weight"""
        return None if d is None else self.w * d[self.face_of]

    # ---- reductions ------------------------------------------------------------------------------------------------------
    def _bin(self, row, terms, nrows, sel=None):
        """row: the row (< nrows) of every entry, or of the entries `sel` (ascending indices) alone; terms: per-entry arrays
        over all entries.  Returns the keys row * nseg + segment of the groups that have entries, and per group the sums of
        _term_sums.  Groups without entries are not returned: what the caller holds for them stays +0.0."""
        seg = self.seg if sel is None else self.seg[sel]
        # the entries are in segment order: a stable sort by row leaves every (row, segment) group contiguous
        order = numpy.argsort(row.astype(numpy.int16 if nrows < 2**15 else numpy.int64), kind='stable')
        key = row[order] * self.nseg + seg[order]
        starts = numpy.flatnonzero(numpy.concatenate([[True], key[1:] != key[:-1]])) if key.size else numpy.zeros(0, int)
        return key[starts], _term_sums(terms, starts, order if sel is None else sel[order])   # key[starts] has no repeats

    def _each_level(self, level, threads=1):
        """the levels are independent until they are added up: `threads` > 1 works on that many at a time"""
        if threads > 1:
            with concurrent.futures.ThreadPoolExecutor(threads) as pool:
                list(pool.map(level, range(self.nz)))
        else:
            for z in range(self.nz):
                level(z)

    def _with_totals(self, a):
        """(..., nseg) -> (..., row_length) in float64: [segments | transects]"""
        o = self.tr_off
        tot = [a[..., o[p]:o[p + 1]].sum(axis=-1, dtype=ACC)[..., None] for p in range(o.size - 1)]
        return numpy.concatenate([a] + tot, axis=-1).astype(numpy.float64)

    def _pair(self, a, q):
        """columns q (values) and q + 1 (sum of |terms|) of a (..., nseg, 2 k) as [segments | transects] float64 rows"""
        return self._with_totals(a[..., q]), self._with_totals(a[..., q + 1])

    # ---- one step ----------------------------------------------------------------------------------------------------------
    def step(self, values, edge_sets=(), threads=1, volume_classes=True, tracer=True):
        """values(name, z, cells) -> the raw values of 'uo', 'vo', 'tracer' (carried; tracer=True only), 'class' (class field;
        with edge sets only) and 'e3u', 'e3v' (cell_thickness only) of level z at the flat cell indices `cells`, in the
        array's dtype.  Returns a dict of (want, mag) pairs of [segments | transects] rows: 'volume' and 'tracer'
        (row_length,), 'volume_profile' and 'tracer_profile' (nz, row_length), and for every k ('volume_classes', k) and
        ('tracer_classes', k), (len(edge_sets[k]) + 2, row_length).  With `threads` > 1 `values` is called from those
        threads.  volume_classes=False leaves the 'volume_classes' rows out (they are not in the result); tracer=False
        leaves every tracer value 0."""
        nseg, nz = self.nseg, self.nz
        edge_sets = [numpy.asarray(e, dtype=numpy.float64) for e in edge_sets]
        # last axis: volume, sum |volume terms|, tracer, sum |tracer terms|
        prof = numpy.zeros((nz, nseg, 4), ACC)
        # every set's row follows from the row among the union of all edges, so the terms are binned once per level
        union = numpy.unique(numpy.concatenate(edge_sets)) if edge_sets else numpy.zeros(0)
        fine = numpy.zeros(((union.size + 2) * nseg, 4), ACC)
        lock = threading.Lock()

        def level(z):
            dv, dt = self._factors(values, z, tracer)[:2]
            tv, tt = self._entries(dv), self._entries(dt)
            prof[z][self.useg] = _term_sums([tv, tt], self.seg_starts)
            if edge_sets:
                row = self._class_rows(values, z, union)[self.face_of]
                keys, sums = self._bin(row, [tv if volume_classes else None, tt], union.size + 2)
                with lock:
                    fine[keys] += sums

        self._each_level(level, threads)
        out = {}
        sums = prof.sum(axis=0, dtype=ACC)
        out['volume'], out['tracer'] = self._pair(sums, 0), self._pair(sums, 2)
        out['volume_profile'], out['tracer_profile'] = self._pair(prof, 0), self._pair(prof, 2)
        fine = fine.reshape(union.size + 2, nseg, 4)
        for k, e in enumerate(edge_sets):
            # union row q > 0 holds the values in [union[q - 1], union[q]): as many edges of e are <= them as are <= union[q - 1]
            row_of = numpy.concatenate([[0], numpy.searchsorted(e, union, side='right'), [e.size + 1]])
            acc = numpy.zeros((e.size + 2, nseg, 4), ACC)
            for q in range(union.size + 2):
                acc[row_of[q]] += fine[q]
            out['tracer_classes', k] = self._pair(acc, 2)
            if volume_classes:
                out['volume_classes', k] = self._pair(acc, 0)
        return out


def array_values(arrays, t):
    """the `values` callback for host arrays {'uo': (nt, nz, ny, nx), ..., 'e3u': (nt or 1, nz, ny, nx), ...} at step t: an
    array with one step is static"""
    def values(name, z, cells):
        a = arrays[name]
        return a[t if a.shape[0] > 1 else 0, z].reshape(-1)[cells]
    return values
