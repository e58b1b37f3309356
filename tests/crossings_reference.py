"""The reference of the crossings of one time step (nf_field_compute_crossings), for any grid size.  Entries, faces, presence,
face values, the volume and tracer terms and the thickness th are those of tests/resolved_reference.py (its _factors and
_entries give q and c); the rule by which a face counts and the area terms are those of tests/section_reference.py (a, b), and
g is the area term without the tracer condition:

    q  the volume term                       c  the tracer term
    a  |w| * (th * arc) where the velocity at the face is present and the carried tracer has a finite face value x, else 0
    b  a * (x - reference)
    g  |w| * (th * arc) where the velocity at the face is present, else 0

No Sverdrup scale in a, b, g.  What is this module's own is the grouping: crossing k is entries 4k .. 4k + 3 of getWeights()
(slots south, east, north, west of one cell and one target segment), and a value is the float64 sum of its four terms in slot
order, ((s + e) + n) + w, with row 0's south slot as +0.0 -- nothing is summed over records, levels or segments.  `mag` is the
sum of the absolute values of the four terms.
"""
import numpy

from resolved_reference import ResolvedReference, _present, array_values  # noqa: F401  (for the callers)

PLANES = {False: ('q', 'g'), True: ('q', 'c', 'a', 'b')}


class CrossingsReference(ResolvedReference):
    """ResolvedReference with the per-record planes.  The entries must come four to a record, in slot order."""

    def __init__(self, cell_slot, weight, segment, *a, **kw):
        ce, sg = numpy.asarray(cell_slot, dtype=numpy.int64), numpy.asarray(segment, dtype=numpy.int64)
        assert ce.size % 4 == 0
        self.nrec = ce.size // 4
        quad = ce.reshape(-1, 4)
        assert numpy.array_equal(quad % 4, numpy.tile(numpy.arange(4), (self.nrec, 1))), 'entries: four slots per record'
        assert numpy.all(quad // 4 == quad[:, :1] // 4) and numpy.all(sg.reshape(-1, 4) == sg.reshape(-1, 4)[:, :1])
        assert numpy.all(numpy.diff(sg) >= 0), 'entries: sorted by segment'
        ResolvedReference.__init__(self, ce, weight, sg, *a, **kw)
        nx = int(a[3] if len(a) > 3 else kw['nx'])
        # the base class keeps the entries that carry something, in their order (sorted by segment already): where they were
        self.entry_of = numpy.flatnonzero(~((ce % 4 == 0) & (ce // 4 < nx)))
        assert self.entry_of.size == self.w.size and numpy.array_equal(self.seg, sg[self.entry_of])
        self.rec_cell, self.rec_seg = quad[:, 0] // 4, sg[::4]

    def _per_record(self, t):
        """per kept entry -> (value, mag) per record: the four slots added in slot order, a dropped entry as +0.0"""
        full = numpy.zeros(4 * self.nrec, numpy.float64)
        full[self.entry_of] = t
        s, e, n, w = full.reshape(-1, 4).T
        with numpy.errstate(invalid='ignore', over='ignore'):
            return ((s + e) + n) + w, ((numpy.abs(s) + numpy.abs(e)) + numpy.abs(n)) + numpy.abs(w)

    def crossing_step(self, values, carry):
        """values(name, z, cells): as in ResolvedReference.step.  Returns (want, mag), each (2 or 4, nz, nrec): the planes
        q, g (carry False) or q, c, a, b (carry True)."""
        names = PLANES[bool(carry)]
        want, mag = (numpy.zeros((len(names), self.nz, self.nrec), numpy.float64) for _ in range(2))
        aw, abs_arc = numpy.abs(self.w), numpy.abs(self.f_arc)
        for z in range(self.nz):
            dv, dt, has_t, xt = self._factors(values, z, tracer=bool(carry))
            uo, vo = values('uo', z, self.cells), values('vo', z, self.cells)
            has_v = numpy.where(self.f_is_u, _present(uo, self.uv_markers)[self.ia], _present(vo, self.uv_markers)[self.ia])
            tharc = self._thick(values, z) * abs_arc
            terms = {'q': self._entries(dv)}
            if carry:
                counts = has_v & has_t & numpy.isfinite(numpy.where(has_t, xt, 0.0))
                alpha = aw * numpy.where(counts, tharc, 0.0)[self.face_of]
                dx = numpy.where(counts, xt, self.reference) - self.reference
                terms.update(c=self._entries(dt), a=alpha, b=alpha * dx[self.face_of])
            else:
                terms['g'] = aw * numpy.where(has_v, tharc, 0.0)[self.face_of]
            for p, nm in enumerate(names):
                want[p, z], mag[p, z] = self._per_record(terms[nm])
        return want, mag


def line_cell_pieces(x0, y0, x1, y1, gx0, gy0, dx, dy, nx, ny):
    """Closed form on an un-rotated regular lon-lat grid (cell (j, i) = [gx0 + i dx, gx0 + (i + 1) dx] x [gy0 + j dy, ...]):
    the pieces of the straight planar segment (x0, y0) -> (x1, y1) are bounded by its crossings with the grid lines
    lon = gx0 + k dx, lat = gy0 + k dy.  Returns [(ta, tb, j, i)] in the order along the segment, pieces outside the grid
    left out; i is not wrapped (the caller shifts the segment by the period instead)."""
    ts = {0.0, 1.0}
    for p0, p1, g0, d, n in ((x0, x1, gx0, dx, nx), (y0, y1, gy0, dy, ny)):
        if p1 != p0:
            for k in range(n + 1):
                t = (g0 + k * d - p0) / (p1 - p0)
                if 0.0 < t < 1.0:
                    ts.add(t)
    ts = sorted(ts)
    out = []
    for ta, tb in zip(ts[:-1], ts[1:]):
        if tb - ta <= 1e-13:
            continue
        tm = 0.5 * (ta + tb)
        i = int(numpy.floor((x0 + tm * (x1 - x0) - gx0) / dx))
        j = int(numpy.floor((y0 + tm * (y1 - y0) - gy0) / dy))
        if 0 <= i < nx and 0 <= j < ny:
            out.append((ta, tb, j, i))
    return out
