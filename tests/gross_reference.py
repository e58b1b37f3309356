"""The reference of the gross transports of one time step (nf_field_compute_gross_profile), for any grid size.  Entries, faces,
the volume and tracer terms (th scalar or read at the face) and the summation are those of tests/resolved_reference.py; its
own is the split by the sign of the water term.  Per level z and entry

    water term    q = the volume term
    carried term  c = q (volume form), or the tracer term (carried form)

    P[z] = sum of c over the entries with q > 0,    N[z] = sum of c over the entries with q < 0;    q == 0: in neither.

Terms are summed per (level, segment), the transect columns from the segments; `mag` is the sum of |c| over the same entries.
The sign of q is the product of the signs of its factors unless the product underflows: min_abs_q, the smallest non-zero |q|
met, says how far the inputs are from that.

gross_velocities / gross_thickness: the inputs of the tests, made so that no |q| comes near underflow -- velocities of
magnitude in [0.01, 1] with either sign, exactly 0, or missing; thicknesses in [0.2, 3], exactly 0, or missing.
"""
import numpy

from resolved_reference import ACC, ResolvedReference, _present, _term_sums, array_values  # noqa: F401  (for the callers)

FILL, MISSING = 1.e20, -999.             # uo / vo
THFILL, THMISSING = -1.e30, 9.e9         # e3u / e3v
MIN_ABS_Q = 1e-200


def gross_velocities(real, shape, seed):
    """uo, vo of `shape` (nt, nz, ny, nx): magnitudes in [0.01, 1], either sign; a tenth exactly 0; blocks of _FillValue, NaN
    and the second marker (land), and each of the three scattered over single cells"""
    rng = numpy.random.default_rng(seed)
    dt = numpy.dtype(real).type
    nt, nz, ny, nx = shape
    out = []
    for k in range(2):
        a = (rng.uniform(0.0101, 1., shape) * rng.choice([-1., 1.], shape)).astype(real)   # inside [0.01, 1] in float32 too
        a[rng.random(shape) < 0.1] = 0
        for m in (FILL, MISSING, numpy.nan):
            a[rng.random(shape) < 0.03] = dt(m)
        out.append(a)
    u, v = out
    j0, j1, i0, i1 = ny // 9, ny // 4 + 1, nx // 7, nx // 4 + 1
    u[:, nz // 2:, j0:j1, i0:i1] = dt(FILL)
    v[:, nz // 2:, j0:j1, i0:i1] = numpy.nan
    u[:, :2, ny // 2:ny // 2 + 2, nx // 3:nx // 2] = dt(MISSING)
    v[:, nz - 1:, ny // 2:ny // 2 + 2, nx // 3:nx // 2] = dt(MISSING)
    return u, v


def gross_thickness(real, shape, seed):
    """e3u, e3v of `shape` (1 or nt, nz, ny, nx): values in [0.2, 3]; exactly 0, both markers and NaN scattered"""
    rng = numpy.random.default_rng(seed)
    dt = numpy.dtype(real).type
    out = []
    for k in range(2):
        a = rng.uniform(0.2001, 3., shape).astype(real)
        for m in (0.0, THFILL, THMISSING, numpy.nan):
            a[rng.random(shape) < 0.03] = dt(m)
        out.append(a)
    return out


def inputs_are_safe(u, v, e3=(), markers=(FILL, MISSING), thick_markers=(THFILL, THMISSING)):
    """the condition on the inputs: every velocity is missing, exactly 0 or of magnitude in [0.01, 1]; every thickness is
    missing, exactly 0 or >= 0.2"""
    ok = True
    for a in (u, v):
        x = numpy.abs(a[_present(a, markers)].astype(numpy.float64))
        ok = ok and bool(numpy.all((x == 0) | ((x >= 0.01) & (x <= 1.0))))
    for a in e3:
        x = a[_present(a, thick_markers)].astype(numpy.float64)
        ok = ok and bool(numpy.all((x == 0) | (x >= 0.2)))
    return ok


class GrossReference(ResolvedReference):
    """ResolvedReference with the rows of the gross profile."""

    def _gross_terms(self, values, z, tracer):
        """per entry: q, the carried terms [q] or [q, tracer term], and the smallest non-zero |q| (inf: every q is 0)"""
        dv, dt = self._factors(values, z, tracer)[:2]
        q = self._entries(dv)
        return q, [q, self._entries(dt)] if tracer else [q], float(numpy.abs(q[q != 0]).min(initial=numpy.inf))

    def _gross_result(self, acc, min_q):
        """acc: (2, ..., nseg, 2 forms), last axis: per form the sum, the sum of |terms|"""
        res = {nm: self._pair(acc, 2 * k) for k, nm in enumerate(('volume', 'carried')[:acc.shape[-1] // 2])}
        res['min_abs_q'] = min(min_q)
        return res

    def gross_step(self, values, tracer=True, threads=1):
        """values(name, z, cells): as in ResolvedReference.step, 'uo', 'vo' (and 'tracer' with tracer=True, 'e3u', 'e3v' with
        cell_thickness).  Returns {'volume': (want, mag), 'carried': (want, mag) (tracer=True), 'min_abs_q': float}; want and
        mag have shape (2, nz, row_length): P then N, rows [segments | transects]; mag is the sum of |c| of the entries of
        the value.  min_abs_q: the smallest non-zero |q|, inf when every q is 0."""
        prof = numpy.zeros((2, self.nz, self.nseg, 4 if tracer else 2), ACC)
        min_q = [numpy.inf] * self.nz

        def level(z):
            q, cs, min_q[z] = self._gross_terms(values, z, tracer)
            for part, sel in enumerate((q > 0, q < 0)):
                prof[part, z][self.useg] = _term_sums([numpy.where(sel, c, 0.0) for c in cs], self.seg_starts)

        self._each_level(level, threads)
        return self._gross_result(prof, min_q)
