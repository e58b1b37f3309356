"""A sparse float64 / long-double reference of the gross transports of one time step (nf_field_compute_gross_profile), for any
grid size: the definition of include/nemoflux_amd.h restated in numpy over the cells the weight entries touch.  It uses the
entry / face bookkeeping and the summation of tests/resolved_reference.py, through tests/cellthick_reference.py, and shares no
code with the product.

Per level z and entry (cell c, slot, weight w, segment), with `a` the cell whose face the slot is (east, north: c; west: the
west cell; south: the south cell; the south entries of row 0 are dropped):

    water term    q = w * ((th * fixed(vel)) * arc)         vel = uo[t, z, a], arc = +arcE[a] for the east and west slots,
                                                            vel = vo[t, z, a], arc = -arcN[a] for the north and south slots
    carried term  c = q                                     (volume form)
                  c = w * ((th * (fixed(vel) * tf)) * arc)  (carried form; tf = the tracer's face value - reference, 0 for a
                                                            face without a value)

each times 6.371 in Sverdrup mode; th = thickness[z], or fixth(e3u[t', z, a]) / fixth(e3v[t', z, a]) with cell thicknesses.

    P[z] = sum of c over the entries with q > 0,    N[z] = sum of c over the entries with q < 0;    q == 0: in neither.

Terms are formed in float64 and summed in long double per (level, segment), the transect columns from the segments; `mag` is
the sum of |c| over the same entries.  The sign of q is the product of the signs of its factors unless the product underflows:
min_abs_q, the smallest non-zero |q| met, says how far the inputs are from that.

gross_velocities / gross_thickness: the inputs of the tests, made so that no |q| comes near underflow -- velocities of
magnitude in [0.01, 1] with either sign, exactly 0, or missing; thicknesses in [0.2, 3], exactly 0, or missing.
"""
import concurrent.futures

import numpy

from cellthick_reference import CellThickReference, array_values  # noqa: F401  (array_values: for the callers)
from resolved_reference import ACC, _face, _group_sums, _present

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


class GrossReference(CellThickReference):
    """CellThickReference with the rows of the gross profile.  cell_thickness=True: the thickness is read at the face
    ('e3u', 'e3v' of the callback, markers thick_markers); otherwise `thickness` (nz,) is used."""

    def __init__(self, *a, cell_thickness=False, **kw):
        super().__init__(*a, **kw)
        self.cell_thickness = bool(cell_thickness)

    def gross_step(self, values, tracer=True, threads=1):
        """values(name, z, cells) -> the raw values of 'uo', 'vo' (and 'tracer' with tracer=True, 'e3u', 'e3v' with
        cell_thickness) of level z at the flat cell indices `cells`, in the array's dtype.  Returns {'volume': (want, mag),
        'carried': (want, mag) (tracer=True), 'min_abs_q': float}; want and mag have shape (2, nz, row_length): P then N, rows
        [segments | transects]; mag is the sum of |c| of the entries of the value.  min_abs_q: the smallest non-zero |q|,
        inf when every q is 0."""
        nz, nseg = self.nz, self.nseg
        forms = ('volume', 'carried') if tracer else ('volume',)
        prof = {nm: numpy.zeros((2, nz, nseg, 2), ACC) for nm in forms}   # last axis: the sum, the sum of |terms|
        min_q = [numpy.inf] * nz

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
            q = self.w * d['volume'][self.face_of]                        # per entry
            nonzero = numpy.abs(q[q != 0])
            if nonzero.size:
                min_q[z] = float(nonzero.min())
            for nm in forms:
                c = q if nm == 'volume' else self.w * d[nm][self.face_of]
                for part, sel in enumerate((q > 0, q < 0)):
                    t = numpy.where(sel, c, 0.0)
                    out = numpy.zeros((self.seg_starts.size, 2), ACC)
                    out[:, 0], out[:, 1] = _group_sums(t, self.seg_starts), _group_sums(numpy.abs(t), self.seg_starts)
                    prof[nm][part, z][self.useg] = out

        if threads > 1:
            with concurrent.futures.ThreadPoolExecutor(threads) as pool:
                list(pool.map(level, range(nz)))
        else:
            for z in range(nz):
                level(z)
        res = {nm: (self._with_totals(prof[nm][..., 0]), self._with_totals(prof[nm][..., 1])) for nm in forms}
        res['min_abs_q'] = min(min_q)
        return res
