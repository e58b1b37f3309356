"""The numpy restatement of nf_time_mean_steps and nf_time_mean_weighted_steps (include/nemoflux_amd.h,
nemoflux_amd/csrc/nf_timemean.hip), vectorised over the values and looping over the table in its order, and the scalar Python
loops it is pinned to (tests/test_selected_mean_cpu.py).  `src` (and `thk`) are the listed steps already gathered in table
order, (nsteps, n): row j is the step at step_offsets[j]; `weights` has one float64 per row, None = all 1.

Plain form, per value i:  s = +0.0, wp = +0.0, c = 0 (or the carried ones);  for j in table order:
    x = src[j, i]; x present (tests/timemean_reference.py):  s = s + (w_j * float64(x)), wp = wp + w_j, c += 1
the product rounded to float64, then added.  The last call finishes: OVER_STEPS s / total_weight, OVER_PRESENT s / wp, and
fill_out where c == 0.
Thickness-weighted form:  g = w_j * fixth(thk[j, i]), rounded;  sH = sH + g at every step;  x present: sF = sF + (g *
float64(x)), c += 1.  Finish: c == 0 ? fill_out : (sH == 0 ? +0.0 : sF / sH) and sH / total_weight.
float64 products, sums and quotients are IEEE operations in numpy as on the device: the results are reproduced bit for bit
(same_bits of tests/timemean_reference.py)."""
import numpy

from timemean_reference import OVER_PRESENT, OVER_STEPS, present, same_bits  # noqa: F401  (for the tests that import this)
from weighted_mean_reference import fixth

MONTHS = numpy.array([31., 28., 31., 30., 31., 30., 31., 31., 30., 31., 30., 31.])


def _weights(weights, nsteps):
    w = numpy.ones(nsteps, numpy.float64) if weights is None else numpy.array(weights, dtype=numpy.float64)
    assert w.shape == (nsteps,)
    return w


def total_weight(weights, nsteps=None):
    """the float64 sum of the weights added in order, as the caller of the C ABI forms it"""
    w = _weights(weights, nsteps if weights is None else len(weights))
    tot = numpy.float64(0.0)
    for x in w:
        tot = tot + x
    return float(tot)


def accumulate(src, weights=None, markers=(), s=None, wp=None, c=None):
    """Returns (s, wp, c) after these rows: float64, float64, uint32; s, wp, c given: carried."""
    src = numpy.asarray(src)
    w = _weights(weights, src.shape[0])
    s = numpy.zeros(src.shape[1:], numpy.float64) if s is None else numpy.array(s, dtype=numpy.float64)
    wp = numpy.zeros(src.shape[1:], numpy.float64) if wp is None else numpy.array(wp, dtype=numpy.float64)
    c = numpy.zeros(src.shape[1:], numpy.uint32) if c is None else numpy.array(c, dtype=numpy.uint32)
    with numpy.errstate(invalid='ignore', over='ignore'):
        for j in range(src.shape[0]):
            ok = present(src[j], markers)
            prod = w[j] * src[j].astype(numpy.float64)
            s = numpy.where(ok, s + prod, s)
            wp = numpy.where(ok, wp + w[j], wp)
            c = c + ok.astype(numpy.uint32)
    return s, wp, c


def finish(s, wp, c, rule, total=None, fill_out=numpy.nan):
    with numpy.errstate(invalid='ignore', divide='ignore', over='ignore'):
        mean = s / numpy.float64(total) if rule == OVER_STEPS else s / wp
    return numpy.where(c == 0, numpy.float64(fill_out), mean)


def selected_mean(src, weights=None, markers=(), rule=OVER_PRESENT, total=None, fill_out=numpy.nan):
    """the mean of the rows of src in one go; total: the ordered sum of the weights when not given"""
    src = numpy.asarray(src)
    s, wp, c = accumulate(src, weights, markers)
    return finish(s, wp, c, rule, total_weight(weights, src.shape[0]) if total is None else total, fill_out)


def accumulate_weighted(src, thk, weights=None, markers=(), thk_markers=(), sF=None, sH=None, c=None):
    """Returns (sF, sH, c) after these rows; sF, sH, c given: carried."""
    src, thk = numpy.asarray(src), numpy.asarray(thk)
    assert src.shape == thk.shape and src.dtype == thk.dtype
    w = _weights(weights, src.shape[0])
    sF = numpy.zeros(src.shape[1:], numpy.float64) if sF is None else numpy.array(sF, dtype=numpy.float64)
    sH = numpy.zeros(src.shape[1:], numpy.float64) if sH is None else numpy.array(sH, dtype=numpy.float64)
    c = numpy.zeros(src.shape[1:], numpy.uint32) if c is None else numpy.array(c, dtype=numpy.uint32)
    with numpy.errstate(invalid='ignore', over='ignore'):
        for j in range(src.shape[0]):
            g = w[j] * fixth(thk[j], thk_markers)
            sH = sH + g
            ok = present(src[j], markers)
            prod = g * src[j].astype(numpy.float64)
            sF = numpy.where(ok, sF + prod, sF)
            c = c + ok.astype(numpy.uint32)
    return sF, sH, c


def finish_weighted(sF, sH, c, total, fill_out=numpy.nan):
    """(the weighted mean, the mean thickness)"""
    with numpy.errstate(invalid='ignore', divide='ignore', over='ignore'):
        mean = numpy.where(sH == 0, numpy.float64(0.0), sF / sH)
        hbar = sH / numpy.float64(total)
    return numpy.where(c == 0, numpy.float64(fill_out), mean), hbar


def selected_weighted_mean(src, thk, weights=None, markers=(), thk_markers=(), total=None, fill_out=numpy.nan):
    src = numpy.asarray(src)
    sF, sH, c = accumulate_weighted(src, thk, weights, markers, thk_markers)
    return finish_weighted(sF, sH, c, total_weight(weights, src.shape[0]) if total is None else total, fill_out)


def _marks(dt, markers):
    with numpy.errstate(over='ignore'):
        return [dt(m) for m in markers if m == m]


def scalar_selected_mean(src, weights, markers, rule, total, fill_out):
    """the plain definition as a scalar Python loop over values and table rows; numpy scalars, so that float32 compares stay
    float32.  Returns (the mean, s, wp, c)."""
    src = numpy.asarray(src)
    nsteps, n = src.shape
    w = _weights(weights, nsteps)
    marks = _marks(src.dtype.type, markers)
    mean, outS, outW = (numpy.zeros(n, numpy.float64) for _ in range(3))
    cnt = numpy.zeros(n, numpy.uint32)
    with numpy.errstate(invalid='ignore', over='ignore', divide='ignore'):
        for i in range(n):
            s, wp, c = numpy.float64(0.0), numpy.float64(0.0), 0
            for j in range(nsteps):
                x = src[j, i]
                if x != x or any(x == m for m in marks):
                    continue
                prod = w[j] * numpy.float64(x)
                s = s + prod
                wp = wp + w[j]
                c += 1
            outS[i], outW[i], cnt[i] = s, wp, c
            mean[i] = fill_out if c == 0 else (s / numpy.float64(total) if rule == OVER_STEPS else s / wp)
    return mean, outS, outW, cnt


def scalar_selected_weighted_mean(src, thk, weights, markers, thk_markers, total, fill_out):
    """the thickness-weighted definition as a scalar loop.  Returns (the weighted mean, the mean thickness, sF, sH, c)."""
    src, thk = numpy.asarray(src), numpy.asarray(thk)
    nsteps, n = src.shape
    w = _weights(weights, nsteps)
    marks, hmarks = _marks(src.dtype.type, markers), _marks(src.dtype.type, thk_markers)
    mean, hbar, outF, outH = (numpy.zeros(n, numpy.float64) for _ in range(4))
    cnt = numpy.zeros(n, numpy.uint32)
    with numpy.errstate(invalid='ignore', over='ignore', divide='ignore'):
        for i in range(n):
            sF, sH, c = numpy.float64(0.0), numpy.float64(0.0), 0
            for j in range(nsteps):
                h = thk[j, i]
                h = numpy.float64(0.0) if (h != h or any(h == m for m in hmarks)) else numpy.float64(h)
                g = w[j] * h
                sH = sH + g
                x = src[j, i]
                if x != x or any(x == m for m in marks):
                    continue
                prod = g * numpy.float64(x)
                sF = sF + prod
                c += 1
            outF[i], outH[i], cnt[i] = sF, sH, c
            mean[i] = fill_out if c == 0 else (numpy.float64(0.0) if sH == 0 else sF / sH)
            hbar[i] = sH / numpy.float64(total)
    return mean, hbar, outF, outH, cnt


def _fill_of(a, markers):
    m = [x for x in markers if x == x]
    with numpy.errstate(over='ignore'):
        return float(a.dtype.type(m[0])) if m else numpy.nan


def field_selected_mean_arrays(uo, vo, uv_markers, select, weights=None, tracers=(), e3=None, e3_markers=()):
    """What Field.timeMean(select=, weights=) hands to Field.fromArrays, from host arrays (nt, nz, ny, nx): the float64 means
    of uo, vo over the steps `select` under the velocity rule, (1, nz, ny, nx), with their fill, and for each (array, markers)
    of `tracers` the mean under the tracer rule with its fill.  e3 = (e3u, e3v): the thickness-weighted form, which also returns
    the mean thicknesses.  Returns (u, v, fill), [(tau, fill), ...], (hu, hv) or None."""
    select = list(select)
    tot = total_weight(weights, len(select))

    def rows(a):
        return a[select].reshape(len(select), -1)

    def shaped(m, a):
        return m.reshape((1,) + a.shape[1:])

    fill = _fill_of(uo, uv_markers)
    out = [(shaped(selected_mean(rows(t), weights, m, OVER_PRESENT, tot, _fill_of(t, m)), t), _fill_of(t, m)) for t, m in tracers]
    if e3 is None:
        u, v = (shaped(selected_mean(rows(a), weights, uv_markers, OVER_STEPS, tot, fill), a) for a in (uo, vo))
        return (u, v, fill), out, None
    got = [selected_weighted_mean(rows(a), rows(h), weights, uv_markers, e3_markers, tot, fill) for a, h in zip((uo, vo), e3)]
    (u, hu), (v, hv) = [(shaped(f, uo), shaped(h, uo)) for f, h in got]
    return (u, v, fill), out, (hu, hv)
