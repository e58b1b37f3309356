"""The numpy restatement of nf_time_mean_weighted (include/nemoflux_amd.h, nemoflux_amd/csrc/nf_timemean.hip), vectorised over
the values and looping over the steps in ascending order, and the scalar Python loop it is pinned to
(tests/test_weighted_mean_cpu.py).

Per value i:  sF = +0.0, sH = +0.0, c = 0 (or the carried ones);  for t ascending:
    h = fixth(thk[t, i])     NaN or one of the thickness's markers (compared in its dtype) -> 0, else float64(thk[t, i])
    sH = sH + h              at every step
    x = src[t, i]; x present (tests/timemean_reference.py, src's own markers):  sF = sF + (h * float64(x)), c += 1
the product rounded to float64, then added.  The last call finishes: the weighted mean c == 0 ? fill_out : (sH == 0 ? +0.0 :
sF / sH) and the mean thickness sH / total_steps.  float64 products, sums and quotients are IEEE operations in numpy as on the
device, so the results are reproduced bit for bit (same_bits of tests/timemean_reference.py)."""
import numpy

from timemean_reference import present, same_bits  # noqa: F401  (same_bits: for the tests that import this module)


def fixth(h, markers):
    """the thickness as float64, 0 where it is NaN or a marker"""
    return numpy.where(present(h, markers), h.astype(numpy.float64), numpy.float64(0.0))


def accumulate(src, thk, markers=(), thk_markers=(), sF=None, sH=None, c=None):
    """src, thk: (nsteps, n) of one dtype, float64 or float32.  Returns (sF, sH, c) after these steps, float64, float64 and
    uint32; sF, sH, c given: carried."""
    src, thk = numpy.asarray(src), numpy.asarray(thk)
    assert src.shape == thk.shape and src.dtype == thk.dtype
    sF = numpy.zeros(src.shape[1:], numpy.float64) if sF is None else numpy.array(sF, dtype=numpy.float64)
    sH = numpy.zeros(src.shape[1:], numpy.float64) if sH is None else numpy.array(sH, dtype=numpy.float64)
    c = numpy.zeros(src.shape[1:], numpy.uint32) if c is None else numpy.array(c, dtype=numpy.uint32)
    with numpy.errstate(invalid='ignore', over='ignore'):
        for t in range(src.shape[0]):
            h = fixth(thk[t], thk_markers)
            sH = sH + h
            ok = present(src[t], markers)
            prod = h * src[t].astype(numpy.float64)
            sF = numpy.where(ok, sF + prod, sF)
            c = c + ok.astype(numpy.uint32)
    return sF, sH, c


def finish(sF, sH, c, total_steps, fill_out=numpy.nan):
    """(the weighted mean, the mean thickness)"""
    with numpy.errstate(invalid='ignore', divide='ignore', over='ignore'):
        mean = numpy.where(sH == 0, numpy.float64(0.0), sF / sH)
        hbar = sH / numpy.float64(total_steps)
    return numpy.where(c == 0, numpy.float64(fill_out), mean), hbar


def weighted_time_mean(src, thk, markers=(), thk_markers=(), total_steps=None, fill_out=numpy.nan):
    """the weighted mean of src and the mean of thk, (nsteps, ...), in one go; total_steps: nsteps when not given"""
    src = numpy.asarray(src)
    sF, sH, c = accumulate(src, thk, markers, thk_markers)
    return finish(sF, sH, c, src.shape[0] if total_steps is None else total_steps, fill_out)


def scalar_weighted_time_mean(src, thk, markers, thk_markers, total_steps, fill_out):
    """the definition as a scalar Python loop over values and steps; numpy scalars, so that float32 compares stay float32.
    Returns (the weighted mean, the mean thickness, sF, sH, c)."""
    src, thk = numpy.asarray(src), numpy.asarray(thk)
    nsteps, n = src.shape
    dt = src.dtype.type
    with numpy.errstate(over='ignore'):
        marks = [dt(m) for m in markers if m == m]
        hmarks = [dt(m) for m in thk_markers if m == m]
    mean, hbar = numpy.zeros(n, numpy.float64), numpy.zeros(n, numpy.float64)
    outF, outH, cnt = numpy.zeros(n, numpy.float64), numpy.zeros(n, numpy.float64), numpy.zeros(n, numpy.uint32)
    with numpy.errstate(invalid='ignore', over='ignore', divide='ignore'):
        for i in range(n):
            sF, sH, c = numpy.float64(0.0), numpy.float64(0.0), 0
            for t in range(nsteps):
                h = thk[t, i]
                h = numpy.float64(0.0) if (h != h or any(h == m for m in hmarks)) else numpy.float64(h)
                sH = sH + h
                x = src[t, i]
                if x != x or any(x == m for m in marks):
                    continue
                prod = h * numpy.float64(x)
                sF = sF + prod
                c += 1
            outF[i], outH[i], cnt[i] = sF, sH, c
            mean[i] = fill_out if c == 0 else (numpy.float64(0.0) if sH == 0 else sF / sH)
            hbar[i] = sH / numpy.float64(total_steps)
    return mean, hbar, outF, outH, cnt


def field_weighted_mean_arrays(uo, vo, uv_markers, e3u, e3v, e3_markers):
    """What Field.timeMean(thicknessWeighted=True) hands to Field.fromArrays and to setCellThickness, from host arrays
    (nt, nz, ny, nx) of one dtype: the weighted means of uo with e3u and of vo with e3v and the mean thicknesses, float64
    (1, nz, ny, nx), and the velocities' fill (the first marker as the dtype holds it, NaN without one).
    Returns (u, v, fill), (hu, hv)."""
    m = [x for x in uv_markers if x == x]
    fill = float(uo.dtype.type(m[0])) if m else numpy.nan

    def mean(a, e3):
        nt = a.shape[0]
        f, h = weighted_time_mean(a.reshape(nt, -1), e3.reshape(nt, -1), uv_markers, e3_markers, nt, fill)
        return f.reshape((1,) + a.shape[1:]), h.reshape((1,) + a.shape[1:])

    u, hu = mean(uo, e3u)
    v, hv = mean(vo, e3v)
    return (u, v, fill), (hu, hv)
