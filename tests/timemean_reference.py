"""The numpy restatement of nf_time_mean (include/nemoflux_amd.h, nemoflux_amd/csrc/nf_timemean.hip), vectorised over the
values and looping over the steps in ascending order, and the scalar Python loop it is pinned to (tests/test_timemean_cpu.py).

Per value i:  s = +0.0, c = 0 (or the carried s, c);  for t ascending: x = src[t, i]; x present: s = s + float64(x), c += 1.
Present: not NaN and different from both markers, each cast to the array's dtype and compared in that dtype; +-inf is present.
The last call finishes: OVER_STEPS s / total_steps, OVER_PRESENT s / c, and fill_out where c == 0 under both rules.  float64
addition and division are IEEE operations in numpy as on the device, so the result is reproduced bit for bit -- except for the
sign and payload of a NaN that an invalid operation (+inf + -inf) produces, which IEEE 754 leaves open: same_bits treats every
NaN as one value and compares everything else, the sign of zero included, by its bits."""
import numpy

OVER_STEPS, OVER_PRESENT = 0, 1


def present(x, markers):
    """x: an array of the source dtype; markers: floats, NaN = unused"""
    ok = ~numpy.isnan(x)
    for m in markers:
        if m == m:
            with numpy.errstate(over='ignore'):
                ok &= x != x.dtype.type(m)
    return ok


def accumulate(src, markers=(), s=None, c=None):
    """src: (nsteps, n) of float64 / float32.  Returns the (s, c) after these steps, float64 and uint32; s, c given: carried."""
    src = numpy.asarray(src)
    s = numpy.zeros(src.shape[1:], numpy.float64) if s is None else numpy.array(s, dtype=numpy.float64)
    c = numpy.zeros(src.shape[1:], numpy.uint32) if c is None else numpy.array(c, dtype=numpy.uint32)
    with numpy.errstate(invalid='ignore', over='ignore'):
        for t in range(src.shape[0]):
            ok = present(src[t], markers)
            s = numpy.where(ok, s + src[t].astype(numpy.float64), s)
            c = c + ok.astype(numpy.uint32)
    return s, c


def finish(s, c, rule, total_steps=None, fill_out=numpy.nan):
    with numpy.errstate(invalid='ignore', divide='ignore', over='ignore'):
        mean = s / numpy.float64(total_steps) if rule == OVER_STEPS else s / c.astype(numpy.float64)
    return numpy.where(c == 0, numpy.float64(fill_out), mean)


def time_mean(src, markers=(), rule=OVER_PRESENT, total_steps=None, fill_out=numpy.nan):
    """the mean of src (nsteps, ...) in one go; total_steps: nsteps when not given"""
    src = numpy.asarray(src)
    s, c = accumulate(src, markers)
    return finish(s, c, rule, src.shape[0] if total_steps is None else total_steps, fill_out)


def scalar_time_mean(src, markers, rule, total_steps, fill_out):
    """the definition as a scalar Python loop over values and steps; numpy scalars, so that float32 compares stay float32"""
    src = numpy.asarray(src)
    nsteps, n = src.shape
    dt = src.dtype.type
    with numpy.errstate(over='ignore'):
        marks = [dt(m) for m in markers if m == m]
    out, cnt = numpy.zeros(n, numpy.float64), numpy.zeros(n, numpy.uint32)
    with numpy.errstate(invalid='ignore', over='ignore', divide='ignore'):
        for i in range(n):
            s, c = numpy.float64(0.0), 0
            for t in range(nsteps):
                x = src[t, i]
                if x != x or any(x == m for m in marks):
                    continue
                s = s + numpy.float64(x)
                c += 1
            cnt[i] = c
            out[i] = fill_out if c == 0 else (s / numpy.float64(total_steps) if rule == OVER_STEPS else s / numpy.float64(c))
    return out, cnt


def same_bits(a, b):
    """a, b float64 arrays of one shape: equal bit for bit, every NaN counting as one value"""
    a, b = numpy.ascontiguousarray(a, dtype=numpy.float64), numpy.ascontiguousarray(b, dtype=numpy.float64)
    if a.shape != b.shape:
        return False
    nan = numpy.isnan(a) & numpy.isnan(b)
    return bool(numpy.all(nan | (a.view(numpy.uint64) == b.view(numpy.uint64))))


def field_mean_arrays(uo, vo, uv_markers, tracers=()):
    """What Field.timeMean hands to Field.fromArrays, from host arrays (nt, nz, ny, nx): the float64 means of uo, vo under the
    velocity rule, (1, nz, ny, nx), with their fill (the first marker as the dtype holds it, NaN without one), and for each
    (array, markers) of `tracers` the mean under the tracer rule with its fill.  Returns (u, v, fill), [(tau, fill), ...]."""
    def fill_of(a, markers):
        m = [x for x in markers if x == x]
        return float(a.dtype.type(m[0])) if m else numpy.nan

    def mean(a, markers, rule):
        nt = a.shape[0]
        m = time_mean(a.reshape(nt, -1), markers, rule, nt, fill_of(a, markers))
        return m.reshape((1,) + a.shape[1:])

    fill = fill_of(uo, uv_markers)
    out = [(mean(t, m, OVER_PRESENT), fill_of(t, m)) for t, m in tracers]
    return (mean(uo, uv_markers, OVER_STEPS), mean(vo, uv_markers, OVER_STEPS), fill), out
