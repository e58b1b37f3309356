"""numpy restatement of nf_iso_depth (include/nemoflux_amd.h is normative): the depth at which a tracer first reaches a value,
column by column.  iso_depth is vectorised over the columns and written from the arrays of the definition (wet mask, kb, D, c,
kref, tau_ref, k*, gathered with take_along_axis); iso_depth_scalar is one Python loop per column written from the same text
as a walk down the levels.  tests/test_iso_depth_cpu.py pins the two to each other bit for bit; the GPU tests compare the
kernel with iso_depth.  Every operation is one IEEE float64 operation in the order of the header.

make_case builds the inputs that the CPU and the GPU tests share, designed so that every branch of the definition is taken by
a share of the columns for every one of the m values; branches names the branch of every (value, column)."""
import numpy

NAN = float('nan')
BRANCHES = ('dry', 'sea bed', 'outcrop', 'at zref', 'interpolated', 'exactly on a level')
DRY, BED, OUTCROP, ATZREF, INTERP, EXACT = range(6)


def present(a, markers):
    """the engine's rule: not NaN and equal to neither marker, each cast to the array's dtype and compared in it"""
    ok = ~numpy.isnan(a)
    with numpy.errstate(over='ignore'):
        for m in markers:
            if m is not None and m == m:
                ok &= a != a.dtype.type(m)
    return ok


def same_bits(a, b):
    """equal value by value, NaNs by position, zeros by sign"""
    a, b = numpy.asarray(a), numpy.asarray(b)
    if a.shape != b.shape or a.dtype != b.dtype:
        return False
    na, nb = numpy.isnan(a), numpy.isnan(b)
    return bool(numpy.array_equal(na, nb) and numpy.array_equal(a[~na], b[~nb])
                and numpy.array_equal(numpy.signbit(a[~na]), numpy.signbit(b[~nb])))


def _wet_and_h(tau, thickness, e3t, tau_markers, e3t_markers):
    nz = tau.shape[0]
    t = tau.reshape(nz, -1)
    wet = present(t, tau_markers)
    if e3t is None:
        h = numpy.broadcast_to(numpy.asarray(thickness, numpy.float64).reshape(nz, 1), t.shape)
    else:
        e = e3t.reshape(nz, -1)
        h = e.astype(numpy.float64)
        with numpy.errstate(invalid='ignore'):
            wet = wet & present(e, e3t_markers) & numpy.isfinite(h) & (h > 0.0)
    return t.astype(numpy.float64), h, wet


def _reached(t, th, sense):
    with numpy.errstate(invalid='ignore'):
        return t >= th if sense > 0 else t <= th


def iso_depth(tau, values, sense, thickness=None, e3t=None, top=0.0, relative=False, zref=10.0, tau_markers=(), e3t_markers=(),
              fill_out=NAN, with_branches=False, with_kstar=False):
    """tau (nz, ny, nx) or (nz, n) of float64 / float32 -> (m, ny, nx) / (m, n) of the same dtype; with_branches: also the
    branch of every (value, column); with_kstar: also k* of every (value, column), kb + 1 where there is none"""
    assert (thickness is None) != (e3t is None)
    nz = tau.shape[0]
    t, h, wet = _wet_and_h(tau, thickness, e3t, tau_markers, e3t_markers)
    n = t.shape[1]
    values = numpy.asarray(values, numpy.float64)
    nwet = numpy.cumprod(wet, axis=0).sum(axis=0)          # kb + 1
    kb = nwet - 1
    D = numpy.empty((nz + 1, n))
    c = numpy.empty((nz, n))
    D[0] = numpy.float64(top)
    with numpy.errstate(all='ignore'):
        for k in range(nz):
            c[k] = D[k] + 0.5 * h[k]
            D[k + 1] = D[k] + h[k]
    cols = numpy.arange(n)
    lev = numpy.arange(nz).reshape(nz, 1)
    inside = lev <= kb
    zr = numpy.float64(zref)

    def at(a, k):
        return a[numpy.clip(k, 0, a.shape[0] - 1), cols]

    if relative:
        with numpy.errstate(invalid='ignore'):
            below = inside & (c <= zr)
        kref = numpy.where(below.any(axis=0), nz - 1 - numpy.argmax(below[::-1], axis=0), 0)
        ta, tb, ca_, cb = at(t, kref), at(t, kref + 1), at(c, kref), at(c, kref + 1)
        with numpy.errstate(all='ignore'):
            interp = ta + (tb - ta) * ((zr - ca_) / (cb - ca_))
            tref = numpy.where((zr <= c[0]) | (kref == kb), ta, interp)
        k0 = kref + 1
    else:
        kref = numpy.zeros(n, numpy.int64)
        tref = numpy.zeros(n)
        k0 = numpy.zeros(n, numpy.int64)
    out = numpy.empty((len(values), n))
    branch = numpy.empty((len(values), n), numpy.int8)
    kstar = numpy.empty((len(values), n), numpy.int64)
    for j, v in enumerate(values):
        with numpy.errstate(all='ignore'):
            th = tref + v if relative else numpy.full(n, v)
            R = _reached(t, th, sense)
            cand = R & inside & (lev >= k0)
            has = cand.any(axis=0)
            ks = numpy.argmax(cand, axis=0)
            a = ks - 1
            tk, ta, ck, ca_ = at(t, ks), at(t, a), at(c, ks), at(c, a)
            frac = (th - ta) / (tk - ta)
            interp = ca_ + (ck - ca_) * frac
            Ra = at(R, a) & (ks > 0)
            r = numpy.where(~has, at(D, kb + 1), numpy.where(ks == 0, D[0], numpy.where(Ra, zr, interp)))
            out[j] = numpy.where(nwet == 0, numpy.float64(fill_out), r)
            kstar[j] = numpy.where(has, ks, kb + 1)
            branch[j] = numpy.where(nwet == 0, DRY, numpy.where(~has, BED, numpy.where(ks == 0, OUTCROP, numpy.where(
                Ra, ATZREF, numpy.where(tk == th, EXACT, INTERP)))))
    with numpy.errstate(over='ignore', invalid='ignore'):
        out = out.astype(tau.dtype).reshape((len(values),) + tau.shape[1:])
    more = ([branch.reshape(out.shape)] if with_branches else []) + ([kstar.reshape(out.shape)] if with_kstar else [])
    return (out, *more) if more else out


def iso_depth_scalar(tau, values, sense, thickness=None, e3t=None, top=0.0, relative=False, zref=10.0, tau_markers=(),
                     e3t_markers=(), fill_out=NAN):
    """the same, one column at a time, as a walk down the levels in Python floats (IEEE float64)"""
    assert (thickness is None) != (e3t is None)
    nz = tau.shape[0]
    t2 = tau.reshape(nz, -1)
    n = t2.shape[1]
    tp = present(t2, tau_markers)
    if e3t is not None:
        e2 = e3t.reshape(nz, -1)
        ep = present(e2, e3t_markers)
    vals = [float(v) for v in values]
    zref, top = float(zref), float(top)
    out = numpy.empty((len(vals), n))
    inf = float('inf')

    def reached(x, th):
        return x >= th if sense > 0 else x <= th

    for i in range(n):
        D = [top]
        c, tt = [], []
        for k in range(nz):
            if not tp[k, i]:
                break
            if e3t is None:
                h = float(thickness[k])
            else:
                h = float(e2[k, i])
                if not (ep[k, i] and h > 0.0 and h < inf):
                    break
            c.append(D[-1] + 0.5 * h)
            D.append(D[-1] + h)
            tt.append(float(t2[k, i]))
        kb = len(tt) - 1
        if kb < 0:
            out[:, i] = fill_out
            continue
        if relative:
            kref = 0
            for k in range(kb + 1):
                if c[k] <= zref:
                    kref = k
            if zref <= c[0] or kref == kb:
                tref = tt[kref]
            else:
                a, b = kref, kref + 1
                with numpy.errstate(all='ignore'):
                    tref = float(numpy.float64(tt[a]) + (numpy.float64(tt[b]) - numpy.float64(tt[a])) *
                                 ((numpy.float64(zref) - numpy.float64(c[a])) / (numpy.float64(c[b]) - numpy.float64(c[a]))))
            k0 = kref + 1
        else:
            tref, k0 = 0.0, 0
        for j, v in enumerate(vals):
            with numpy.errstate(all='ignore'):
                th = float(numpy.float64(tref) + numpy.float64(v)) if relative else v
            ks = None
            for k in range(k0, kb + 1):
                if reached(tt[k], th):
                    ks = k
                    break
            if ks is None:
                r = D[kb + 1]
            elif ks == 0:
                r = D[0]
            elif reached(tt[ks - 1], th):
                r = zref
            else:
                a = ks - 1
                with numpy.errstate(all='ignore'):
                    f = (numpy.float64(th) - numpy.float64(tt[a])) / (numpy.float64(tt[ks]) - numpy.float64(tt[a]))
                    r = float(numpy.float64(c[a]) + (numpy.float64(c[ks]) - numpy.float64(c[a])) * f)
            out[j, i] = r
    with numpy.errstate(over='ignore', invalid='ignore'):
        return out.astype(tau.dtype).reshape((len(vals),) + tau.shape[1:])


# ---- the inputs that the CPU and the GPU tests share ------------------------------------------------------------------------
TFILL, TMISSING = -32768., 1.e20          # the tracer's own markers
EFILL, EMISSING = -999., 5.e15            # e3t's own markers
ZREF = 10.0
ABS_VALUES = {1: [11.5], 3: [9.5, 11.5, 13.25], 8: [9.0, 9.75, 10.5, 11.25, 12.0, 12.75, 13.5, 14.0]}     # rising tracer
REL_VALUES = {1: [0.5], 3: [0.125, 0.5, 2.0], 8: [0.125, 0.25, 0.5, 0.75, 1.0, 1.5, 2.0, 3.0]}
ATZREF_VALUES = [-0.125, 0.0, 0.25]      # offsets <= 0: only they can find level kref itself past the threshold ('at zref')
FLIP = 30.0          # a falling tracer is FLIP - the rising one, its values FLIP - value (relative: -delta)


def level_thickness(nz):
    """level thicknesses on the lattice of multiples of 1/8, c_0 = 2 and c_1 = 10 = ZREF (nz > 1)"""
    if nz <= 7:
        return numpy.array([4.0, 12.0] + [8.0 + 1.125 * k for k in range(5)])[:nz]
    return numpy.concatenate([[4.0, 12.0], numpy.full(nz - 2, 1.25)])


def case_values(m, sense, relative):
    v = numpy.array((REL_VALUES if relative else ABS_VALUES)[m])
    if sense > 0:
        return v
    return -v if relative else FLIP - v


def make_case(real, nz, ny, nx, m, sense, relative, form, seed=0):
    """(tau, thickness or None, e3t or None, values): tau (nz, ny, nx) of `real` on the lattice of multiples of 1/64, with dry
    columns (both markers, NaN), columns that end at a marker, at NaN and -- form 'e3t' -- at a zero, negative, missing or
    infinite thickness, +-inf in the tracer, uniform columns, non-monotone tails, and values placed exactly on levels."""
    if ny * nx == 5:
        return _five_columns(real, nz, m, sense, relative, form)
    rng = numpy.random.default_rng(1000 * nz + 10 * m + (1 if relative else 0) + (2 if sense > 0 else 0) + seed +
                                   (4 if form == 'e3t' else 0) + ny)
    n = ny * nx
    dt = numpy.dtype(real).type
    values = case_values(m, sense, relative)
    rv = numpy.array((REL_VALUES if relative else ABS_VALUES)[m])     # in the rising frame
    hlev = level_thickness(nz)
    if form == 'e3t':
        h = numpy.round(hlev.reshape(nz, 1) * rng.uniform(0.5, 1.5, (nz, n)) * 8.0) / 8.0
        special = rng.random(n) < 0.5           # columns with c_1 == ZREF exactly or zref above c_0
        if nz > 1:
            h[0, special] = numpy.where(rng.random(special.sum()) < 0.5, 4.0, 24.0)
            h[1, special] = 12.0
    else:
        h = numpy.broadcast_to(hlev.reshape(nz, 1), (nz, n)).copy()
    D = numpy.concatenate([numpy.zeros((1, n)), numpy.cumsum(h, axis=0)])
    c = 0.5 * (D[:-1] + D[1:])
    # a rising profile: tau_0 in [0, 20], a total rise in [0, 12] spread over the levels in random shares
    t0 = rng.uniform(0.0, 20.0, n)
    shares = rng.random((nz, n)) + 0.05
    shares[0] = 0.0
    total = numpy.where(rng.random(n) < 0.27, 0.0, rng.uniform(0.0, 12.0, n))      # a quarter of the columns is uniform
    rise = total * numpy.cumsum(shares, axis=0) / numpy.maximum(shares.sum(axis=0), 1.e-9)
    tau = numpy.round((t0 + rise) * 64.0) / 64.0
    cols = numpy.arange(n)
    pexact = min(0.9, 0.2 + 0.15 * m)      # one value per chosen column is put exactly on a level
    if relative and nz > 2:
        below = c <= ZREF
        kref = numpy.where(below.any(axis=0), nz - 1 - numpy.argmax(below[::-1], axis=0), 0)
        # a value exactly on a level: tau_ref is tau_kref itself where c_kref == ZREF or zref <= c_0
        exact = (rng.random(n) < pexact) & ((c[kref, cols] == ZREF) | (c[0] >= ZREF)) & (kref + 2 < nz)
        j = rng.integers(0, m, n)
        th = tau[kref, cols] + rv[j]
        for i in numpy.nonzero(exact)[0]:
            ks = [k for k in range(kref[i] + 1, nz) if tau[k, i] >= th[i]]
            if ks and ks[0] > kref[i] + 1 - (1 if tau[kref[i], i] < th[i] else 0):
                tau[ks[0], i] = th[i]
    elif not relative and nz > 1:
        exact = rng.random(n) < pexact
        j = rng.integers(0, m, n)
        for i in numpy.nonzero(exact)[0]:
            ks = [k for k in range(nz) if tau[k, i] >= rv[j[i]]]
            if ks and ks[0] >= 1:
                tau[ks[0], i] = rv[j[i]]
    if nz > 2:
        # non-monotone tails: what lies below the first crossing must not matter
        wig = rng.random(n) < 0.3
        tau[nz // 2:, wig] = numpy.round(rng.uniform(0.0, 30.0, (nz - nz // 2, int(wig.sum()))) * 64.0) / 64.0
    if sense < 0:
        tau = FLIP - tau
    tau = tau.astype(real)
    e3t = h.astype(real) if form == 'e3t' else None
    # +-inf in the tracer
    for val in (numpy.inf, -numpy.inf):
        hit = rng.choice(n, max(n // 100, 1), replace=False)
        tau[rng.integers(0, nz, hit.size), hit] = dt(val)
    # dry columns and columns that end early
    kinds = rng.random(n)
    for lo, hi, mark in ((0.00, 0.03, TFILL), (0.03, 0.06, TMISSING), (0.06, 0.09, numpy.nan)):
        tau[0, (kinds >= lo) & (kinds < hi)] = dt(mark)
    for lo, hi, mark in ((0.09, 0.14, TFILL), (0.14, 0.19, TMISSING), (0.19, 0.24, numpy.nan)):
        sel = numpy.nonzero((kinds >= lo) & (kinds < hi))[0]
        tau[rng.integers(0, nz, sel.size), sel] = dt(mark)
    if nz == 1 and relative and form != 'e3t':
        # one level in relative mode knows two outcomes only, dry and the sea bed: neither may pass 60 %
        tau[0, (kinds >= 0.5) & (kinds < 0.72)] = dt(numpy.nan)
    if form == 'e3t':
        for lo, hi, mark in ((0.24, 0.27, 0.0), (0.27, 0.30, -4.0), (0.30, 0.33, EFILL), (0.33, 0.36, EMISSING),
                             (0.36, 0.39, numpy.nan), (0.39, 0.41, numpy.inf)):
            sel = numpy.nonzero((kinds >= lo) & (kinds < hi))[0]
            e3t[rng.integers(0, nz, sel.size), sel] = dt(mark)
        e3t[0, (kinds >= 0.41) & (kinds < 0.43)] = dt(0.0)       # dry by the thickness alone
        e3t = e3t.reshape(nz, ny, nx)
    return tau.reshape(nz, ny, nx), (hlev if form != 'e3t' else None), e3t, values


def _five_columns(real, nz, m, sense, relative, form):
    """a launch of 5 columns, made by hand so that each branch that exists holds one column in five for every value: absolute
    mode dry, sea bed, outcrop, interpolated, exact; relative mode (zref = c_1, so tau_ref = tau_1) dry, sea bed, exact and
    two interpolated"""
    assert nz == 7 and m == 3
    h = level_thickness(nz)
    if relative:        # theta = 5.125, 5.5, 7
        cols = [[0.0] * 7, [5.0] * 7, [3.0, 5.0, 8.0, 9.0, 10.0, 11.0, 12.0], [3.0, 5.0, 5.125, 5.5, 7.0, 8.0, 9.0],
                [3.0, 5.0, 6.0, 6.25, 8.0, 9.0, 10.0]]
    else:               # theta = 9.5, 11.5, 13.25
        cols = [[0.0] * 7, [1.0, 2.0, 3.0, 4.0, 5.0, 6.0, 7.0], [20.0, 21.0, 22.0, 23.0, 24.0, 25.0, 26.0],
                [5.0, 9.0, 10.0, 12.0, 14.0, 15.0, 16.0], [5.0, 9.5, 11.5, 13.25, 14.0, 15.0, 16.0]]
    tau = numpy.array(cols).T.copy()
    if sense < 0:
        tau = FLIP - tau
    tau = tau.astype(real)
    tau[0, 0] = numpy.dtype(real).type(TFILL)
    e3t = numpy.ascontiguousarray(numpy.broadcast_to(h.reshape(nz, 1), (nz, 5))).astype(real).reshape(nz, 1, 5)
    return tau.reshape(nz, 1, 5), (h if form != 'e3t' else None), (e3t if form == 'e3t' else None), case_values(m, sense, relative)


def atzref_case(real, ny, nx, sense):
    """a relative case of 7 levels with e3t whose offsets include values <= 0 (ATZREF_VALUES): the inputs of the (37, 73)-like
    relative cases, where uniform layers around zref and columns with c_kref == zref let level kref itself pass the threshold"""
    tau, _, e3t, _ = make_case(real, 7, ny, nx, 3, sense, True, 'e3t', seed=7)
    v = numpy.array(ATZREF_VALUES)
    return tau, e3t, (v if sense > 0 else -v)


def case_reference(real, nz, ny, nx, m, sense, relative, form, with_branches=False, seed=0):
    tau, thk, e3t, values = make_case(real, nz, ny, nx, m, sense, relative, form, seed)
    return iso_depth(tau, values, sense, thickness=thk, e3t=e3t, top=0.0, relative=relative, zref=ZREF,
                     tau_markers=(TFILL, TMISSING), e3t_markers=(EFILL, EMISSING), with_branches=with_branches)


def raw_cases():
    """the cases of the raw-ABI tests: both grids, nz = 1, 7 and 75, both dtypes, each with the level vector and with e3t, in
    absolute and relative mode; m = 1, 3, 8 and the two senses go round so that every pair of settings meets; and a launch of
    5 columns per dtype"""
    cases, i = [], 0
    for real in ('float64', 'float32'):
        for nz in (1, 7, 75):
            for ny, nx in ((36, 72), (37, 73)):
                for relative in (False, True):
                    for form in ('levels', 'e3t'):
                        cases.append((real, nz, ny, nx, (1, 3, 8)[i % 3], (1, -1)[(i // 3 + i // 2) % 2], relative, form))
                        i += 1
        cases.append((real, 7, 1, 5, 3, 1, False, 'levels'))
        cases.append((real, 7, 1, 5, 3, -1, True, 'e3t'))
    return cases


def case_id(case):
    real, nz, ny, nx, m, sense, relative, form = case
    return f'{real}-{nz}x{ny}x{nx}-m{m}-{"rising" if sense > 0 else "falling"}-{"rel" if relative else "abs"}-{form}'
