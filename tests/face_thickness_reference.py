"""The numpy restatement of nf_face_thickness (include/nemoflux_amd.h): layer thicknesses at the U and V faces from the
thickness at T-points.  Everything is float64, every operation one correctly rounded IEEE operation in the order of the
definition, inputs widened first, each result rounded once to the dtype of the inputs -- so the device gives these bits.

face_thickness is the restatement, vectorised over the grid; face_thickness_loop the same definition as a scalar Python loop
over the faces (tests/test_face_thickness_cpu.py holds the two against each other).  make_case / raw_cases / wide_cases / series are
the inputs of the GPU tests: thicknesses on the lattice of the multiples of 1/8 in [0.25, 4] (tests/depth_remap_reference.py) with
exact zeros, both markers and NaN scattered."""
import numpy

EFILL, EMISSING = 1.e20, -999.0              # the markers of e3t
SFILL, SMISSING = 9.96921e36, -32768.0       # the markers of the statics
MIN, MEAN, ANOMALY = 0, 1, 2
RULES = {'min': MIN, 'mean': MEAN, 'anomaly': ANOMALY}
# the branch a face takes
BOTH, ONE_MISSING, NO_NEIGHBOUR, F0_MISSING, F0_KEPT = 0, 1, 2, 3, 4
BRANCHES = {MIN: (BOTH, ONE_MISSING, NO_NEIGHBOUR), MEAN: (BOTH, ONE_MISSING, NO_NEIGHBOUR),
            ANOMALY: (BOTH, F0_KEPT, NO_NEIGHBOUR, F0_MISSING)}


def same_bits(a, b):
    a, b = numpy.ascontiguousarray(a), numpy.ascontiguousarray(b)
    u = {4: numpy.uint32, 8: numpy.uint64}[a.dtype.itemsize]
    return a.shape == b.shape and a.dtype == b.dtype and numpy.array_equal(a.view(u), b.view(u))


def present(a, markers):
    """not NaN and equal to neither marker, each cast to the dtype of a and compared in that dtype; NaN / None: no marker"""
    a = numpy.asarray(a)
    ok = ~numpy.isnan(a)
    with numpy.errstate(over='ignore'):
        for m in markers:
            if m is not None and m == m:
                ok &= a != a.dtype.type(m)
    return ok


def _neighbours(a, wrap):
    """(east neighbour, north neighbour) of every cell, the cell's own value where there is none by geometry"""
    east = numpy.roll(a, -1, axis=-1)
    if not wrap:
        east[..., -1] = a[..., -1]
    north = numpy.concatenate([a[..., 1:, :], a[..., -1:, :]], axis=-2)
    return east, north


def _geometry(shape, wrap):
    has_e, has_n = numpy.ones(shape, bool), numpy.ones(shape, bool)
    if not wrap:
        has_e[..., -1] = False
    has_n[..., -1, :] = False
    return has_e, has_n


def _face(A, B, A0, B0, F0, has, rule, markers, static_markers):
    """one face array: (values of the dtype of A, branch codes)"""
    real = A.dtype
    both = present(A, markers) & present(B, markers)
    Ad, Bd = A.astype(numpy.float64), B.astype(numpy.float64)
    zero = numpy.zeros(A.shape, numpy.float64)
    with numpy.errstate(all='ignore'):
        if rule == MIN:
            out = numpy.where(both, numpy.where(Bd < Ad, Bd, Ad), zero)
        elif rule == MEAN:
            out = numpy.where(both, 0.5 * (Ad + Bd), zero)
        else:
            pf = present(F0, static_markers)
            every = both & present(A0, static_markers) & present(B0, static_markers)
            F0d = F0.astype(numpy.float64)
            val = F0d + 0.5 * ((Ad - A0.astype(numpy.float64)) + (Bd - B0.astype(numpy.float64)))
            out = numpy.where(pf, numpy.where(every, val, F0d), zero)
        out = out.astype(real)
    if rule == ANOMALY:
        branch = numpy.where(~has, NO_NEIGHBOUR, numpy.where(~pf, F0_MISSING, numpy.where(every, BOTH, F0_KEPT)))
    else:
        branch = numpy.where(~has, NO_NEIGHBOUR, numpy.where(both, BOTH, ONE_MISSING))
    return out, branch


def face_thickness(e3t, rule, e3t0=None, e3u0=None, e3v0=None, wrap=True, markers=(), static_markers=(), with_branches=False):
    """(e3u, e3v) of e3t (..., ny, nx) by the definition; rule: MIN, MEAN, ANOMALY or its name.  with_branches: also the branch
    codes of the U and of the V faces."""
    rule = RULES.get(rule, rule)
    e3t = numpy.asarray(e3t)
    Be, Bn = _neighbours(e3t, wrap)
    has_e, has_n = _geometry(e3t.shape, wrap)
    if rule == ANOMALY:
        e3t0, e3u0, e3v0 = (numpy.broadcast_to(numpy.asarray(x), e3t.shape) for x in (e3t0, e3u0, e3v0))
        B0e, B0n = _neighbours(numpy.array(e3t0), wrap)
    else:
        assert e3t0 is None and e3u0 is None and e3v0 is None
        B0e = B0n = None
    u, bu = _face(e3t, Be, e3t0, B0e, e3u0, has_e, rule, markers, static_markers)
    v, bv = _face(e3t, Bn, e3t0, B0n, e3v0, has_n, rule, markers, static_markers)
    return (u, v, bu, bv) if with_branches else (u, v)


def _present1(x, dt, markers):
    if x != x:
        return False
    with numpy.errstate(over='ignore'):
        return all(not (m is not None and m == m and x == dt(m)) for m in markers)


def face_thickness_loop(e3t, rule, e3t0=None, e3u0=None, e3v0=None, wrap=True, markers=(), static_markers=()):
    """the definition face by face, in Python floats (IEEE float64), for (nz, ny, nx) arrays"""
    rule = RULES.get(rule, rule)
    nz, ny, nx = e3t.shape
    dt = e3t.dtype.type
    out = [numpy.empty(e3t.shape, e3t.dtype), numpy.empty(e3t.shape, e3t.dtype)]
    for z in range(nz):
        for j in range(ny):
            for i in range(nx):
                for which in (0, 1):
                    if which == 0:
                        nb = (z, j, i + 1) if i + 1 < nx else ((z, j, 0) if wrap else None)
                    else:
                        nb = (z, j + 1, i) if j + 1 < ny else None
                    here = (z, j, i)
                    a = e3t[here]
                    b = a if nb is None else e3t[nb]
                    both = _present1(a, dt, markers) and _present1(b, dt, markers)
                    A, B = float(a), float(b)
                    with numpy.errstate(all='ignore'):
                        if rule == MIN:
                            r = dt(B if B < A else A) if both else dt(0.0)
                        elif rule == MEAN:
                            r = dt(numpy.float64(0.5) * (numpy.float64(A) + numpy.float64(B))) if both else dt(0.0)
                        else:
                            f0 = (e3u0, e3v0)[which][here]
                            a0 = e3t0[here]
                            b0 = a0 if nb is None else e3t0[nb]
                            if not _present1(f0, dt, static_markers):
                                r = dt(0.0)
                            elif both and _present1(a0, dt, static_markers) and _present1(b0, dt, static_markers):
                                d = (numpy.float64(A) - numpy.float64(a0)) + (numpy.float64(B) - numpy.float64(b0))
                                r = dt(numpy.float64(f0) + numpy.float64(0.5) * d)
                            else:
                                r = f0
                    out[which][here] = r
    return out[0], out[1]


# ---- inputs ---------------------------------------------------------------------------------------------------------------------
def _lattice(rng, real, shape, marks, rate):
    dt = numpy.dtype(real).type
    a = (rng.integers(2, 33, shape) / 8.).astype(real)
    with numpy.errstate(over='ignore'):
        for m in (0.0,) + tuple(marks) + (numpy.nan,):
            a[rng.random(shape) < rate] = dt(m)
    return a


def make_case(real, nz, ny, nx, rule, seed=0):
    """(e3t, e3t0, e3u0, e3v0) of shape (nz, ny, nx), the statics None unless rule is ANOMALY: multiples of 1/8 in [0.25, 4]
    with exact zeros, both markers and NaN scattered"""
    rule = RULES.get(rule, rule)
    rng = numpy.random.default_rng(1000 + seed)
    shape = (nz, ny, nx)
    e3t = _lattice(rng, real, shape, (EFILL, EMISSING), 0.04)
    if rule != ANOMALY:
        return e3t, None, None, None
    return (e3t,) + tuple(_lattice(rng, real, shape, (SFILL, SMISSING), 0.03) for _ in range(3))


SHAPES = [(1, 36, 72), (7, 36, 72), (1, 37, 73), (7, 37, 73), (3, 1, 5)]
SMALL_SEED = {MIN: 1, MEAN: 1, ANOMALY: 1}      # the 5-column launch: seeds with which every branch is taken


def raw_cases():
    """(real, nz, ny, nx, rule, wrap) of the raw GPU tests"""
    return [(real, nz, ny, nx, rule, wrap) for real in ('float64', 'float32') for (nz, ny, nx) in SHAPES
            for rule in (MIN, MEAN, ANOMALY) for wrap in (True, False)]


# Past one column chunk.  The kernels deal a row out in chunks of 256 lanes of VEC = 16 / itemsize values each, of one value
# each when a base or nx does not allow 16-byte lanes; the shapes are the smallest that reach: one full chunk (lane 255 holds
# the wrap); two chunks, the last of one lane (one value per lane: three chunks); three chunks with several row and level
# groups; an odd nx (one value per lane whatever the bases).  They are kept out of SHAPES: the scalar loops run over those whole.
WIDE_SHAPES = {'float64': [(2, 5, 512), (2, 5, 514), (9, 6, 1026), (2, 5, 515)],
               'float32': [(2, 5, 1024), (2, 5, 1028), (9, 6, 2052), (2, 5, 1027)]}
LANES = 256


def wide_cases():
    """(real, nz, ny, nx, rule, wrap) of the raw GPU tests past one column chunk"""
    return [(real, nz, ny, nx, rule, wrap) for real in ('float64', 'float32') for (nz, ny, nx) in WIDE_SHAPES[real]
            for rule in (MIN, MEAN, ANOMALY) for wrap in (True, False)]


def lane_width(nx, itemsize, moved=False):
    """the values a lane holds: 16 bytes' worth when every base is 16-byte aligned (moved: one of them is not) and nx is a
    multiple of that, else one"""
    vec = 16 // itemsize
    return 1 if moved or nx % vec else vec


def chunks_of(nx, vec):
    return -(-nx // (LANES * vec))


def chunk_and_lane(x, vec):
    """where column x falls: (chunk, lane) with vec values per lane"""
    return x // (LANES * vec), x % (LANES * vec) // vec


def boundary_columns(nx, itemsize):
    """the columns whose east neighbour another chunk holds, in the 16-byte lane form and in the one-value form (k * P - 1 <
    nx - 1 for P = 256 * VEC and P = 256), and the last column, whose east neighbour is column 0 or none"""
    cols = {nx - 1}
    for per_chunk in (LANES * (16 // itemsize), LANES):
        cols.update(range(per_chunk - 1, nx - 1, per_chunk))
    return sorted(cols)


def lane_forms(nx, itemsize):
    """the lane forms a wide case runs in, as vec{VEC}x{chunks}: with the bases as the allocator gives them and then with one
    of them moved by one element"""
    forms = []
    for moved in (False, True):
        vec = lane_width(nx, itemsize, moved)
        form = f'vec{vec}x{chunks_of(nx, vec)}'
        if form not in forms:
            forms.append(form)
    return '+'.join(forms)


def wide_id(case):
    return case_id(case) + '-' + lane_forms(case[3], numpy.dtype(case[0]).itemsize)


def case_seed(case):
    real, nz, ny, nx, rule, wrap = case
    return SMALL_SEED[rule] if nx == 5 else 10 * nz + rule


def case_id(case):
    real, nz, ny, nx, rule, wrap = case
    return f'{real}-{nz}x{ny}x{nx}-{("min", "mean", "anomaly")[rule]}-{"wrap" if wrap else "nowrap"}'


def case_arrays(case):
    real, nz, ny, nx, rule, wrap = case
    return make_case(real, nz, ny, nx, rule, case_seed(case))


def series(real, grid, nt, nz, rule):
    """(e3t (nt, nz, ny, nx), e3t0, e3u0, e3v0 (nz, ny, nx) or None) of the Field tests on grid = (nx, ny)"""
    nx, ny = grid
    steps = [make_case(real, nz, ny, nx, rule, seed=500 + 7 * t) for t in range(nt)]
    return (numpy.stack([s[0] for s in steps]),) + steps[0][1:]


def want_series(e3t, rule, statics=(None, None, None), wrap=True):
    """the restatement's (e3u, e3v) of a series (nt, nz, ny, nx) or of a static (nz, ny, nx), the markers those above"""
    return face_thickness(e3t, rule, *statics, wrap=wrap, markers=(EFILL, EMISSING), static_markers=(SFILL, SMISSING))
