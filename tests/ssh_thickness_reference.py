"""The numpy restatement of nf_column_depth and nf_ssh_thickness (include/nemoflux_amd.h): z* layer thicknesses at the U and V
faces from the sea surface height, e3u0 * (1 + ssh_u / hu0).  Everything is float64, every operation one correctly rounded
IEEE operation in the order of the definition, inputs widened first, each result rounded once to the dtype of the inputs -- so
the device gives these bits.

column_depth / ssh_thickness are the restatement, vectorised over the grid; column_depth_loop / ssh_thickness_loop the same
definition as a scalar Python loop over faces and levels (tests/test_ssh_thickness_cpu.py holds the two against each other).
make_case / raw_cases / series are the inputs of the GPU tests: statics on the lattice of the multiples of 1/8 in [0.25, 4] with
partial-step columns (a per-column bottom level below which the static is the marker; some columns have no level at all),
exact zeros, both markers and NaN; ssh on the multiples of 1/8 in [-2, 2] with both markers and NaN; areas on the multiples of
1/4 in [1, 8] with a few NaN and a few face areas <= 0."""
import numpy

from face_thickness_reference import present, same_bits, _neighbours, _geometry, _present1      # noqa: F401
from face_thickness_reference import WIDE_SHAPES, boundary_columns, chunk_and_lane, chunks_of, lane_forms, lane_width  # noqa: F401

EFILL, EMISSING = 1.e20, -999.0              # the markers of ssh
SFILL, SMISSING = 9.96921e36, -32768.0       # the markers of the statics
EM, SM = (EFILL, EMISSING), (SFILL, SMISSING)
# the branches a face (k, j, i) can take; they overlap (a face below the bottom of a column without water is both F0_MISSING
# and H_ZERO), so they are masks and not codes
BOTH, ONE_MISSING, NO_NEIGHBOUR, F0_MISSING, H_ZERO, AREA_FALLBACK = 'both', 'one-missing', 'no-neighbour', 'F0-missing', \
    'H-zero', 'area-fallback'


def column_depth(e3_0, static_markers=()):
    """(ny, nx) float64: H = +0.0, then H = H + (double)F0[k] for k ascending where F0[k] is present"""
    e3_0 = numpy.asarray(e3_0)
    H = numpy.zeros(e3_0.shape[1:], numpy.float64)
    ok = present(e3_0, static_markers)
    with numpy.errstate(all='ignore'):
        for k in range(e3_0.shape[0]):
            H = numpy.where(ok[k], H + e3_0[k].astype(numpy.float64), H)
    return H


def _factor(Sa, Sb, Ta, Tb, F, H, has, markers):
    """the factor f = 1 + s / H of one face plane and its branch masks"""
    both = present(Sa, markers) & present(Sb, markers)
    a, b = Sa.astype(numpy.float64), Sb.astype(numpy.float64)
    zero = numpy.zeros(Sa.shape, numpy.float64)
    with numpy.errstate(all='ignore'):
        if Ta is None:
            s = numpy.where(both, 0.5 * (a + b), zero)
            fallback = numpy.zeros(Sa.shape, bool)
        else:
            p, q = Ta * a, Tb * b
            good = ~numpy.isnan(Ta) & ~numpy.isnan(Tb) & (F > 0)
            s = numpy.where(both & good, (0.5 * (p + q)) / F, zero)
            fallback = both & ~good
        r = numpy.where(H > 0, s / H, zero)
        f = 1.0 + r
    masks = {BOTH: has & both & ~fallback, ONE_MISSING: has & ~both, NO_NEIGHBOUR: ~has & numpy.ones(Sa.shape, bool),
             H_ZERO: ~(H > 0) & numpy.ones(Sa.shape, bool), AREA_FALLBACK: fallback}
    return f, masks


def ssh_thickness(ssh, e3u0, e3v0, hu0=None, hv0=None, areas=None, wrap=True, markers=(), static_markers=(),
                  with_branches=False):
    """(e3u, e3v) of ssh (..., ny, nx) and the statics (nz, ny, nx) by the definition: (..., nz, ny, nx) of the dtype of the
    statics.  hu0 / hv0 None: column_depth of the statics.  areas: None or (area_t, area_u, area_v), float64 (ny, nx).
    with_branches: also the dicts of branch masks of the U and of the V faces."""
    ssh, e3u0, e3v0 = numpy.asarray(ssh), numpy.asarray(e3u0), numpy.asarray(e3v0)
    real = e3u0.dtype
    assert ssh.dtype == real and e3v0.dtype == real
    hu0 = column_depth(e3u0, static_markers) if hu0 is None else numpy.asarray(hu0, numpy.float64)
    hv0 = column_depth(e3v0, static_markers) if hv0 is None else numpy.asarray(hv0, numpy.float64)
    Se, Sn = _neighbours(ssh, wrap)
    has_e, has_n = _geometry(ssh.shape, wrap)
    if areas is None:
        T = Te = Tn = Fu = Fv = None
    else:
        T, Fu, Fv = (numpy.asarray(a, numpy.float64) for a in areas)
        Te, Tn = _neighbours(numpy.array(T), wrap)
    out, branches = [], []
    for Sb, Tb, F, H, has, F0 in ((Se, Te, Fu, hu0, has_e, e3u0), (Sn, Tn, Fv, hv0, has_n, e3v0)):
        f, masks = _factor(ssh, Sb, T, Tb, F, H, has, markers)
        ok = present(F0, static_markers)
        with numpy.errstate(all='ignore'):
            val = F0.astype(numpy.float64) * f[..., None, :, :]
            out.append(numpy.where(ok, val, 0.0).astype(real))
        shape = out[-1].shape
        masks = {k: numpy.broadcast_to(m[..., None, :, :], shape) for k, m in masks.items()}
        masks[F0_MISSING] = numpy.broadcast_to(~ok, shape)
        branches.append(masks)
    return (out[0], out[1], branches[0], branches[1]) if with_branches else (out[0], out[1])


def column_depth_loop(e3_0, static_markers=()):
    nz, ny, nx = e3_0.shape
    dt = e3_0.dtype.type
    H = numpy.empty((ny, nx), numpy.float64)
    with numpy.errstate(all='ignore'):
        for j in range(ny):
            for i in range(nx):
                h = numpy.float64(0.0)
                for k in range(nz):
                    if _present1(e3_0[k, j, i], dt, static_markers):
                        h = h + numpy.float64(e3_0[k, j, i])
                H[j, i] = h
    return H


def ssh_thickness_loop(ssh, e3u0, e3v0, hu0=None, hv0=None, areas=None, wrap=True, markers=(), static_markers=()):
    """the definition face by face and level by level, in numpy.float64 scalars, for ssh (ny, nx) and statics (nz, ny, nx)"""
    nz, ny, nx = e3u0.shape
    dt = e3u0.dtype.type
    f64 = numpy.float64
    depths = [column_depth_loop(s, static_markers) if h is None else numpy.asarray(h, f64)
              for s, h in ((e3u0, hu0), (e3v0, hv0))]
    out = [numpy.empty(e3u0.shape, e3u0.dtype), numpy.empty(e3u0.shape, e3u0.dtype)]
    with numpy.errstate(all='ignore'):
        for j in range(ny):
            for i in range(nx):
                for which in (0, 1):
                    if which == 0:
                        nb = (j, i + 1) if i + 1 < nx else ((j, 0) if wrap else None)
                    else:
                        nb = (j + 1, i) if j + 1 < ny else None
                    sa = ssh[j, i]
                    sb = sa if nb is None else ssh[nb]
                    both = _present1(sa, dt, markers) and _present1(sb, dt, markers)
                    if areas is None:
                        s = f64(0.5) * (f64(sa) + f64(sb)) if both else f64(0.0)
                    else:
                        ta = f64(areas[0][j, i])
                        tb = ta if nb is None else f64(areas[0][nb])
                        F = f64(areas[1 + which][j, i])
                        p, q = ta * f64(sa), tb * f64(sb)
                        if both and ta == ta and tb == tb and F > 0:
                            s = (f64(0.5) * (p + q)) / F
                        else:
                            s = f64(0.0)
                    H = f64(depths[which][j, i])
                    r = s / H if H > 0 else f64(0.0)
                    f = f64(1.0) + r
                    F0 = (e3u0, e3v0)[which]
                    for k in range(nz):
                        x = F0[k, j, i]
                        out[which][k, j, i] = dt(f64(x) * f) if _present1(x, dt, static_markers) else dt(0.0)
    return out[0], out[1]


# ---- inputs ---------------------------------------------------------------------------------------------------------------------
def _static(rng, real, nz, ny, nx):
    dt = numpy.dtype(real).type
    a = (rng.integers(2, 33, (nz, ny, nx)) / 8.).astype(real)
    bottom = rng.integers(0, nz + 1, (ny, nx))            # the number of levels of the column; 0: no level at all
    with numpy.errstate(over='ignore'):
        a[numpy.arange(nz)[:, None, None] >= bottom[None]] = dt(SFILL)
        for m in (0.0, SFILL, SMISSING, numpy.nan):
            a[rng.random(a.shape) < 0.03] = dt(m)
        a[:, bottom == 0] = dt(SFILL)                     # nothing scattered into a column without water
    return a


def _plane(rng, lo, hi, step, shape, specials, rate):
    a = rng.integers(int(lo / step), int(hi / step) + 1, shape) * step
    for m in specials:
        a[rng.random(shape) < rate] = m
    return a


def make_case(real, nz, ny, nx, seed=0):
    """dict(ssh (ny, nx), e3u0, e3v0 (nz, ny, nx), hu0, hv0 (the supplied column depths: not those of the statics), areas)"""
    rng = numpy.random.default_rng(4000 + seed)
    e3u0, e3v0 = _static(rng, real, nz, ny, nx), _static(rng, real, nz, ny, nx)
    with numpy.errstate(over='ignore'):
        ssh = _plane(rng, -2.0, 2.0, 0.125, (ny, nx), (EFILL, EMISSING, numpy.nan), 0.04).astype(real)
    hu0, hv0 = (_plane(rng, 4.0, 40.0, 0.25, (ny, nx), (0.0, numpy.nan, -3.0), 0.02) for _ in range(2))
    at = _plane(rng, 1.0, 8.0, 0.25, (ny, nx), (numpy.nan,), 0.02)
    au, av = (_plane(rng, 1.0, 8.0, 0.25, (ny, nx), (numpy.nan, 0.0, -1.0), 0.01) for _ in range(2))
    return dict(ssh=ssh, e3u0=e3u0, e3v0=e3v0, hu0=hu0, hv0=hv0, areas=(at, au, av))


SHAPES = [(7, 36, 72), (7, 37, 73), (1, 36, 72), (3, 1, 5)]
SMALL_SEED = 90         # the 5-column launch: a seed with which every branch is taken (tests/test_ssh_thickness_cpu.py)


def raw_cases():
    """(real, nz, ny, nx, areas, wrap, supplied) of the raw GPU tests"""
    return [(real, nz, ny, nx, areas, wrap, supplied) for real in ('float64', 'float32') for (nz, ny, nx) in SHAPES
            for areas in (False, True) for wrap in (True, False) for supplied in (False, True)]


# past one column chunk: WIDE_SHAPES of tests/face_thickness_reference.py (nz = 9: a full level group and one of one level),
# kept out of SHAPES as they are there
def wide_cases():
    """(real, nz, ny, nx, areas, wrap, supplied) of the raw GPU tests past one column chunk"""
    return [(real, nz, ny, nx, areas, wrap, supplied) for real in ('float64', 'float32') for (nz, ny, nx) in WIDE_SHAPES[real]
            for areas in (False, True) for wrap in (True, False) for supplied in (False, True)]


def wide_id(case):
    return case_id(case) + '-' + lane_forms(case[3], numpy.dtype(case[0]).itemsize)


def case_id(case):
    real, nz, ny, nx, areas, wrap, supplied = case
    return (f'{real}-{nz}x{ny}x{nx}-{"areas" if areas else "plain"}-{"wrap" if wrap else "nowrap"}-'
            f'{"supplied" if supplied else "computed"}')


def case_inputs(case):
    """(ssh, e3u0, e3v0, keywords of ssh_thickness) of a raw case"""
    real, nz, ny, nx, areas, wrap, supplied = case
    c = make_case(real, nz, ny, nx, SMALL_SEED if nx == 5 else 10 * nz + nx)
    kw = dict(hu0=c['hu0'] if supplied else None, hv0=c['hv0'] if supplied else None, areas=c['areas'] if areas else None,
              wrap=wrap, markers=EM, static_markers=SM)
    return c['ssh'], c['e3u0'], c['e3v0'], kw


def branches_of(case):
    """the branches the definition names for a raw case"""
    real, nz, ny, nx, areas, wrap, supplied = case
    return (BOTH, ONE_MISSING, NO_NEIGHBOUR, F0_MISSING, H_ZERO) + ((AREA_FALLBACK,) if areas else ())


def series(real, grid, nt, nz, seed=0):
    """the inputs of the Field tests on grid = (nx, ny): make_case's dict with ssh (nt, ny, nx) and e3t0 (nz, ny, nx) beside"""
    nx, ny = grid
    c = make_case(real, nz, ny, nx, seed=700 + seed)
    steps = [make_case(real, 1, ny, nx, seed=800 + seed + 7 * t)['ssh'] for t in range(nt)]
    c['ssh'] = numpy.stack(steps)
    c['e3t0'] = _static(numpy.random.default_rng(900 + seed), real, nz, ny, nx)
    return c


def flat_bottom_case(real, nz, ny, nx, total=8.0, seed=0):
    """statics on the 1/8 lattice whose every wet column sums to exactly `total` (dry columns: the marker), ssh on the 1/8
    lattice: every step of the definition is exact"""
    rng = numpy.random.default_rng(5000 + seed)
    dt = numpy.dtype(real).type
    n8 = int(total * 8)
    out = []
    for _ in range(2):
        cuts = numpy.sort(rng.integers(1, n8, (nz - 1, ny, nx)), axis=0)
        edges = numpy.concatenate([numpy.zeros((1, ny, nx), int), cuts, numpy.full((1, ny, nx), n8)])
        a = (numpy.diff(edges, axis=0) / 8.).astype(real)
        with numpy.errstate(over='ignore'):
            a[:, rng.random((ny, nx)) < 0.1] = dt(SFILL)
        out.append(a)
    ssh = (rng.integers(-16, 17, (ny, nx)) / 8.).astype(real)
    return ssh, out[0], out[1]
