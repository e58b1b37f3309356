"""A dense probe of the tracer planes of K1tau (k_tracer_flux), shared by tests/test_gpu_tracer_planes.py and its CPU twin
tests/test_tracer_planes_cpu.py.  Nothing here touches the GPU.

The planes eU_tau, eV_tau have no read-back, but a transect row is a known linear function of them through the weight
entries.  The probe is one zig-zag transect per grid row with one vertex strictly inside every cell of the row: a line set in
which every east face and every north face of the grid -- the wrap faces of the last column and the neighbourless north
faces of the last row included -- has a weight of at least MIN_WEIGHT in some segment's row.  A plane value that is wrong at
any one face then moves some per-segment value by MIN_WEIGHT times the error, which the bar of the tests sees.

Grid: regular cells of CELL = 0.25 degrees on [0, nx / 4] x [0, ny / 4], not periodic (256 rows stay on the sphere).  In cell
(j, i) the vertex sits at xi = 0.6 and eta = 0.3 (even i) or 0.7 (odd i) of the cell.  A segment from cell i to cell i + 1
therefore crosses exactly one east face, with d xi = 0.4 and |d eta| = 0.16 inside cell i, d xi = 0.6 and |d eta| = 0.24 inside
cell i + 1.  With the lowest-order face weights (east: d eta * xi_mid, west: d eta * (1 - xi_mid), north: d xi * eta_mid)

    east slot of cell i       |w| = 0.16 * 0.8 = 0.128  (piece that leaves the cell),  0.24 * 0.3 = 0.072  (piece that arrives)
    west slot of cell i + 1   |w| = 0.24 * 0.7 = 0.168
    north slot of any cell    |w| >= 0.4 * 0.38 = 0.152

so the last column's east face (only an arriving piece) and column 0's west slot (only a leaving piece, 0.16 * 0.2 = 0.032)
are carried too; the probe condition is asserted from the weights, not taken from this arithmetic."""
import numpy

FILL, MISSING = 1.e20, -999.             # uo / vo
TFILL, TMISSING = -32768., 12345.        # the tracer
REFERENCE = 3.25
NZ, NT = 5, 2
CELL = 0.25
MIN_WEIGHT = 0.05
XI, ETA = 0.6, (0.3, 0.7)

# (nx, ny): what each shape is for is stated where the index rules are, in tests/test_tracer_planes_cpu.py
SHAPES = [(7, 128), (11, 256), (129, 64), (61, 35), (128, 34)]
REALS = ['float64', 'float32']


def shape_id(g):
    return f'{g[0]}x{g[1]}'


def probe_box(nx, ny):
    """(xmin, xmax, ymin, ymax) of the grid"""
    return 0., nx * CELL, 0., ny * CELL


def probe_lines(nx, ny):
    """one (nx, 3) polyline per grid row: vertex i strictly inside cell (j, i)"""
    i = numpy.arange(nx)
    out = []
    for j in range(ny):
        xyz = numpy.zeros((nx, 3))
        xyz[:, 0] = (i + XI) * CELL
        xyz[:, 1] = (j + numpy.where(i % 2 == 0, ETA[0], ETA[1])) * CELL
        out.append(xyz)
    return out


def probe_seed(nx, ny):
    return nx * 100 + ny


def probe_inputs(real, nx, ny, seed=None):
    """u, v ~ N(0, 1) with _FillValue, a second missing value and NaN; tau = 10 + 5 N(0, 1) with both tracer markers and NaN
    on about a seventh of the cells each: faces with both, one and no side present.  (NT, NZ, ny, nx) of `real`."""
    rng = numpy.random.default_rng(probe_seed(nx, ny) if seed is None else seed)
    dt = numpy.dtype(real).type
    shape = (NT, NZ, ny, nx)
    u = rng.standard_normal(shape).astype(dt)
    v = rng.standard_normal(shape).astype(dt)
    u.reshape(-1)[rng.choice(u.size, u.size // 9, replace=False)] = dt(FILL)
    v.reshape(-1)[rng.choice(v.size, v.size // 9, replace=False)] = numpy.nan
    u.reshape(-1)[rng.choice(u.size, u.size // 11, replace=False)] = dt(MISSING)
    v.reshape(-1)[rng.choice(v.size, v.size // 11, replace=False)] = dt(MISSING)
    tau = (10. + 5. * rng.standard_normal(shape)).astype(dt)
    for m in (TFILL, TMISSING, numpy.nan):
        tau.reshape(-1)[rng.choice(tau.size, tau.size // 7, replace=False)] = dt(m)
    return u, v, tau


def probe_thickness(real, nx, ny, nt_th):
    """e3u, e3v (nt_th, NZ, ny, nx) on the lattice of the depth-bin tests: multiples of 1/8 in [0.25, 4], exact zeros, both
    thickness markers and NaN"""
    from depth_remap_reference import depth_thickness
    return depth_thickness(real, (nt_th, NZ, ny, nx), probe_seed(nx, ny) + 1)


def probe_condition(cell_slot, weight, coverage, nx, ny, wrap):
    """the probe condition, from weight entries (cell * 4 + slot; slots south, east, north, west).  Returns a list of what
    fails (empty: the condition holds): every cell's east face (east slot of the cell or west slot of its east neighbour, which
    with `wrap` is column 0 for the last column) and every cell's north face (north slot of the cell or south slot of the cell
    above) has |w| >= MIN_WEIGHT in some entry, and the coverage of every segment is 1."""
    ce = numpy.asarray(cell_slot, dtype=numpy.int64)
    w = numpy.abs(numpy.asarray(weight, dtype=numpy.float64))
    ncell = nx * ny
    best = numpy.zeros((ncell, 4))
    numpy.maximum.at(best.reshape(-1), ce, w)
    c = numpy.arange(ncell)
    j, i = c // nx, c % nx
    east_nb = numpy.where(i < nx - 1, c + 1, c + 1 - nx)
    has_east_nb = (i < nx - 1) | bool(wrap)
    east = numpy.maximum(best[:, 1], numpy.where(has_east_nb, best[east_nb, 3], 0.0))
    north_nb = numpy.minimum(c + nx, ncell - 1)
    north = numpy.maximum(best[:, 2], numpy.where(j < ny - 1, best[north_nb, 0], 0.0))
    bad = []
    if not (east >= MIN_WEIGHT).all():
        bad.append(f'east faces of cells {numpy.flatnonzero(east < MIN_WEIGHT)[:8].tolist()} carry less than {MIN_WEIGHT}')
    if not (north >= MIN_WEIGHT).all():
        bad.append(f'north faces of cells {numpy.flatnonzero(north < MIN_WEIGHT)[:8].tolist()} carry less than {MIN_WEIGHT}')
    cov = numpy.concatenate([numpy.asarray(x, dtype=numpy.float64).reshape(-1) for x in coverage])
    if cov.size != ny * (nx - 1) or not (numpy.abs(cov - 1.0) <= 1e-12).all():
        bad.append(f'coverage: {cov.size} segments, min {cov.min():.17g}, max {cov.max():.17g}')
    return bad


def face_presence(tau, nx, ny, wrap):
    """the number of present sides (0, 1, 2) of the faces at the rim, per step and level: the east faces of column nx - 1
    (second cell: column 0 with `wrap`, else none) (NT, NZ, ny); the faces between the last two rows (NT, NZ, nx); the north
    faces of the last row, which have no second cell (NT, NZ, nx)"""
    dt = tau.dtype.type
    ok = (~numpy.isnan(tau) & (tau != dt(TFILL)) & (tau != dt(TMISSING))).astype(int)
    east = ok[..., :, nx - 1] + (ok[..., :, 0] if wrap else 0)
    below = ok[..., ny - 2, :] + ok[..., ny - 1, :]
    return east, below, ok[..., ny - 1, :]
