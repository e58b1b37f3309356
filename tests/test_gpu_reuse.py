"""One handle of the C ABI re-used through its setters, in any order: every result equals, bit for bit, that of a fresh
handle given only the final state.  The device buffers of a handle follow the sizes of its latest inputs -- in particular
the staging slabs of host-resident fields, which a larger grid or more levels must grow."""
import ctypes

import numpy
import pytest

pytestmark = pytest.mark.gpu

NF_F64, NF_F32 = 0, 1
NF_ERR_STATE = 2
GRIDS = [(6, 12), (10, 20), (16, 32), (24, 40)]
TRANSECTS = [[(-170., -60.), (-20., 10.), (150., 70.)], [(-100., 50.), (100., -50.)], [(10., -75.), (10., 75.)],
             [(-150., 0.), (-90., 30.), (0., -20.), (120., 40.)]]


def lib_check():
    from nemoflux_amd._lib import lib, check
    return lib, check


def xyz(points):
    a = numpy.zeros((len(points), 3))
    a[:, :2] = points
    return a


def grid_bounds(ny, nx, dtype):
    """(ny, nx, 4) corner longitudes / latitudes of a lon-lat grid (corners SW, SE, NE, NW), mildly irregular."""
    lon = numpy.linspace(-180., 180., nx + 1)
    lat = numpy.linspace(-80., 80., ny + 1) + 3. * numpy.sin(numpy.linspace(0., 3., ny + 1))
    blon = numpy.broadcast_to(numpy.stack([lon[:-1], lon[1:], lon[1:], lon[:-1]], -1)[None], (ny, nx, 4))
    blat = numpy.broadcast_to(numpy.stack([lat[:-1], lat[:-1], lat[1:], lat[1:]], -1)[:, None], (ny, nx, 4))
    return numpy.ascontiguousarray(blon, dtype), numpy.ascontiguousarray(blat, dtype)


def velocities(rng, nt, nz, ny, nx, dtype, fill):
    u = rng.standard_normal((nt, nz, ny, nx)).astype(dtype)
    v = rng.standard_normal((nt, nz, ny, nx)).astype(dtype)
    if fill is not None:
        land = rng.random((ny, nx)) < 0.15
        u[:, :, land] = fill
        v[:, :, land] = fill
    return u, v


class Handle:
    """An nf_field handle and the arrays it borrows (kept alive here)."""

    def __init__(self):
        self.lib, self.check = lib_check()
        self.h = ctypes.c_void_p()
        self.check(self.lib.nf_field_new(ctypes.byref(self.h)))
        self.keep = {}

    def __del__(self):
        self.lib.nf_field_del(ctypes.byref(self.h))

    def call(self, name, *args):
        self.check(getattr(self.lib, 'nf_field_' + name)(ctypes.byref(self.h), *args))

    def set_bounds(self, ny, nx, dtype, on_device):
        import torch
        blon, blat = grid_bounds(ny, nx, dtype)
        if on_device:
            blon, blat = torch.from_numpy(blon).cuda(), torch.from_numpy(blat).cuda()
            torch.cuda.synchronize()
            ptrs = blon.data_ptr(), blat.data_ptr()
        else:
            ptrs = blon.ctypes.data, blat.ctypes.data
        self.call('set_bounds', ptrs[0], ptrs[1], ny, nx, NF_F32 if dtype == numpy.float32 else NF_F64, int(on_device))

    def set_thickness(self, thick):
        self.keep['thick'] = thick
        self.call('set_thickness', thick.ctypes.data_as(ctypes.POINTER(ctypes.c_double)), thick.size)

    def set_uv(self, u, v, on_device, fill):
        import torch
        code = NF_F32 if u.dtype == numpy.float32 else NF_F64
        if on_device:
            u, v = torch.from_numpy(u).cuda(), torch.from_numpy(v).cuda()
            torch.cuda.synchronize()
            ptrs = u.data_ptr(), v.data_ptr()
        else:
            ptrs = u.ctypes.data, v.ctypes.data
        self.keep['uv'] = (u, v)
        self.call('set_uv', ptrs[0], ptrs[1], u.shape[0], code, int(on_device), float('nan') if fill is None else fill)

    def add_transect(self, points):
        a = xyz(points)
        self.call('add_transect', a.ctypes.data_as(ctypes.POINTER(ctypes.c_double)), a.shape[0], 0, None)

    def rowlen(self):
        n = ctypes.c_int()
        self.call('row_length', ctypes.byref(n))
        return n.value

    def compute(self, kind, t, ncell):
        """(rows, iV (ncell,4), |eU|, |eV|, running max) of one compute call."""
        import torch
        dp = ctypes.POINTER(ctypes.c_double)
        if kind != 'read':
            self.call('reset_max')
        if kind == 'flux':
            rows = numpy.full(self.rowlen(), numpy.nan)
            self.call('compute_flux', t, rows.ctypes.data_as(dp))
        elif kind == 'all':
            out = torch.full((self.keep['uv'][0].shape[0], self.rowlen()), float('nan'), dtype=torch.float64, device='cuda')
            self.call('compute_all_async', out.data_ptr())
            torch.cuda.synchronize()
            rows = out.cpu().numpy()
        else:                                               # read_step only: the planes of the latest step
            rows = None
        iv, eu, ev, m = numpy.full((ncell, 4), numpy.nan), numpy.full(ncell, numpy.nan), numpy.full(ncell, numpy.nan), \
            ctypes.c_double()
        self.call('read_step', iv.ctypes.data_as(dp), eu.ctypes.data_as(dp), ev.ctypes.data_as(dp), ctypes.byref(m))
        return rows, iv, eu, ev, m.value


def same_bits(a, b):
    return numpy.array_equal(numpy.asarray(a).view(numpy.uint64), numpy.asarray(b).view(numpy.uint64))


class Model:
    """The state a sequence of setter calls leaves; fresh() makes a new handle from it alone."""

    def __init__(self, rng):
        self.rng = rng
        self.grid = None
        self.thick = None
        self.uv = None          # (u, v, on_device, fill)
        self.compact = 0
        self.slab = None
        self.transects = []

    def steps(self):
        return self.uv[0].shape[0]

    def apply(self, h, op):
        rng = self.rng
        if op == 'bounds':
            ny, nx = GRIDS[rng.integers(len(GRIDS))]
            self.grid = (ny, nx, [numpy.float64, numpy.float32][rng.integers(2)], bool(rng.integers(2)))
            h.set_bounds(*self.grid)
        elif op == 'thickness':
            self.thick = rng.uniform(1., 50., int(rng.integers(1, 8)))
            h.set_thickness(self.thick)
        elif op == 'uv':
            self.set_uv(h)
        elif op == 'compact':
            self.compact = int(rng.integers(2))
            h.call('set_compact', self.compact)
        elif op == 'slab':
            self.set_slab(h)
        elif op == 'transect':
            self.transects.append(TRANSECTS[rng.integers(len(TRANSECTS))])
            h.add_transect(self.transects[-1])

    def set_uv(self, h):
        if self.grid is None:
            self.apply(h, 'bounds')
        if self.thick is None:
            self.apply(h, 'thickness')
        ny, nx = self.grid[:2]
        dtype = [numpy.float64, numpy.float32][self.rng.integers(2)]
        fill = [None, 1.e20][self.rng.integers(2)]
        u, v = velocities(self.rng, int(self.rng.integers(1, 4)), self.thick.size, ny, nx, dtype, fill)
        self.uv = (u, v, bool(self.rng.integers(2)), fill)
        h.set_uv(*self.uv)

    def set_slab(self, h):
        total = self.steps() * self.thick.size if self.uv is not None and self.thick is not None else 8
        b = int(self.rng.integers(0, total))
        self.slab = (b, int(self.rng.integers(b + 1, total + 1)))
        h.call('set_slab_range', *self.slab)

    def ready(self, h):
        """Setter calls that make the state computable: fields of the current sizes, an owned slab, built weights."""
        if self.grid is None:
            self.apply(h, 'bounds')
        if self.thick is None:
            self.apply(h, 'thickness')
        ny, nx = self.grid[:2]
        if self.uv is None or self.uv[0].shape[1:] != (self.thick.size, ny, nx):
            self.set_uv(h)
        if self.slab is not None and self.slab[0] >= self.steps() * self.thick.size:
            self.set_slab(h)
        if not self.transects:
            self.apply(h, 'transect')
        h.call('build_weights', 16, 360.)

    def owned_steps(self):
        nz = self.thick.size
        if self.slab is None:
            return list(range(self.steps()))
        return [t for t in range(self.steps()) if t * nz < self.slab[1] and (t + 1) * nz > self.slab[0]]

    def fresh(self):
        f = Handle()
        f.set_bounds(*self.grid)
        f.set_thickness(self.thick)
        f.set_uv(*self.uv)
        if self.compact:
            f.call('set_compact', 1)
        if self.slab is not None:
            f.call('set_slab_range', *self.slab)
        for p in self.transects:
            f.add_transect(p)
        f.call('build_weights', 16, 360.)
        return f


def compare(h, model, kind):
    ncell = model.grid[0] * model.grid[1]
    t = int(model.rng.choice(model.owned_steps()))
    fresh = model.fresh()
    if kind == 'read':                                 # the planes of the same step, computed by each handle
        h.compute('flux', t, ncell)
        fresh.compute('flux', t, ncell)
    got, want = h.compute(kind, t, ncell), fresh.compute(kind, t, ncell)
    for g, w in zip(got, want):
        assert (g is None and w is None) or same_bits(g, w), (kind, t)


def run_sequence(seed, nops=16):
    rng = numpy.random.default_rng(seed)
    model, h = Model(rng), Handle()
    ops = ['bounds', 'thickness', 'uv', 'compact', 'slab', 'transect', 'compute']
    for _ in range(nops):
        op = ops[rng.integers(len(ops))]
        if op == 'compute':
            model.ready(h)
            compare(h, model, ['flux', 'all', 'read'][rng.integers(3)])
        else:
            model.apply(h, op)
    model.ready(h)
    compare(h, model, 'flux')


@pytest.mark.parametrize('seed', range(12))
def test_field_handle_reuse_equals_fresh_handle(seed):
    run_sequence(seed)


def test_host_staged_step_grows_with_the_grid_and_the_levels():
    """A small host-resident step first, then a larger grid with more levels on the same handle: the staging slabs grow
    with the step (they used to keep the size of the first one).  float32 first, float64 after: more bytes again."""
    rng = numpy.random.default_rng(7)
    model, h = Model(rng), Handle()
    model.grid = (6, 12, numpy.float64, False)
    h.set_bounds(*model.grid)
    model.thick = numpy.array([10., 20.])
    h.set_thickness(model.thick)
    u, v = velocities(rng, 2, 2, 6, 12, numpy.float32, None)
    model.uv = (u, v, False, None)
    h.set_uv(*model.uv)
    model.transects.append(TRANSECTS[0])
    h.add_transect(TRANSECTS[0])
    h.call('build_weights', 16, 360.)
    h.compute('flux', 1, 6 * 12)
    model.grid = (24, 40, numpy.float32, False)
    h.set_bounds(*model.grid)
    model.thick = rng.uniform(1., 50., 7)
    h.set_thickness(model.thick)
    u, v = velocities(rng, 3, 7, 24, 40, numpy.float64, 1.e20)
    model.uv = (u, v, False, 1.e20)
    h.set_uv(*model.uv)
    h.call('build_weights', 16, 360.)
    for kind in ('flux', 'all', 'read'):
        compare(h, model, kind)


# ----------------------------------------------------------------------------------------------------- Level 1
def grid_points(ny, nx):
    blon, blat = grid_bounds(ny, nx, numpy.float64)
    pts = numpy.zeros((ny * nx, 4, 3))
    pts[:, :, 0] = blon.reshape(-1, 4)
    pts[:, :, 1] = blat.reshape(-1, 4)
    return pts


def test_level1_objects_reuse_equals_fresh_objects():
    lib, check = lib_check()
    dp = ctypes.POINTER(ctypes.c_double)
    rng = numpy.random.default_rng(3)
    pts = grid_points(16, 32)
    grid = ctypes.c_void_p()
    check(lib.mnt_grid_new(ctypes.byref(grid)))
    check(lib.mnt_grid_setPointsPtr(ctypes.byref(grid), pts.ctypes.data_as(dp)))
    check(lib.mnt_grid_build(ctypes.byref(grid), 4, pts.shape[0]))
    data = rng.standard_normal((pts.shape[0], 4))

    def pli_new():
        p = ctypes.c_void_p()
        check(lib.mnt_polylineintegral_new(ctypes.byref(p)))
        check(lib.mnt_polylineintegral_setGrid(ctypes.byref(p), grid))
        check(lib.mnt_polylineintegral_buildLocator(ctypes.byref(p), 16, 360., 0))
        return p

    def pli_weights(p, line):
        a = xyz(line)
        check(lib.mnt_polylineintegral_computeWeights(ctypes.byref(p), a.shape[0], a.ctypes.data_as(dp), 0))

    def pli_results(p):
        host, dev = ctypes.c_double(), ctypes.c_double()
        check(lib.mnt_polylineintegral_getIntegral(ctypes.byref(p), data.ctypes.data_as(dp), 0, ctypes.byref(host)))
        import torch
        d = torch.from_numpy(data).cuda()
        torch.cuda.synchronize()
        check(lib.mnt_polylineintegral_getIntegralDev(ctypes.byref(p), d.data_ptr(), 0, ctypes.byref(dev), None))
        n = ctypes.c_size_t()
        check(lib.mnt_polylineintegral_getNumberOfWeights(ctypes.byref(p), ctypes.byref(n)))
        ce, w = numpy.zeros(n.value, numpy.int64), numpy.zeros(n.value)
        check(lib.mnt_polylineintegral_getWeights(ctypes.byref(p), ce.ctypes.data_as(ctypes.POINTER(ctypes.c_int64)),
                                                  w.ctypes.data_as(dp), None))
        return numpy.array([host.value, dev.value]), ce, w

    def vi_new():
        v = ctypes.c_void_p()
        check(lib.mnt_vectorinterp_new(ctypes.byref(v)))
        check(lib.mnt_vectorinterp_setGrid(ctypes.byref(v), grid))
        check(lib.mnt_vectorinterp_buildLocator(ctypes.byref(v), 16, 360., 0))
        return v

    def vi_find(v, targets):
        nf = ctypes.c_size_t()
        check(lib.mnt_vectorinterp_findPoints(ctypes.byref(v), targets.shape[0], targets.ctypes.data_as(dp), 1.e-10,
                                              ctypes.byref(nf)))

    def vi_vectors(v, n):
        out = numpy.zeros((n, 3))
        rc = lib.mnt_vectorinterp_getFaceVectors(ctypes.byref(v), data.ctypes.data_as(dp), 0, out.ctypes.data_as(dp))
        return rc, out

    short, long_ = TRANSECTS[1], TRANSECTS[3] + [(170., 60.)]
    few = numpy.column_stack([rng.uniform(-170., 170., 5), rng.uniform(-70., 70., 5), numpy.zeros(5)])
    many = numpy.column_stack([rng.uniform(-170., 170., 300), rng.uniform(-70., 70., 300), numpy.zeros(300)])

    used, new = pli_new(), pli_new()
    pli_weights(used, short)
    pli_results(used)
    pli_weights(used, long_)
    pli_weights(new, long_)
    for g, w in zip(pli_results(used), pli_results(new)):
        assert same_bits(g, w)

    vused, vnew = vi_new(), vi_new()
    vi_find(vused, few)
    assert vi_vectors(vused, 5)[0] == 0
    vi_find(vused, many)
    vi_find(vnew, many)
    rc_u, got = vi_vectors(vused, 300)
    rc_n, want = vi_vectors(vnew, 300)
    assert rc_u == rc_n == 0 and same_bits(got, want)

    # a rebuilt grid (more cells): what the objects computed on the old one is refused
    pts2 = grid_points(24, 40)
    check(lib.mnt_grid_setPointsPtr(ctypes.byref(grid), pts2.ctypes.data_as(dp)))
    check(lib.mnt_grid_build(ctypes.byref(grid), 4, pts2.shape[0]))
    r = ctypes.c_double()
    assert lib.mnt_polylineintegral_getIntegral(ctypes.byref(used), data.ctypes.data_as(dp), 0, ctypes.byref(r)) == NF_ERR_STATE
    assert vi_vectors(vused, 300)[0] == NF_ERR_STATE
    for p in (used, new):
        lib.mnt_polylineintegral_del(ctypes.byref(p))
    for v in (vused, vnew):
        lib.mnt_vectorinterp_del(ctypes.byref(v))
    lib.mnt_grid_del(ctypes.byref(grid))
