"""The entry path of the fourteen per-step products of a Field, both forms: the synchronous call (no `out`) and the `_async`
one (an `out` tensor in HBM) return the same bits; the tensor holds the raw rows and none of the NaN it was given; a step that
the rank does not own gives exact +0.0 from both; a time index past the end raises the same message from both and leaves the
tensor alone; a Field without transects gives the empty shapes; the five products that take no cell thickness say so under
the name of the symbol called, the other nine run with one.

The entry path does not depend on the grid: nt = 2, nz = 3, ny = 4, nx = 6 is the smallest shape with owned-level subsets on
both sides (slab range (1, 5): step 0 owns levels [1, 3), step 1 owns [0, 2)) and a step a rank does not touch ((4, 6): step 0).
Two transects: one of two segments, one of one."""
import numpy
import pytest

from gpu_helpers import _field, _rows, _same_bits

pytestmark = pytest.mark.gpu

NT, NZ, NY, NX = 2, 3, 4, 6
LINES = [numpy.array([(3., 4., 0.), (33., 27., 0.), (52., 33., 0.)]), numpy.array([(8., 33., 0.), (47., 6., 0.)])]
CLASS_EDGES = [0.8, 1.5, 2.3]
DEPTH_EDGES = [5., 25., 70.]
JOINT_EDGES = ([1.0, 2.0], [26.0, 27.5])
SLABS = [None, (1, 5), (4, 6)]
NO_THICKNESS = ': this form does not take per-cell thicknesses yet and a cell thickness is set; ' \
               'nf_field_set_cell_thickness(NULL) clears it'


def _pairs(f, r, n):
    """a (totals, segments) pair whose axes in front hold n rows, as (n, row_length) raw rows"""
    return _rows(r).reshape(n, f._row_width)


# name, the method, takes carry, the C symbol, the shape of `out`, the raw rows of `out` from what the method returns,
# refuses a cell thickness
PRODUCTS = [
    ('profile', 'computeFluxProfile', False, 'nf_field_compute_profile', lambda f, c: (NZ, f._row_width),
     lambda f, r: _pairs(f, r, NZ), False),
    ('tracer_profile', 'computeTracerProfile', False, 'nf_field_compute_tracer_profile', lambda f, c: (NZ, f._row_width),
     lambda f, r: _pairs(f, r, NZ), True),
    ('area_profile', 'computeAreaProfile', False, 'nf_field_compute_area_profile', lambda f, c: (2, NZ, f._row_width),
     lambda f, r: numpy.stack([_rows(r[0]), _rows(r[1])]), False),
    ('gross_profile', 'computeGrossProfile', True, 'nf_field_compute_gross_profile', lambda f, c: (2 * NZ, f._row_width),
     lambda f, r: _pairs(f, r, 2 * NZ), False),
    ('crossings', 'computeCrossings', True, 'nf_field_compute_crossings', lambda f, c: (4 if c else 2, NZ, len(f.getCrossings())),
     lambda f, r: r, False),
    ('class_transport', 'computeClassTransport', False, 'nf_field_compute_class_transport', lambda f, c: (5, f._row_width),
     lambda f, r: _pairs(f, r, 5), True),
    ('class_tracer_transport', 'computeClassTracerTransport', False, 'nf_field_compute_class_tracer_transport',
     lambda f, c: (5, f._row_width), lambda f, r: _pairs(f, r, 5), True),
    ('class_remap', 'computeClassRemap', True, 'nf_field_compute_class_remap', lambda f, c: (5, f._row_width),
     lambda f, r: _pairs(f, r, 5), True),
    ('depth_transport', 'computeDepthTransport', True, 'nf_field_compute_depth_transport', lambda f, c: (5, f._row_width),
     lambda f, r: _pairs(f, r, 5), False),
    ('surface_transport', 'computeSurfaceTransport', True, 'nf_field_compute_surface_transport', lambda f, c: (4, f._row_width),
     lambda f, r: _pairs(f, r, 4), False),
    ('joint_class_transport', 'computeJointClassTransport', True, 'nf_field_compute_joint_class_transport',
     lambda f, c: (16, f._row_width), lambda f, r: _pairs(f, r, 16), True),
    ('gross_class_transport', 'computeGrossClassTransport', True, 'nf_field_compute_gross_class_transport',
     lambda f, c: (10, f._row_width), lambda f, r: _pairs(f, r, 10), False),
    ('gross_class_remap', 'computeGrossClassRemap', True, 'nf_field_compute_gross_class_remap', lambda f, c: (10, f._row_width),
     lambda f, r: _pairs(f, r, 10), False),
    ('class_area', 'computeClassArea', False, 'nf_field_compute_class_area', lambda f, c: (10, f._row_width),
     lambda f, r: _pairs(f, r, 10), False),
]
CASES = [(p, carry) for p in PRODUCTS for carry in ((False, True) if p[2] else (None,))]
CASE_IDS = [p[0] + ('' if carry is None else '-carry' if carry else '-volume') for p, carry in CASES]
DTYPES = [numpy.float64, numpy.float32]
_FIELDS = {}


def _inputs(dtype):
    """cell bounds of a regular 10-degree grid, thicknesses, and smooth fields with both signs of the flow"""
    x, y = numpy.arange(NX + 1) * 10., numpy.arange(NY + 1) * 10.
    blon = numpy.zeros((NY, NX, 4))
    blat = numpy.zeros((NY, NX, 4))
    blon[..., 0], blon[..., 1], blon[..., 2], blon[..., 3] = x[None, :-1], x[None, 1:], x[None, 1:], x[None, :-1]
    blat[..., 0], blat[..., 1], blat[..., 2], blat[..., 3] = y[:-1, None], y[:-1, None], y[1:, None], y[1:, None]
    db = numpy.array([[0., 10.], [10., 30.], [30., 80.]])
    t, z, j, i = numpy.meshgrid(numpy.arange(NT), numpy.arange(NZ), numpy.arange(NY), numpy.arange(NX), indexing='ij')
    u = (numpy.sin(0.9 * i + 0.4 * j + 0.7 * z + t) + 0.2).astype(dtype)
    v = (numpy.cos(0.5 * i - 0.8 * j + 0.3 * z - t) - 0.1).astype(dtype)
    tau = (1.5 + numpy.sin(0.3 * i + 0.5 * j) - 0.3 * z + 0.1 * t).astype(dtype)
    sig = (26.0 + 0.6 * z + 0.2 * numpy.cos(0.7 * i - 0.2 * j) + 0.05 * t).astype(dtype)
    surf = [(8. + 2. * numpy.sin(0.8 * i[0, 0] + j[0, 0])).astype(dtype), (40. + 5. * numpy.cos(0.6 * i[0, 0])).astype(dtype)]
    e3 = ((db[:, 1] - db[:, 0])[:, None, None] * (1. - 0.1 * numpy.sin(i[0] + 2. * j[0]) ** 2)).astype(dtype)
    return dict(blon=blon, blat=blat, db=db, u=u, v=v, tau=tau, sig=sig, surf=surf, e3=e3)


def _make(dtype, slab=None, lines=LINES, cell=False):
    a = _inputs(dtype)
    f = _field(a['blon'], a['blat'], a['db'], a['u'], a['v'], lines, slab_range=slab, readback=False)
    f.setTracer(a['tau'], reference=0.25)
    f.setClassTracer(a['sig'])
    f.setClassEdges(CLASS_EDGES)
    f.setDepthEdges(DEPTH_EDGES)
    f.setDepthSurfaces(a['surf'])
    f.setJointClassEdges(*JOINT_EDGES)
    if cell:
        f.setCellThickness(a['e3'], a['e3'])
    return f


def _shared(dtype, slab=None, lines=LINES, cell=False):
    """one Field per setting for the whole module: the products promise to leave one another's state alone"""
    key = (numpy.dtype(dtype).name, slab, len(lines), cell)
    if key not in _FIELDS:
        _FIELDS[key] = _make(dtype, slab, lines, cell)
    return _FIELDS[key]


def _call(f, product, carry, t, out=None):
    kw = {} if carry is None else {'carry': carry}
    return getattr(f, product[1])(t, out=out, **kw)


def _flat(r):
    """the arrays of a result, in order"""
    return [r] if isinstance(r, numpy.ndarray) else [a for part in r for a in _flat(part)]


def _nan_tensor(shape):
    import torch
    return torch.full(shape, float('nan'), dtype=torch.float64, device='cuda')


def _owned(slab, t):
    """the levels [z0, z1) of step t inside the slab range"""
    lo = min(max(t * NZ, slab[0]), (t + 1) * NZ)
    hi = max(min((t + 1) * NZ, slab[1]), lo)
    return lo - t * NZ, hi - t * NZ


def _zero_bits(a):
    return not numpy.ascontiguousarray(a, numpy.float64).view(numpy.uint64).any()


def test_the_table_names_fourteen_products_and_the_slabs_cut_as_said():
    assert len(PRODUCTS) == 14 and len(CASES) == 22
    assert sorted(p[0] for p in PRODUCTS if p[6]) == ['class_remap', 'class_tracer_transport', 'class_transport',
                                                      'joint_class_transport', 'tracer_profile']
    assert _owned((1, 5), 0) == (1, 3) and _owned((1, 5), 1) == (0, 2)
    assert _owned((4, 6), 1) == (1, 3) and _owned((4, 6), 0) == (3, 3)


@pytest.mark.parametrize('slab', SLABS, ids=['whole', 'slab1-5', 'slab4-6'])
@pytest.mark.parametrize('product,carry', CASES, ids=CASE_IDS)
@pytest.mark.parametrize('dtype', DTYPES, ids=['f64', 'f32'])
def test_both_forms(dtype, product, carry, slab):
    f = _shared(dtype, slab)
    assert len(f.plis) == 2 and f._nseg == 3 and f._rowlen == 5
    shape = product[4](f, carry)
    for t in range(NT):
        sync = _call(f, product, carry, t)
        out = _nan_tensor(shape)
        asyn = _call(f, product, carry, t, out=out)
        held = out.cpu().numpy()
        a, b = _flat(sync), _flat(asyn)
        assert len(a) == len(b) and all(_same_bits(x, y) for x, y in zip(a, b)), (product[0], t)
        assert not numpy.isnan(held).any(), (product[0], t)
        assert _same_bits(held, product[5](f, asyn)), (product[0], t)
        if slab == (4, 6) and t == 0:
            assert all(_zero_bits(x) for x in a + b) and _zero_bits(held), product[0]
        if slab is None:
            assert any(numpy.any(x != 0.0) for x in a), product[0]          # the inputs reach every product
    # a time index past the end: the same words from both forms, and nothing written
    out = _nan_tensor(shape)
    with pytest.raises(RuntimeError) as e_sync:
        _call(f, product, carry, NT)
    with pytest.raises(RuntimeError) as e_async:
        _call(f, product, carry, NT, out=out)
    assert str(e_sync.value) == str(e_async.value) and type(e_sync.value) is type(e_async.value)
    assert f'time index {NT} out of range' in str(e_sync.value)
    assert numpy.isnan(out.cpu().numpy()).all()


@pytest.mark.parametrize('dtype', DTYPES, ids=['f64', 'f32'])
def test_a_field_without_transects_gives_the_empty_shapes(dtype):
    full, f = _shared(dtype), _shared(dtype, lines=[])
    assert f._rowlen == 0 and f._row_width == 1 and len(f.getCrossings()) == 0
    for product, carry in CASES:
        want = [x.shape[:-1] + (0,) for x in _flat(_call(full, product, carry, 1))]
        sync = _flat(_call(f, product, carry, 1))
        asyn = _flat(_call(f, product, carry, 1, out=_nan_tensor(product[4](f, carry))))
        assert [x.shape for x in sync] == want and [x.shape for x in asyn] == want, product[0]
        assert all(x.dtype == numpy.float64 for x in sync + asyn), product[0]


@pytest.mark.parametrize('dtype', DTYPES, ids=['f64', 'f32'])
def test_with_a_cell_thickness_five_products_refuse_and_nine_run(dtype):
    from nemoflux_amd._lib import NemofluxError
    f = _shared(dtype, cell=True)
    for product, carry in CASES:
        shape = product[4](f, carry)
        if product[6]:
            for suffix, out in (('', None), ('_async', _nan_tensor(shape))):
                with pytest.raises(NemofluxError) as e:
                    _call(f, product, carry, 1, out=out)
                assert str(e.value) == 'nemoflux_amd error 2: ' + product[3] + suffix + NO_THICKNESS
                assert out is None or numpy.isnan(out.cpu().numpy()).all()
            continue
        out = _nan_tensor(shape)
        sync, asyn = _call(f, product, carry, 1), _call(f, product, carry, 1, out=out)
        a, b = _flat(sync), _flat(asyn)
        assert len(a) == len(b) and all(_same_bits(x, y) for x, y in zip(a, b)), product[0]
        assert _same_bits(out.cpu().numpy(), product[5](f, asyn)), product[0]
        assert any(numpy.any(x != 0.0) for x in a), product[0]
