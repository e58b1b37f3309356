"""One nf_field handle of the C ABI driven through ALL of its setters in any order -- tracer, class tracer, class edges, cell
thickness in its four homes, markers, Sverdrup switch, streams -- with the ten compute kinds interleaved: every result equals,
bit for bit, that of a fresh handle given the final state alone, or the call is refused with the code the header documents
(tests/reuse_model.py holds the model; tests/test_reuse_model_cpu.py holds what the random sequences must reach).  The calls
that promise to leave the resident planes alone are held to it, refused calls included; a pass is run twice into the same
rows, refilled with NaN in between (where the pass is captured -- a non-null stream, resident uo / vo and thickness, not the
all-steps-in-one-launch form of small grids: few of the random passes -- the second time is a replay, and so is a later
pass with only tracer and class calls since); and at the end of every sequence the re-used handle is anchored to the long-double
references of the products (tests/resolved_reference.py, cellthick_reference.py, section_reference.py) at their bar of
1e-12 x sum |terms|, for float64 and float32 fields alike (the references start from the values as stored).

Directed: a static host cell thickness that the handle uploaded is refused (NF_ERR_STATE) after set_bounds or set_thickness
changed the shape, also when the byte count stays the same; the scratch arrays follow the weights and the dtype; the class rows
follow the latest class edges; NULL forgets the markers; a captured pass is replayed, rightly, after tracer and class calls.

Grids 6 x 12 to 24 x 40, 1..7 levels, 1..3 steps, up to 6 class edges, 16 sequences of 28 ops.

Found by the sequences: seed 14 -- stream 1, two resident steps, a time-varying cell thickness in HBM, a slab range that owns
step 0 alone -- replayed a captured pass of nf_field_compute_all_async after a flux call and a class tracer setter, and the
row of step 1, which the handle does not own, held other bytes than zeros (a fresh handle: zeros).  Nothing in the library
writes that row but the memset of the rows that are not owned, which was a node of the captured graph; why the replayed node
left other bytes is not established.  The memsets are issued on the stream before every launch of the graph now, and the
sequence is kept by hand in test_replayed_pass_zeroes_the_rows_of_the_steps_it_does_not_own.  No other sequence found a
difference between the re-used and the fresh handle.

Measured on an MI355X: worst |err| / sum |terms| against the references 3.7e-16 (bar 1e-12) over the 16 sequences; the
26 tests of this file take about 4 s together, most of it the first one (library load and first launches)."""
import ctypes

import numpy
import pytest

import reuse_model
from reuse_model import NF_ERR_STATE, Model, run_sequence
from test_gpu_reuse import TRANSECTS, Handle, same_bits
from section_reference import SectionReference, array_values

pytestmark = pytest.mark.gpu

NF_F64, NF_F32 = 0, 1
BAR = 1e-12
WORST = {'ratio': 0.0}
_STREAMS = []
dp = ctypes.POINTER(ctypes.c_double)


def stream_pointer(index):
    """0: the null stream; 1, 2: two streams of the process, made at first use"""
    import torch
    if not _STREAMS:
        _STREAMS.extend([torch.cuda.Stream(), torch.cuda.Stream()])
    return None if index == 0 else _STREAMS[index - 1].cuda_stream


class ProductHandle(Handle):
    """An nf_field handle with every setter; keeps all it was ever lent until it is gone."""

    def __init__(self):
        super().__init__()
        self.lent, self.out = [], {}

    def raw(self, name, *args):
        return getattr(self.lib, 'nf_field_' + name)(ctypes.byref(self.h), *args)

    def lend(self, a, on_device):
        """the address of `a` for the library, in HBM or on the host"""
        import torch
        if on_device:
            a = torch.from_numpy(a).cuda()
            torch.cuda.synchronize()
        self.lent.append(a)
        return a.data_ptr() if on_device else a.ctypes.data

    @staticmethod
    def marker(x):
        return float('nan') if x is None else x

    def set_stream(self, index):
        import torch
        torch.cuda.synchronize()
        self.call('set_stream', stream_pointer(index))

    def set_uv(self, u, v, on_device, fill):
        self.lent.append(self.keep.get('uv'))
        super().set_uv(u, v, on_device, fill)

    def set_tracer(self, a, on_device, fill):
        self.call('set_tracer', self.lend(a, on_device), a.shape[0], NF_F32 if a.dtype == numpy.float32 else NF_F64,
                  int(on_device), self.marker(fill))

    def set_class_tracer(self, a, on_device, fill):
        if a is None:
            return self.call('set_class_tracer', None, 0, NF_F64, 0, float('nan'))
        self.call('set_class_tracer', self.lend(a, on_device), a.shape[0], NF_F32 if a.dtype == numpy.float32 else NF_F64,
                  int(on_device), self.marker(fill))

    def set_class_edges(self, edges):
        e = numpy.ascontiguousarray(edges, numpy.float64)
        self.call('set_class_edges', e.ctypes.data_as(dp), e.size)

    def set_cell_thickness(self, e3u, e3v, on_device, fill):
        if e3u is None:
            return self.call('set_cell_thickness', None, None, 0, NF_F64, 0, float('nan'))
        self.call('set_cell_thickness', self.lend(e3u, on_device), self.lend(e3v, on_device), e3u.shape[0],
                  NF_F32 if e3u.dtype == numpy.float32 else NF_F64, int(on_device), self.marker(fill))

    def planes(self, ncell):
        """(iV (ncell, 4), |eU|, |eV|, running max) of nf_field_read_step"""
        iv, eu, ev, m = numpy.full((ncell, 4), numpy.nan), numpy.full(ncell, numpy.nan), numpy.full(ncell, numpy.nan), \
            ctypes.c_double()
        self.call('read_step', iv.ctypes.data_as(dp), eu.ctypes.data_as(dp), ev.ctypes.data_as(dp), ctypes.byref(m))
        return iv, eu, ev, numpy.array(m.value)

    def rows_in_hbm(self, shape):
        """a NaN-filled float64 tensor of this shape, the same one (same address) for the same shape: a later pass into it
        may replay the captured one"""
        import torch
        if shape not in self.out:
            self.out[shape] = torch.empty(shape, dtype=torch.float64, device='cuda')
        self.out[shape].fill_(float('nan'))
        torch.cuda.synchronize()
        return self.out[shape]

    def product(self, plan, model):
        """(return code, message, arrays) of the compute call of `plan`.  The calls that must leave the resident planes alone
        are checked for it here, refused or not."""
        import torch
        kind, form, t = plan['kind'], plan['form'], plan['t']
        nz, nt, ncell = model.thick.size, model.steps(), model.grid[0] * model.grid[1]
        rowlen = max(self.rowlen(), 1)
        nclass = (model.edges.size if model.edges is not None else 0) + 2
        if kind == 'read':
            return 0, b'', self.planes(ncell)
        if kind in ('flux', 'all'):
            self.call('reset_max')
            before = self.planes(ncell)

        def untouched():                   # a refused call launches nothing
            for b, a in zip(before, self.planes(ncell)):
                assert same_bits(b, a), ('the resident planes changed in a refused call', kind)

        if kind == 'flux':
            rows = numpy.full(rowlen, numpy.nan)
            rc = self.raw('compute_flux', t, rows.ctypes.data_as(dp))
            msg = self.lib.nf_last_error()
            if rc != 0:
                untouched()
            return rc, msg, ((rows,) + self.planes(ncell) if rc == 0 else ())
        if kind == 'all':                  # twice into the same rows: the second pass replays a graph where there is one
            out = self.rows_in_hbm((nt, rowlen))
            rc = self.raw('compute_all_async', out.data_ptr())
            if rc != 0:
                msg = self.lib.nf_last_error()
                torch.cuda.synchronize()
                untouched()
                return rc, msg, ()
            torch.cuda.synchronize()
            first = out.cpu().numpy()
            assert self.rows_in_hbm((nt, rowlen)) is out       # NaN again: the second pass must write every row itself
            self.check(self.raw('compute_all_async', out.data_ptr()))
            torch.cuda.synchronize()
            return rc, b'', (first, out.cpu().numpy()) + self.planes(ncell)
        shape = {'profile': (nz, rowlen), 'tracer_flux': (rowlen,), 'tracer_all': (nt, rowlen), 'class_transport': (nclass, rowlen),
                 'tracer_profile': (nz, rowlen), 'area_profile': (2, nz, rowlen), 'class_tracer_transport': (nclass, rowlen)}[kind]
        before = self.planes(ncell)
        name = 'compute_' + kind
        if form == 'sync':
            rows = numpy.full(shape, numpy.nan)
            rc = self.raw(name, t, rows.ctypes.data_as(dp))
        else:
            out = self.rows_in_hbm(shape)
            rc = self.raw(name + '_async', out.data_ptr()) if kind == 'tracer_all' else self.raw(name + '_async', t, out.data_ptr())
            torch.cuda.synchronize()
            rows = out.cpu().numpy()
        msg = self.lib.nf_last_error()
        for b, a in zip(before, self.planes(ncell)):
            assert same_bits(b, a), ('the resident planes changed', kind, form)
        return rc, msg, ((rows,) if rc == 0 else ())


def compare(h, model, plan):
    """the compute of `plan` on the re-used handle: the rows of a fresh handle bit for bit, or the refusal the model names"""
    import torch
    torch.cuda.synchronize()
    fresh = None
    if not plan['codes'] or plan['on_fresh']:
        fresh = model.fresh(ProductHandle)
    if plan['kind'] == 'read':              # the planes of the same step, computed by each handle
        for x in (h, fresh):
            assert x.product(dict(plan, kind='flux'), model)[0] == 0
    rc, msg, got = h.product(plan, model)
    what = (plan['kind'], plan['form'], plan['t'], plan['causes'])
    if plan['codes']:
        assert rc in plan['codes'] and msg, (what, rc, msg)
        if 'ct_stale' in plan['causes'] and rc == NF_ERR_STATE and len(plan['causes']) == 1:
            assert b'nf_field_set_cell_thickness' in msg and b'NULL' in msg, msg
        if fresh is not None:
            rc_fresh, msg_fresh, _ = fresh.product(plan, model)
            assert rc_fresh == rc and msg_fresh, (what, rc, rc_fresh, msg_fresh)
        return None
    assert rc == 0, (what, rc, msg)
    rc_fresh, msg_fresh, want = fresh.product(plan, model)
    assert rc_fresh == 0, (what, rc_fresh, msg_fresh)
    assert len(got) == len(want) and len(got) > 0
    for k, (g, w) in enumerate(zip(got, want)):
        assert g.shape == w.shape and same_bits(g, w), (what, k)
    if plan['kind'] == 'all':
        assert same_bits(got[0], got[1]), (what, 'the second pass differs from the first')
    return got


# ---- the anchor: the re-used handle against the definitions ------------------------------------------------------------------
def weights_of(h, model):
    n = ctypes.c_size_t()
    h.call('num_weights', ctypes.byref(n))
    ce, w, sg = numpy.empty(n.value, numpy.int64), numpy.empty(n.value), numpy.empty(n.value, numpy.int32)
    h.call('get_weights', ce.ctypes.data_as(ctypes.POINTER(ctypes.c_int64)), w.ctypes.data_as(dp),
           sg.ctypes.data_as(ctypes.POINTER(ctypes.c_int)))
    tr_off = numpy.zeros(len(model.transects) + 1, numpy.int32)
    h.call('segment_offsets', tr_off.ctypes.data_as(ctypes.POINTER(ctypes.c_int)))
    arc = numpy.zeros((model.grid[0] * model.grid[1], 4))
    h.call('get_arclengths', arc.ctypes.data_as(dp))
    return ce, w, sg, arc, tr_off


def close(got, pair, label):
    want, mag = pair
    assert got.shape == want.shape, label
    err = numpy.abs(got - want)
    ratio = float((err / numpy.maximum(mag, 1e-300)).max()) if err.size else 0.0
    WORST['ratio'] = max(WORST['ratio'], ratio)
    assert numpy.all(err <= BAR * mag), (label, ratio)


def anchor(h, model):
    """every product the final state allows, on the re-used handle, against the long-double references; the levels outside
    the slab range carry no thickness there, as they contribute nothing here"""
    model.ready(h, 'area_profile', lazy=False)
    with_ct = model.ct is not None
    if not with_ct:
        model.ready(h, 'class_tracer_transport', lazy=False)
    ny, nx = model.grid[:2]
    t = int(model.rng.choice(model.owned_steps()))
    own = model.owned_levels(t)
    nan = float('nan')
    tau = model.tracer[0]
    arrays = {'uo': model.uv[0], 'vo': model.uv[1], 'tracer': tau, 'class': tau if model.sig is None else model.sig[0]}
    markers = dict(uv_markers=(model.uv[3] or nan, model.missing or nan), tracer_markers=(model.tracer[2] or nan, model.tracer_missing or nan))
    markers['class_markers'] = markers['tracer_markers'] if model.sig is None else (model.sig[2] or nan, model.sig_missing or nan)
    if with_ct:
        mask = own[None, :, None, None]
        arrays['e3u'], arrays['e3v'] = numpy.where(mask, model.ct[0], 0), numpy.where(mask, model.ct[1], 0)
        markers['thick_markers'] = (model.ct[3] or nan, model.ct_missing or nan)
    ce, w, sg, arc, tr_off = weights_of(h, model)
    ref = SectionReference(ce, w, sg, arc, numpy.where(own, model.thick, 0.), tr_off, nx, ny,
                           cell_thickness=with_ct, reference=model.tracer_ref, wrap=bool(model.tracer_wrap),
                           sverdrup=bool(model.sverdrup), **markers)
    values = array_values(arrays, t)
    want = ref.step(values, edge_sets=() if with_ct else [model.edges])
    want.update(ref.area_step(values))

    def rows(kind, form='sync'):
        rc, msg, got = h.product(dict(kind=kind, form=form, t=t), model)
        assert rc == 0, (kind, rc, msg)
        return got

    assert want['volume'][1].max() > 0, 'the final state must carry flux'
    close(rows('flux')[0], want['volume'], 'volume')
    close(rows('all')[0][t], want['volume'], 'volume of the pass')
    close(rows('profile')[0], want['volume_profile'], 'profile')
    close(rows('tracer_flux')[0], want['tracer'], 'tracer')
    close(rows('tracer_all', 'async')[0][t], want['tracer'], 'tracer of the pass')
    area = rows('area_profile', 'async')[0]
    close(area[0], want['area_profile'], 'area')
    close(area[1], want['tracer_area_profile'], 'area-weighted tracer')
    if not with_ct:
        close(rows('tracer_profile')[0], want['tracer_profile'], 'tracer profile')
        close(rows('class_transport', 'async')[0], want['volume_classes', 0], 'volume classes')
        close(rows('class_tracer_transport')[0], want['tracer_classes', 0], 'tracer classes')
    print(f'worst |err| / sum |terms| against the references so far: {WORST["ratio"]:.3g}')


@pytest.mark.parametrize('seed', reuse_model.SEEDS)
def test_handle_reuse_equals_fresh_handle_all_products(seed):
    model, h = Model(numpy.random.default_rng(seed)), ProductHandle()
    run_sequence(model, h, reuse_model.NOPS, lambda plan: compare(h, model, plan))
    anchor(h, model)


# ---- directed: the state is set by hand, compare() and the model's prediction stay the judges ---------------------------------
class Directed:
    """a model and a handle whose state a test writes itself"""

    def __init__(self, seed):
        self.rng = numpy.random.default_rng(seed)
        self.m, self.h = Model(self.rng), ProductHandle()

    def bounds(self, ny, nx, dtype=numpy.float64, on_device=False):
        self.m.grid, self.m.weights_built = (ny, nx, dtype, on_device), False
        self.h.set_bounds(*self.m.grid)

    def thickness(self, nz):
        self.m.thick = self.rng.uniform(1., 50., nz)
        self.h.set_thickness(self.m.thick)

    def fields(self, nt, dtype, on_device=False, tracer=True, sig=False):
        """uo / vo of the shape in force, and with them the tracer (and the class tracer) again"""
        m, shape = self.m, (nt,) + self.m.shape3()
        m.uv = (reuse_model.land_array(self.rng, shape, dtype, 1.e20), reuse_model.land_array(self.rng, shape, dtype, 1.e20),
                on_device, 1.e20)
        self.h.set_uv(*m.uv)
        if tracer:
            m.tracer = (reuse_model.land_array(self.rng, shape, dtype, None, 0., 10.), on_device, None)
            self.h.set_tracer(*m.tracer)
        if sig:
            m.sig = (reuse_model.land_array(self.rng, shape, dtype, None, 0., 10.), on_device, None)
            self.h.set_class_tracer(*m.sig)

    def static_host_thickness(self, arrays=None):
        m = self.m
        shape = (1,) + m.shape3()
        if arrays is None:
            arrays = [reuse_model.land_array(self.rng, shape, m.uv[0].dtype.type, None, 0.5, 40., zeros=True) for _ in range(2)]
        m.ct = (arrays[0], arrays[1], False, None, True)
        self.h.set_cell_thickness(arrays[0], arrays[1], False, None)

    def stream(self, index):
        self.m.stream = index
        self.h.set_stream(index)

    def static_hbm_thickness(self):
        m = self.m
        e3u, e3v = (reuse_model.land_array(self.rng, (1,) + m.shape3(), m.uv[0].dtype.type, None, 0.5, 40., zeros=True) for _ in range(2))
        m.ct = (e3u, e3v, True, None, True)
        self.h.set_cell_thickness(e3u, e3v, True, None)

    def clear_thickness(self):
        self.m.ct, self.m.ct_missing = None, None
        self.h.set_cell_thickness(None, None, False, None)

    def clear_class_tracer(self):
        self.m.sig, self.m.sig_missing = None, None
        self.h.set_class_tracer(None, False, None)

    def transect(self, points):
        self.m.transects.append(points)
        self.m.weights_built = False
        self.h.add_transect(points)

    def edges(self, e):
        self.m.edges = numpy.array(e, numpy.float64)
        self.h.set_class_edges(self.m.edges)

    def build(self):
        self.m.build_weights(self.h)

    def check(self, kinds, causes=()):
        """every kind, in each form it has: what the model predicts (which must be `causes`) holds on the handle"""
        out = {}
        for kind in kinds:
            for form in (('sync', 'async') if kind in reuse_model.BOTH_FORMS else ('async' if kind in ('all', 'tracer_all') else 'sync',)):
                plan = self.m.plan(kind, form)
                assert plan['causes'] == tuple(causes), (kind, plan['causes'])
                out[kind] = compare(self.h, self.m, plan)
        return out


READ_THE_THICKNESS = ['flux', 'all', 'profile', 'tracer_flux', 'area_profile']


@pytest.mark.parametrize('change', ['bounds', 'thickness'])
def test_owned_static_thickness_is_refused_after_a_change_of_shape(change):
    """a static host thickness uploaded at (3 levels, 6 x 12); set_bounds to 24 x 40 or set_thickness to 7 levels: the upload
    is of another shape, and every call that would read it is refused until it is set again or cleared"""
    d = Directed(11)
    d.bounds(6, 12)
    d.thickness(3)
    d.fields(2, numpy.float64)
    d.transect(TRANSECTS[0])
    d.build()
    d.static_host_thickness()
    d.check(READ_THE_THICKNESS)

    def change_shape(ny, nx, nz):
        if change == 'bounds':
            d.bounds(ny, nx)
        else:
            d.thickness(nz)
        d.fields(2, numpy.float64)
        d.build()

    change_shape(24, 40, 7)
    d.check(READ_THE_THICKNESS, causes=('ct_stale',))
    d.check(['tracer_profile'], causes=('ct_set',))          # the forms that take none are refused as before
    d.static_host_thickness()                                  # set again: the rows of a fresh handle
    d.check(READ_THE_THICKNESS)
    d.bounds(*d.m.grid[:2], dtype=numpy.float32)               # the same shape again: the upload stays valid
    d.thickness(d.m.thick.size)
    d.build()
    d.check(READ_THE_THICKNESS)
    change_shape(10, 20, 2)
    d.check(['flux'], causes=('ct_stale',))
    d.clear_thickness()                                        # cleared: the rows of a handle that never had one
    d.check(READ_THE_THICKNESS + ['tracer_profile'])


def test_owned_static_thickness_same_bytes_other_shape():
    """2 levels x 10 x 20 and 4 levels x 10 x 10 are as many bytes: the shapes are compared"""
    d = Directed(12)
    d.bounds(10, 20)
    d.thickness(2)
    d.fields(2, numpy.float32)
    d.transect(TRANSECTS[1])
    d.build()
    d.static_host_thickness()
    d.check(READ_THE_THICKNESS)
    d.bounds(10, 10)
    d.thickness(4)
    assert d.m.ct[0].size == 4 * 10 * 10
    d.fields(2, numpy.float32)
    d.build()
    d.check(READ_THE_THICKNESS, causes=('ct_stale',))


def test_scratch_follows_the_weights_and_the_dtype():
    """the run sums of the profile, tracer profile, area profile and class calls are sized by the records times a chunk that
    depends on the dtype: one short transect first, then a long one as well, then float32 fields"""
    kinds = ['profile', 'tracer_profile', 'area_profile', 'class_transport', 'class_tracer_transport']
    d = Directed(13)
    d.bounds(24, 40)
    d.thickness(7)
    d.fields(2, numpy.float64, on_device=True, sig=True)
    d.edges([2.5, 4., 5., 7.5])
    d.transect(TRANSECTS[2])
    d.build()
    d.check(kinds)
    d.transect(TRANSECTS[3] + [(170., 60.), (-60., 75.), (-175., -70.)])
    d.build()
    d.check(kinds)
    d.fields(3, numpy.float32, on_device=False, sig=True)
    d.check(kinds)
    d.fields(1, numpy.float64, on_device=True, sig=True)
    d.check(kinds)


def test_class_rows_follow_the_latest_edges():
    """6 edges, then 2 and at once 5 with no compute in between, then 2: the rows are those of a fresh handle with the
    latest edges, nedges + 2 of them"""
    kinds = ['class_transport', 'class_tracer_transport']
    d = Directed(14)
    d.bounds(16, 32)
    d.thickness(5)
    d.fields(2, numpy.float64)
    d.transect(TRANSECTS[0])
    d.transect(TRANSECTS[2])
    d.build()
    for sets, nrows in (([[2., 3., 4.5, 5., 6., 7.75]], 8), ([[3., 6.], [2.25, 4., 5., 5.5, 7.]], 7), ([[4., 5.]], 4)):
        for e in sets:
            d.edges(e)
        for kind, got in d.check(kinds).items():
            assert got[0].shape[0] == nrows and numpy.isfinite(got[0]).all(), kind
            assert numpy.abs(got[0][:-1]).max() > 0, kind


def test_clearing_with_null_forgets_the_markers():
    """a second missing value of the cell thickness (of the class tracer), then NULL, then the same arrays again: the marker
    is forgotten, as on a fresh handle that never heard of it -- and the rows differ from those with the marker"""
    d = Directed(15)
    d.bounds(10, 20)
    d.thickness(4)
    d.fields(2, numpy.float64, sig=True)
    d.m.sig[0][..., ::3] = reuse_model.MISSING
    d.edges([3., 5., 6.5])
    d.transect(TRANSECTS[0])
    d.build()
    kinds = ['class_transport', 'class_tracer_transport']
    d.m.sig_missing = reuse_model.MISSING
    d.h.call('set_class_tracer_missing_value', reuse_model.MISSING)
    marked = d.check(kinds)
    sig = d.m.sig
    d.clear_class_tracer()
    d.m.sig = sig
    d.h.set_class_tracer(*sig)
    for kind, got in d.check(kinds).items():
        assert not same_bits(got[0], marked[kind][0]), kind
    d.clear_class_tracer()

    d.static_host_thickness()
    for a in d.m.ct[:2]:
        a[..., ::3] = reuse_model.MISSING
    arrays = d.m.ct[:2]
    d.static_host_thickness(arrays)
    d.m.ct_missing = reuse_model.MISSING
    d.h.call('set_cell_thickness_missing_value', reuse_model.MISSING)
    marked = d.check(READ_THE_THICKNESS)
    d.clear_thickness()
    d.static_host_thickness(arrays)
    for kind, got in d.check(READ_THE_THICKNESS).items():
        assert not same_bits(got[0], marked[kind][0]), kind


@pytest.mark.parametrize('nt, thickness', [(2, True), (1, False), (3, True)], ids=['nt2-e3', 'nt1-plain', 'nt3-e3'])
def test_captured_pass_is_replayed_after_tracer_and_class_calls(nt, thickness):
    """A non-null stream, resident uo / vo and (with two steps or more: the one-launch form is off then) a resident cell
    thickness: nf_field_compute_all_async captures its pass.  Tracer, class tracer and class edge setters and every other
    compute come in between -- none invalidates the pass, all of them use the stream and the run-sum scratch it uses -- and
    the next pass into the same rows, a replay, gives the rows of a fresh handle."""
    d = Directed(16 + nt)
    d.stream(1)
    d.bounds(16, 32)
    d.thickness(5)
    d.fields(nt, numpy.float64, on_device=True)
    d.transect(TRANSECTS[0])
    d.transect(TRANSECTS[3])
    d.build()
    if thickness:
        d.static_hbm_thickness()
    assert d.m.capturable()
    first = d.check(['all'])['all']
    others = ['profile', 'tracer_flux', 'tracer_all', 'area_profile']
    refused = ['tracer_profile', 'class_transport', 'class_tracer_transport']
    for round_ in range(2):
        shape = (nt,) + d.m.shape3()
        d.m.tracer = (reuse_model.land_array(d.rng, shape, numpy.float64, None, 0., 10.), bool(round_), None)
        d.h.set_tracer(*d.m.tracer)
        d.m.sig = (reuse_model.land_array(d.rng, shape, numpy.float64, None, 0., 10.), not round_, None)
        d.h.set_class_tracer(*d.m.sig)
        d.edges([2.5, 4., 6.][:2 + round_])
        d.m.tracer_ref = 3.5 - round_
        d.h.call('set_tracer_reference', d.m.tracer_ref)
        d.check(others)
        if thickness:
            d.check(refused, causes=('ct_set',))
        else:
            d.check(refused)
        again = d.check(['all'])['all']
        for a, b in zip(first, again):                       # the velocities did not change: neither did the rows and planes
            assert same_bits(a, b)
        d.check(['flux'])
        d.check(['all'])


def test_replayed_pass_zeroes_the_rows_of_the_steps_it_does_not_own():
    """Sequence 14 of the random test, by hand: stream 1, two resident steps, a resident time-varying thickness and a slab
    range that owns step 0 alone.  The pass is captured; a flux call, a class tracer in HBM and the fresh handles made for
    comparison come in between; the replay left other bytes than zeros in row 1 while the memsets of the rows that are not
    owned were nodes of the graph.  They are issued before every launch of it now."""
    d = Directed(14)
    d.bounds(16, 32)
    d.thickness(2)
    d.fields(2, numpy.float32, on_device=True)
    d.transect(TRANSECTS[1])
    d.build()
    d.m.slab = (0, 2)
    d.h.call('set_slab_range', 0, 2)
    d.stream(1)
    m, shape = d.m, (2,) + d.m.shape3()
    e3u, e3v = (reuse_model.land_array(d.rng, shape, numpy.float32, None, 0.5, 40., zeros=True) for _ in range(2))
    m.ct = (e3u, e3v, True, None, False)
    d.h.set_cell_thickness(e3u, e3v, True, None)
    assert m.capturable()
    for round_ in range(3):
        got = d.check(['all'])['all']
        assert numpy.all(got[0][1] == 0) and numpy.all(got[1][1] == 0) and numpy.abs(got[0][0]).max() > 0
        d.check(['flux'])
        m.sig = (reuse_model.land_array(d.rng, shape, numpy.float32, None, 0., 10.), True, None)
        d.h.set_class_tracer(*m.sig)
