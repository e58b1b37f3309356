"""GPU: the placement half of the device ingest (nf_inflate.hip) at toy size -- every launch nf_inflater_run can take
(tests/test_place_cpu.py checks that the geometry table reaches them all), the scalar fallback of the four-per-lane form,
whole-plane chunks that hang over nz, more chunks than gridDim.y holds, and the stager's grouping (a short last group,
uo and vo chunked differently) -- against the numpy reference of tests/place_reference.py and the CPU oracle, bit for bit."""
import zlib

import numpy
import pytest

from conftest import deflated_dataset, transect_xyz
from place_reference import geometries, place_form, place_reference, random_plan

pytestmark = pytest.mark.gpu

TAIL = 64


@pytest.fixture(scope='module')
def decoder():
    from nemoflux_amd.ingest import ChunkDecoder
    return ChunkDecoder()


def run_placement(decoder, blocks, plan, keep, rng):
    """deflate the kept chunks, decode + place them into a slab that is pre-filled with a marker pattern and TAIL bytes
    longer than it has to be; returns (what the device left there, what the reference says), both as flat bytes"""
    from nemoflux_amd._lib import DeviceBuffer
    from nemoflux_amd.ingest import StagedChunks
    nz, ny, nx = plan['slab_dims']
    es = plan['elem_size']
    streams = [zlib.compress(blocks[i], int(rng.integers(0, 3))) for i in keep]
    in_off = numpy.zeros(len(keep), numpy.int64)
    pos = 0
    for k, s in enumerate(streams):
        in_off[k] = pos
        pos += (len(s) + 7) & ~7
    pinned = decoder.new_pinned(pos + 16)
    for k, s in enumerate(streams):
        pinned.array[in_off[k]:in_off[k] + len(s)] = numpy.frombuffer(s, numpy.uint8)
    origin = numpy.ascontiguousarray(numpy.array([plan['chunks'][i][2] for i in keep], numpy.int64).reshape(-1, 3))
    staged = StagedChunks(pinned, pos, in_off, numpy.array([len(s) for s in streams], numpy.int64), origin, plan)
    nbytes = nz * ny * nx * es
    marker = ((numpy.arange(nbytes + TAIL, dtype=numpy.uint64) * 37 + 11) % 251).astype(numpy.uint8)
    buf = DeviceBuffer(nbytes + TAIL)
    try:
        buf.upload(marker)
        status = decoder.decode(staged, buf.ptr)
        assert not status.any()
        got = buf.download((nbytes + TAIL,), numpy.uint8)
    finally:
        buf.free()
    want = marker.copy()
    sub = dict(plan, chunks=[plan['chunks'][i] for i in keep])
    place_reference([blocks[i] for i in keep], sub, out=want[:nbytes].reshape(nz, ny, nx, es))
    return got, want


@pytest.mark.parametrize('dtype, shuffled', [('<f4', 1), ('<f4', 0), ('<f8', 1), ('<f8', 0), ('u1', 0)])
def test_every_placement_form_against_numpy(dtype, shuffled, decoder):
    """Every geometry of the table: all chunks, and all but some (what they would have covered must keep the marker, like
    the TAIL bytes behind the slab: a store outside a chunk's box shows up)."""
    rng = numpy.random.default_rng(31 + shuffled + numpy.dtype(dtype).itemsize)
    forms = set()
    for dt, sh, slab, chunk in geometries():
        if (dt, sh) != (dtype, shuffled):
            continue
        forms.add(place_form(numpy.dtype(dt).itemsize, sh, chunk, slab))
        blocks, plan = random_plan(dt, sh, slab, chunk, rng)
        n = len(blocks)
        subsets = [list(range(n))]
        if n > 1:
            subsets.append([i for i in range(n) if rng.random() < 0.6] or [n - 1])
            subsets.append([n - 1])                         # the chunk that hangs over in every direction, alone
        for keep in subsets:
            got, want = run_placement(decoder, blocks, plan, keep, rng)
            bad = numpy.nonzero(got != want)[0]
            assert bad.size == 0, (dt, sh, slab, chunk, keep, bad[:8], got[bad[:8]], want[bad[:8]])
    assert len(forms) == {('<f4', 1): 4, ('<f8', 1): 3}.get((dtype, shuffled), 1)


def test_more_chunks_than_grid_rows(decoder):
    """70 000 chunks of (1, 1, 4) float32 in ONE launch: the placement kernels' gridDim.y is capped at 65 535 and every
    block walks on from there; each chunk has its own content"""
    rng = numpy.random.default_rng(41)
    n = 70000
    vals = rng.integers(0, 1 << 32, (n, 4), dtype=numpy.uint64).astype('<u4')
    planes = numpy.ascontiguousarray(vals.view(numpy.uint8).reshape(n, 4, 4).transpose(0, 2, 1))   # HDF5 shuffle, per chunk
    streams = [zlib.compress(planes[i].tobytes(), 1) for i in range(n)]
    assert place_form(4, 1, (1, 1, 4), (n, 1, 4)) == 'NF_PLACE_PLANES4_F4'
    out = decoder.decode_streams(streams, 16, elem_size=4, shuffled=1)
    got = out.view('<u4')
    bad = numpy.nonzero((got != vals).any(axis=1))[0]
    assert bad.size == 0, bad[:10]


@pytest.mark.parametrize('dtype, shuffled', [('<f4', 1), ('<f4', 0), ('<f8', 1)])
def test_stacked_slabs_keep_their_chunks_apart(dtype, shuffled, decoder):
    """What the stager does with the variables and steps of a group: three slabs stacked along z, decoded by ONE launch
    (ChunkDecoder.gather_many).  A chunk that hangs over nz must stop at the end of ITS slab -- the levels behind it are
    the next slab's (found by this test: the kernels used to cut at the end of the stack only).  Whole-plane chunks
    (sixteen and four per lane), tiled rows, one element per lane; the bytes beyond the edge are random."""
    from nemoflux_amd._lib import DeviceBuffer
    rng = numpy.random.default_rng(51)
    es = numpy.dtype(dtype).itemsize
    for slab, chunk in (((5, 4, 8), (2, 4, 8)), ((4, 5, 4), (3, 5, 4)), ((5, 18, 36), (2, 7, 12)), ((3, 5, 7), (2, 2, 3)),
                        ((5, 2, 3), (3, 2, 3))):
        nz, ny, nx = slab
        nstack = 3
        blob, items, want = bytearray(b'\x00' * 5), [], []
        for k in range(nstack):
            blocks, plan = random_plan(dtype, shuffled, slab, chunk, rng)
            chunks = []
            for blk, (_, _, origin) in zip(blocks, plan['chunks']):
                s = zlib.compress(blk, 1)
                chunks.append((len(blob), len(s), origin))
                blob += s
            plan['chunks'] = chunks
            want.append(place_reference(blocks, plan))
            items.append((plan, k * nz))
        raw = bytes(blob)
        pinned = decoder.new_pinned(len(raw) + 8 * sum(len(p['chunks']) for p, _ in items) + 64)
        staged = decoder.gather_many([(raw, p, zoff) for p, zoff in items], pinned, nstack * nz)
        assert len(staged) == 1 and staged[0].plan['slab_dims'] == (nstack * nz, ny, nx) and staged[0].plan['stack_nz'] == nz
        nbytes = nstack * nz * ny * nx * es
        marker = ((numpy.arange(nbytes + TAIL, dtype=numpy.uint64) * 37 + 11) % 251).astype(numpy.uint8)
        buf = DeviceBuffer(nbytes + TAIL)
        try:
            buf.upload(marker)
            assert not decoder.decode(staged[0], buf.ptr).any()
            got = buf.download((nbytes + TAIL,), numpy.uint8)
        finally:
            buf.free()
        expect = numpy.concatenate([w.reshape(-1) for w in want] + [marker[nbytes:]])
        bad = numpy.nonzero(got != expect)[0]
        assert bad.size == 0, (dtype, shuffled, slab, chunk, bad[:8])


NX, NY, NZ, NT = 36, 18, 5, 5
PSI = "(1+10*z)*(t+1)*(cos(2*pi*y/360) + sin(2*pi*x/360))"


@pytest.fixture(scope='module')
def toy():
    from nemoflux_amd.datagen import DataGen
    dg = DataGen(real='float32')
    dg.setSizes(NX, NY, NZ, NT)
    dg.setBoundingBox(-180., 180., -90., 90., 0., 1.)
    dg.build()
    dg.applyStreamFunction(PSI)
    dg.computeUVFromPotential()
    rng = numpy.random.default_rng(2)
    u, v = dg.u.cpu().numpy(), dg.v.cpu().numpy()
    u *= (1 + numpy.float32(1e-3) * rng.standard_normal(u.shape, dtype=numpy.float32))
    v *= (1 + numpy.float32(1e-3) * rng.standard_normal(v.shape, dtype=numpy.float32))
    v[:, :, -1, :] = 0                              # datagen's pole row is 1e13-sized garbage
    u[:, 3:, 4:9, 10:20] = numpy.float32(1.e20)     # land below level 3: _FillValue
    v[:, 3:, 4:9, 10:20] = numpy.float32(1.e20)
    return dg, u, v


@pytest.fixture(scope='module')
def toy_fields(toy, oracle):
    """the CPU oracle's (ncell, 4) field and transect totals of every step, on the values the files decode to"""
    dg, u, v = toy
    blon, blat = dg.bounds_lon.cpu().numpy(), dg.bounds_lat.cpu().numpy()
    tr = [transect_xyz("(-100,-80),(100,-80),(0,80)"), transect_xyz("(-170,10),(-20,-55),(135,62),(-170,10)")]
    pts = oracle.assemble_points(blon, blat)
    ows = [oracle.polyline_weights(pts, xyz) for xyz in tr]
    return blon, blat, tr, ows


@pytest.mark.parametrize('vchunk', [(1, 1, NY, NX), (1, 2, 7, 12)], ids=['same_chunking', 'vo_tiled'])
@pytest.mark.parametrize('prefetch', [True, False], ids=['prefetch', 'no_prefetch'])
def test_grouping_with_a_short_last_group(toy, toy_fields, prefetch, vchunk, oracle, monkeypatch):
    """File-backed Field, groups of two steps over five (the last group holds one), steps visited out of order and again,
    then invalidate() and computeAll(); with vo chunked differently from uo a group is staged as TWO StagedChunks (two
    launches into one slab).  Every step's full (ncell, 4) field equals the CPU oracle's bit for bit."""
    import contextlib
    import io as _io
    from nemoflux_amd.field import Field
    dg, u, v = toy
    blon, blat, tr, ows = toy_fields
    monkeypatch.setenv('NF_INFLATE_GROUP', '2')
    lu, _ = deflated_dataset(u, 'uo', (1, 1, NY, NX), attrs={'_FillValue': numpy.float32(1.e20)})
    lv, _ = deflated_dataset(v, 'vo', vchunk, attrs={'_FillValue': numpy.float32(1.e20)})
    with contextlib.redirect_stdout(_io.StringIO()):
        ff = Field.fromArrays(blon, blat, dg.deptht_bounds, lu, lv, tr, fill_value=1.e20, prefetch=prefetch)
    st = ff._stager
    assert st.on_device and st.comp_bytes[0] is not None and st.comp_bytes[1] is not None and st.group == 2
    th = dg.zbot - dg.ztop
    fill = float(numpy.float32(1.e20))
    state = oracle.EdgeFluxState(NY, NX)
    want = {}
    nstaged = set()
    for t in (4, 0, 3, 1, 2, 4):
        oracle.edge_flux(state, oracle.vertical_integral(u[t], th, fill), oracle.vertical_integral(v[t], th, fill), ff.arcLengths)
        got = ff.computeFlux(t, readback=True)
        assert numpy.array_equal(ff.integratedVelocity, state.integratedVelocity), t
        want[t] = numpy.array([oracle.get_integral(w, state.integratedVelocity) for w in ows])
        bound = 1e-12 * max(numpy.abs(w.weight * state.integratedVelocity.reshape(-1)[w.cell_edge]).sum() for w in ows)
        assert numpy.abs(numpy.array(got) - want[t]).max() <= bound, t
        slot = [s for s in (0, 1) if st._range[s][0] <= t < st._range[s][1]]
        assert slot and st._range[slot[-1]] == (2 * (t // 2), min(2 * (t // 2) + 2, NT))      # (4, 5): the short group
        nstaged.add(len(st._slots[slot[-1]]['staged']))
    assert nstaged == ({1} if vchunk == (1, 1, NY, NX) else {2})       # gather_many: one StagedChunks per chunk geometry
    st.invalidate()
    ff._lazy_step = -1
    tot, _ = ff.computeAll()
    for t in range(NT):
        assert numpy.abs(tot[t] - want[t]).max() <= 1e-12 * max(1.0, numpy.abs(want[t]).max()) * 10
    ff.computeFlux(4, readback=True)               # the last, short group once more after the whole pass
    oracle.edge_flux(state, oracle.vertical_integral(u[4], th, fill), oracle.vertical_integral(v[4], th, fill), ff.arcLengths)
    assert numpy.array_equal(ff.integratedVelocity, state.integratedVelocity)
