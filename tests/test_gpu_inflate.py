"""GPU parity of the file-ingest decoder (nf_inflate.hip: one wavefront per deflated HDF5 chunk, through the C ABI
nf_inflater_run): the device build of nf_inflate_core.h against zlib on the streams of tests/test_inflate_cpu.py, the inverse
of HDF5's shuffle filter, placement of tiled / over-hanging chunks in the slab, and malformed streams (error code per chunk,
nothing written outside the slab)."""
import zlib

import numpy
import pytest

from test_inflate_cpu import payloads

pytestmark = pytest.mark.gpu


@pytest.fixture(scope='module')
def decoder():
    from nemoflux_amd.ingest import ChunkDecoder
    return ChunkDecoder()


@pytest.mark.parametrize('name', [n for n in payloads() if n != 'empty'])     # a chunk holds at least one element
def test_device_inflate_matches_zlib(name, decoder):
    """every block type, level and strategy of zlib, 25 streams per launch (one wavefront each)"""
    data = payloads()[name]
    streams = []
    for level in (0, 1, 4, 6, 9):
        for strategy in (zlib.Z_DEFAULT_STRATEGY, zlib.Z_FIXED, zlib.Z_HUFFMAN_ONLY, zlib.Z_RLE, zlib.Z_FILTERED):
            co = zlib.compressobj(level, zlib.DEFLATED, 15, 8, strategy)
            streams.append(co.compress(data) + co.flush())
    out = decoder.decode_streams(streams, len(data))
    want = numpy.frombuffer(data, numpy.uint8)
    for i in range(len(streams)):
        assert numpy.array_equal(out[i], want), (name, i)


@pytest.mark.parametrize('dtype', ['<f4', '<f8'])
def test_device_unshuffle(dtype, decoder):
    rng = numpy.random.default_rng(1)
    rows = []
    streams = []
    for k in range(40):
        a = (numpy.sin(numpy.arange(50000) * 1e-3 * (k + 1)) * (1 + 1e-3 * rng.standard_normal(50000))).astype(dtype)
        rows.append(a)
        es = a.dtype.itemsize
        streams.append(zlib.compress(numpy.ascontiguousarray(a.view(numpy.uint8).reshape(-1, es).T).tobytes(), 4))
    out = decoder.decode_streams(streams, rows[0].nbytes, elem_size=rows[0].dtype.itemsize, shuffled=1)
    for k, a in enumerate(rows):
        assert numpy.array_equal(out[k].view(dtype), a)


def test_device_tiled_and_overhanging_chunks(decoder):
    """chunks that tile y and x, with edge chunks hanging over the slab (HDF5 stores them whole), through
    hdf5min.Dataset.device_plan and ChunkDecoder.gather / decode"""
    from nemoflux_amd import hdf5min
    from nemoflux_amd._lib import DeviceBuffer
    rng = numpy.random.default_rng(2)
    nt, nz, ny, nx = 2, 5, 18, 37
    cz, cy, cx = 2, 7, 10
    a = rng.standard_normal((nt, nz, ny, nx)).astype('<f4')
    blobs, chunks, off = [], [], 0
    for t in range(nt):
        for z0 in range(0, nz, cz):
            for y0 in range(0, ny, cy):
                for x0 in range(0, nx, cx):
                    blk = rng.standard_normal((cz, cy, cx)).astype('<f4')            # what lies beyond the edge is arbitrary
                    sub = a[t, z0:z0 + cz, y0:y0 + cy, x0:x0 + cx]
                    blk[:sub.shape[0], :sub.shape[1], :sub.shape[2]] = sub
                    b = zlib.compress(numpy.ascontiguousarray(blk.view(numpy.uint8).reshape(-1, 4).T).tobytes(), 4)
                    blobs.append(b)
                    chunks.append(((t, z0, y0, x0, 0), len(b), 0, off))
                    off += len(b)

    class MemFile(object):
        def __init__(self, blob):
            self._m, self._base = blob, 0
    ds = hdf5min.Dataset(MemFile(b''.join(blobs)), 'uo', a.shape, numpy.dtype('<f4'), ('chunked', None, (1, cz, cy, cx, 4), None),
                         [(2, [4]), (1, [4])], {})
    ds._chunks = chunks
    lv = hdf5min.LazyVariable(ds)
    assert numpy.array_equal(lv.read_step(1), a[1])                     # the host reader agrees with the construction
    plan = lv.device_plan(1)
    assert plan is not None and plan['chunk_dims'] == (cz, cy, cx) and plan['slab_dims'] == (nz, ny, nx) and len(plan['chunks']) == 36
    pinned = decoder.new_pinned(decoder.staging_bytes(lv, nt) + 64)
    slab = DeviceBuffer(a[1].nbytes)
    for t in (1, 0):
        staged = decoder.gather(lv.raw_bytes(), lv.device_plan(t), pinned)
        decoder.decode(staged, slab.ptr)
        assert numpy.array_equal(slab.download(a[t].shape, '<f4'), a[t])
    # a dataset the device cannot take goes back to the host path: unfiltered chunk (filter mask), missing chunk
    ds._chunks = [(c[0], c[1], 1, c[3]) if i == 3 else c for i, c in enumerate(chunks)]
    assert lv.device_plan(0) is None and lv.device_plan(1) is not None
    ds._chunks = chunks[1:]
    assert lv.device_plan(0) is None


def test_device_inflate_single_tiny_stream(decoder):
    """one stream of a few bytes: the compressed buffer is smaller than its own padding"""
    for data in (b'a', b'abcd', b'\x00\x00\x80\x3f'):
        for level in (0, 6):
            out = decoder.decode_streams([zlib.compress(data, level)], len(data))
            assert bytes(out[0]) == data


def test_device_inflate_refuses_malformed_streams(decoder):
    from nemoflux_amd._lib import NemofluxError
    rng = numpy.random.default_rng(4)
    data = rng.integers(0, 16, 50000, dtype=numpy.uint8).tobytes()
    good = zlib.compress(data, 6)
    assert numpy.array_equal(decoder.decode_streams([good, good], len(data))[1], numpy.frombuffer(data, numpy.uint8))
    with pytest.raises(NemofluxError, match=r'chunk 1 of 3.*not a zlib stream'):
        decoder.decode_streams([good, b'\x00\x00' + good[2:], good], len(data))
    with pytest.raises(NemofluxError, match='chunk 0 of 1'):
        decoder.decode_streams([good[:len(good) // 2]], len(data))
    with pytest.raises(NemofluxError, match='decoded length differs'):
        decoder.decode_streams([good], len(data) - 8)
    flipped = 0
    streams = []
    for trial in range(64):                     # random bit flips: every one is noticed (structure, length or Adler-32)
        c = bytearray(good)
        for _ in range(int(rng.integers(1, 4))):
            c[int(rng.integers(2, len(c)))] ^= 1 << int(rng.integers(0, 8))
        if bytes(c) != good:
            streams.append(bytes(c))
    for s in streams:
        with pytest.raises(NemofluxError):
            decoder.decode_streams([s], len(data))
        flipped += 1
    assert flipped > 50
    for trial in range(16):                     # noise behind a valid header: an error, and the process survives
        noise = b'\x78\x9c' + rng.integers(0, 256, 3000, dtype=numpy.uint8).tobytes()
        with pytest.raises(NemofluxError):
            decoder.decode_streams([noise], 10000)
    assert numpy.array_equal(decoder.decode_streams([good], len(data))[0], numpy.frombuffer(data, numpy.uint8))


def test_device_inflate_more_streams_than_resident_wavefronts(decoder):
    """3000 different streams in ONE launch -- about three times the 1024 decoder wavefronts the chip holds at once (the
    shipped build keeps DEFLATE's whole 32 KiB window in LDS: 39 KiB per stream, four streams per CU; nf_inflater_capacity) --
    of mixed content (text-like, runs, noise, shuffled floats, long periods), levels and strategies: every one must come
    back exact."""
    assert 256 <= decoder.capacity() < 3000
    rng = numpy.random.default_rng(9)
    n, size = 3000, 40000
    datas, streams = [], []
    for i in range(n):
        kind = i % 4
        if kind == 0:
            d = rng.integers(0, 1 << int(rng.integers(1, 9)), size, dtype=numpy.uint8)
        elif kind == 1:
            d = numpy.repeat(rng.integers(0, 256, size // 50, dtype=numpy.uint8), 50)
        elif kind == 2:
            f = (numpy.cumsum(rng.standard_normal(size // 4)) * 1e-2).astype('<f4')
            d = numpy.ascontiguousarray(f.view(numpy.uint8).reshape(-1, 4).T).reshape(-1)
        else:
            d = numpy.resize(rng.integers(0, 256, int(rng.integers(1, 3000)), dtype=numpy.uint8), size)   # cyclic fill (numpy.tile(...)[:size] would keep size x period bytes alive per stream)
        d = numpy.ascontiguousarray(d[:size])
        co = zlib.compressobj(int(rng.integers(0, 10)), zlib.DEFLATED, 15, 8,
                              [zlib.Z_DEFAULT_STRATEGY, zlib.Z_FILTERED, zlib.Z_RLE, zlib.Z_FIXED][int(rng.integers(0, 4))])
        datas.append(d)
        streams.append(co.compress(d.tobytes()) + co.flush())
    out = decoder.decode_streams(streams, size)
    for i in range(n):
        assert numpy.array_equal(out[i], datas[i]), i


def test_far_path_on_the_device():
    """The shipped decoder keeps DEFLATE's whole 32 KiB window in LDS, so its FAR path (a match source that has already been
    flushed to HBM) never runs on a GPU -- it would with a smaller window.  To keep that path trustworthy (round-3 advisor)
    the library is built here with -DNFI_WINDOW=8192 (`make window8k`: one object, seconds; test-only, never loaded by the
    package) and decodes capacity + 200 streams, a third of them made of matches 9 000 .. 30 000 bytes back, against zlib;
    then the catalogue of tests/deflate_writer.py."""
    import os
    import subprocess
    import sys
    from conftest import ROOT
    subprocess.check_call(['make', '-C', os.path.join(ROOT, 'nemoflux_amd', 'csrc'), 'window8k', '-s'])
    lib = os.path.join(ROOT, 'build', 'window8k', 'libnemoflux_amd_w8k.so')
    r = subprocess.run([sys.executable, os.path.join(ROOT, 'tools', 'check_inflate_window.py'), '--catalogue'],
                       env=dict(os.environ, NEMOFLUX_AMD_LIB=lib), capture_output=True, text=True, timeout=900)
    assert r.returncode == 0 and 'bit-identical' in r.stdout and 'libnemoflux_amd_w8k.so' in r.stdout, r.stdout[-1500:] + r.stderr[-3000:]
    # ... and the catalogue of legal foreign streams (tests/deflate_writer.py): its distance and copy cases are far here
    from deflate_writer import foreign_streams
    assert f'foreign catalogue OK: {len(foreign_streams())} streams' in r.stdout, r.stdout[-1500:]
    cap = int(r.stdout.split('capacity ')[1].split(')')[0])
    assert cap > 2000            # ten streams per CU with the 8 KiB window (the shipped build: 1024)


def test_shared_scratch_survives_its_owner():
    """Round-4 advisor: nf_inflater_share_scratch used to leave the borrower with a dangling pointer when the OWNER was deleted
    first (a C client has no Python wrapper keeping it alive).  Now the owner detaches its borrowers, which go back to a scratch
    of their own; lending while borrowing, and borrowing from a borrower, are refused."""
    import ctypes
    from nemoflux_amd._lib import lib, check, NemofluxError
    from nemoflux_amd.ingest import ChunkDecoder
    data = (numpy.arange(40000, dtype=numpy.uint32) * 2654435761 % 251).astype(numpy.uint8).tobytes()
    streams = [zlib.compress(data, lvl) for lvl in (1, 6, 9)]
    want = numpy.frombuffer(data, numpy.uint8)
    owner, a, b = ChunkDecoder(), ChunkDecoder(), ChunkDecoder()
    owner.decode_streams(streams, len(data))                     # the owner has a scratch of its own
    a.share_scratch_of(owner)
    b.share_scratch_of(owner)
    assert all(numpy.array_equal(r, want) for r in a.decode_streams(streams, len(data)))
    with pytest.raises(NemofluxError, match='borrows its scratch itself'):
        owner_of_a = ChunkDecoder()
        owner_of_a.share_scratch_of(a)
    with pytest.raises(NemofluxError, match='lends its scratch'):
        owner.share_scratch_of(ChunkDecoder())
    # delete the owner through the C ABI while the borrowers are alive (what a C client might do)
    a._scratch_owner = b._scratch_owner = None
    check(lib.nf_inflater_del(ctypes.byref(owner._h)))
    owner._h = None
    for d in (a, b, a):
        assert all(numpy.array_equal(r, want) for r in d.decode_streams(streams, len(data)))
    # a borrower deleted before its owner leaves the owner usable, and deleting the owner afterwards is clean
    o2, c = ChunkDecoder(), ChunkDecoder()
    c.share_scratch_of(o2)
    c.decode_streams(streams, len(data))
    del c
    assert all(numpy.array_equal(r, want) for r in o2.decode_streams(streams, len(data)))
    del o2
