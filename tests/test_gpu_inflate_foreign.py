"""GPU: the device build of the decoder (its hand-written hot loop included, which no host build compiles) on LEGAL
streams that zlib's own compressor does not write -- the catalogue and the random streams of tests/deflate_writer.py, which
tests/test_inflate_cpu.py pins against zlib and the host build -- and on streams that start at every byte offset.  The
reference is zlib.decompress of the same stream, bit for bit.  Smallest launches first."""
import zlib

import numpy
import pytest

from deflate_writer import foreign_streams, random_streams, stream_of_length
from test_inflate_cpu import payloads

pytestmark = pytest.mark.gpu


@pytest.fixture(scope='module')
def decoder():
    from nemoflux_amd.ingest import ChunkDecoder
    return ChunkDecoder()


def by_length(named):
    """[(decoded length, [(name, stream, zlib's bytes)])], shortest first: one launch per decoded length"""
    groups = {}
    for name, stream in named:
        want = zlib.decompress(stream)
        groups.setdefault(len(want), []).append((name, stream, numpy.frombuffer(want, numpy.uint8)))
    return sorted(groups.items())


def check_launch(decoder, group, size, **kw):
    out = decoder.decode_streams([g[1] for g in group], size, **kw)
    bad = [g[0] for i, g in enumerate(group) if not numpy.array_equal(out[i], g[2])]
    assert not bad, bad


def test_device_decodes_the_foreign_catalogue(decoder):
    cat = foreign_streams()
    launches = by_length((name, s) for name, (s, _) in cat.items())
    assert sum(len(g) for _, g in launches) == len(cat) and len(launches) <= 4
    for size, group in launches:
        check_launch(decoder, group, size)


def test_device_decodes_random_foreign_streams(decoder):
    rnd = random_streams(300, 11)
    (size, group), = by_length((i, s) for i, (s, _) in enumerate(rnd))
    assert len(group) == 300
    check_launch(decoder, group, size)


def test_device_decodes_streams_at_every_byte_offset(decoder):
    """align=1: the streams lie back to back and the last one ends at the last byte of the buffer.  No legal zlib stream is
    shorter than eight bytes, so the offsets are set by seven leading streams whose compressed length is 1 modulo 8: the
    streams of every launch start at offsets 0, 1, ... 7 and on from there."""
    named = [(name, s) for name, (s, _) in foreign_streams().items()]
    for pname in ('short', 'two_bit'):
        data = payloads()[pname]
        for level in (0, 1, 4, 6, 9):
            for strategy in (zlib.Z_DEFAULT_STRATEGY, zlib.Z_FIXED, zlib.Z_HUFFMAN_ONLY, zlib.Z_RLE, zlib.Z_FILTERED):
                co = zlib.compressobj(level, zlib.DEFLATED, 15, 8, strategy)
                named.append(((pname, level, strategy), co.compress(data) + co.flush()))
    assert len(named) == len(foreign_streams()) + 50
    seen = set()
    for size, group in by_length(named):
        lead = []
        for k in range(7):
            s, data = stream_of_length(size, 1, seed=k)
            lead.append((('lead', k), s, numpy.frombuffer(data, numpy.uint8)))
        check_launch(decoder, lead + group, size, align=1)
        off = decoder.last_in_off
        assert list(off[:8]) == list(numpy.cumsum([0] + [len(g[1]) for g in lead]))
        assert numpy.array_equal(off, numpy.cumsum([0] + [len(g[1]) for g in (lead + group)[:-1]]))
        here = {int(o) % 8 for o in off}
        assert here == set(range(8)), (size, here)
        seen |= here
    assert seen == set(range(8))
