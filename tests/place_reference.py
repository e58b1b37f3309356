"""Reference and geometry table for the placement half of the device ingest (nf_inflate.hip: k_place, k_place4, k_place16):
what a decoded HDF5 chunk is (optionally byte-shuffled, stored whole even where it hangs over the slab) and where its
elements go.  Plain numpy; tests/test_place_cpu.py pins it against hdf5min's own host reader, tests/test_gpu_place.py
compares the device with it bit for bit."""
import ctypes

import numpy

FORMS = ('NF_PLACE_BYTES', 'NF_PLACE_PLANES16_F4', 'NF_PLACE_PLANES4_F4', 'NF_PLACE_PLANES4_F8', 'NF_PLACE_ROWS4_F4',
         'NF_PLACE_ROWS4_F8', 'NF_PLACE_ELEM_F4_SHUFFLED', 'NF_PLACE_ELEM_F4', 'NF_PLACE_ELEM_F8_SHUFFLED', 'NF_PLACE_ELEM_F8')


def place_reference(blocks, plan, out=None):
    """blocks[i]: the decoded bytes of chunk i of plan['chunks'] (as the deflate stream holds them: byte planes when
    shuffled); un-shuffle each, then copy the part of its (cz, cy, cx) box that lies inside the slab to its origin.
    Returns the slab as (nz, ny, nx, elem_size) bytes; `out` (same shape) is written in place when given."""
    cz, cy, cx = plan['chunk_dims']
    nz, ny, nx = plan['slab_dims']
    es = plan['elem_size']
    if out is None:
        out = numpy.zeros((nz, ny, nx, es), numpy.uint8)
    assert out.shape == (nz, ny, nx, es) and len(blocks) == len(plan['chunks'])
    n = cz * cy * cx
    for blk, (_, _, (z0, y0, x0)) in zip(blocks, plan['chunks']):
        raw = numpy.frombuffer(blk, numpy.uint8)
        assert raw.size == n * es == plan['chunk_bytes']
        elems = raw.reshape(es, n).T if plan['shuffled'] else raw.reshape(n, es)
        box = elems.reshape(cz, cy, cx, es)
        dz, dy, dx = min(cz, nz - z0), min(cy, ny - y0), min(cx, nx - x0)
        out[z0:z0 + dz, y0:y0 + dy, x0:x0 + dx] = box[:dz, :dy, :dx]
    return out


def place_form(elem_size, shuffled, chunk_dims, slab_dims):
    """name of the launch nf_inflater_run takes for this geometry, from the library's own dispatch (needs no GPU)"""
    from nemoflux_amd._lib import lib, check
    form = ctypes.c_int(-1)
    check(lib.nf_inflater_place_form(int(elem_size), int(shuffled), (ctypes.c_longlong * 3)(*chunk_dims),
                                     (ctypes.c_longlong * 3)(*slab_dims), ctypes.byref(form)))
    return FORMS[form.value]


# (slab (nz, ny, nx), chunk (cz, cy, cx)); every one is run as <f4 and <f8, shuffled and not
SHAPES = [
    # whole-plane chunks, plane sizes 16 / 32 / 48 (sixteen elements per lane), cz in {1, 2, 3}, nz % cz != 0
    ((3, 4, 4), (1, 4, 4)), ((5, 4, 8), (2, 4, 8)), ((4, 4, 12), (3, 4, 12)), ((5, 2, 8), (3, 2, 8)),
    # ... 4 / 20 / 36 (four per lane)
    ((3, 1, 4), (2, 1, 4)), ((5, 5, 4), (2, 5, 4)), ((4, 3, 12), (3, 3, 12)), ((2, 9, 4), (1, 9, 4)),
    # ... 6 / 10 (neither)
    ((3, 2, 3), (2, 2, 3)), ((4, 2, 5), (3, 2, 5)),
    # rows of a multiple of four elements that do not fill the slab: nx % 4 in {1, 2, 3}, unaligned row starts, a last quad
    # across nx, overhang in y and z at once
    ((5, 18, 37), (2, 7, 12)), ((3, 5, 18), (2, 3, 8)), ((3, 6, 23), (2, 4, 4)), ((2, 3, 39), (1, 2, 20)),
    ((3, 7, 16), (2, 3, 16)), ((2, 6, 24), (1, 4, 8)),
    # rows that are not: one element per lane
    ((5, 18, 37), (2, 7, 10)), ((3, 5, 7), (2, 2, 3)), ((2, 4, 9), (1, 4, 9)),
    # rank-2 and rank-3 variables: slabs (1, 1, nx) and (1, ny, nx)
    ((1, 1, 37), (1, 1, 12)), ((1, 1, 16), (1, 1, 16)), ((1, 1, 20), (1, 1, 20)), ((1, 1, 11), (1, 1, 11)), ((1, 1, 11), (1, 1, 4)),
    ((1, 6, 8), (1, 6, 8)), ((1, 7, 18), (1, 3, 8)), ((1, 5, 6), (1, 2, 6)),
]


def geometries():
    """[(dtype, shuffled, slab, chunk)]: SHAPES as <f4 and <f8, shuffled and not, and raw bytes"""
    out = [(dt, sh, slab, chunk) for slab, chunk in SHAPES for dt in ('<f4', '<f8') for sh in (1, 0)]
    out += [('u1', 0, (3, 5, 18), (2, 3, 8)), ('u1', 0, (1, 1, 37), (1, 1, 12)), ('u1', 0, (3, 4, 4), (1, 4, 4))]
    return out


def chunk_origins(slab, chunk):
    return [(z0, y0, x0) for z0 in range(0, slab[0], chunk[0]) for y0 in range(0, slab[1], chunk[1])
            for x0 in range(0, slab[2], chunk[2])]


def random_plan(dtype, shuffled, slab, chunk, rng):
    """(blocks, plan): every chunk of the slab as random bytes -- also beyond the slab's edge -- and the plan of
    hdf5min.Dataset.device_plan's shape (the byte offsets are left to whoever packs the streams)"""
    es = numpy.dtype(dtype).itemsize
    nbytes = chunk[0] * chunk[1] * chunk[2] * es
    origins = chunk_origins(slab, chunk)
    blocks = [rng.integers(0, 256, nbytes, dtype=numpy.uint8).tobytes() for _ in origins]
    plan = dict(chunks=[(None, None, o) for o in origins], chunk_dims=tuple(chunk), slab_dims=tuple(slab), chunk_bytes=nbytes,
                elem_size=es, shuffled=int(shuffled))
    return blocks, plan
