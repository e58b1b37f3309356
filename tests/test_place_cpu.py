"""CPU suite: the placement dispatch of the device ingest (nf_inflater_place_form: the function nf_inflater_run itself asks)
is reached in every form by the geometry table of tests/place_reference.py -- so that tests/test_gpu_place.py runs every
placement launch, and a later change of the dispatch cannot drop one from the suite unnoticed -- and the numpy placement
reference is pinned against hdf5min's own host reader on the same in-memory datasets."""
import ctypes
import os
import re
import zlib

import numpy

from conftest import ROOT, deflated_dataset
from place_reference import FORMS, geometries, place_form, place_reference


def test_form_names_are_the_headers():
    txt = open(os.path.join(ROOT, 'include', 'nemoflux_amd.h')).read()
    enum = dict((k, int(v)) for k, v in re.findall(r'\b(NF_PLACE_[A-Z0-9_]+) = (\d+)', txt))
    assert enum.pop('NF_PLACE_FORMS') == len(FORMS) == len(enum)
    assert [enum[name] for name in FORMS] == list(range(len(FORMS)))


def test_dispatch_on_known_geometries():
    """by hand, from the kernels' own conditions (nf_inflate.hip)"""
    assert place_form(1, 0, (2, 3, 8), (3, 5, 18)) == 'NF_PLACE_BYTES'
    assert place_form(4, 1, (1, 1021, 1440), (75, 1021, 1440)) == 'NF_PLACE_PLANES16_F4'       # one chunk per level of a NEMO file
    assert place_form(4, 1, (2, 5, 4), (5, 5, 4)) == 'NF_PLACE_PLANES4_F4'                     # plane of 20
    assert place_form(8, 1, (1, 4, 4), (3, 4, 4)) == 'NF_PLACE_PLANES4_F8'                     # no sixteen form for 8 bytes
    assert place_form(4, 1, (2, 7, 12), (5, 18, 37)) == 'NF_PLACE_ROWS4_F4'
    assert place_form(8, 1, (2, 3, 8), (3, 5, 18)) == 'NF_PLACE_ROWS4_F8'
    assert place_form(4, 1, (2, 7, 10), (5, 18, 37)) == 'NF_PLACE_ELEM_F4_SHUFFLED'
    assert place_form(4, 0, (1, 4, 4), (3, 4, 4)) == 'NF_PLACE_ELEM_F4'                        # only shuffled chunks take 4 per lane
    assert place_form(8, 1, (2, 2, 3), (3, 2, 3)) == 'NF_PLACE_ELEM_F8_SHUFFLED'
    assert place_form(8, 0, (2, 7, 12), (5, 18, 37)) == 'NF_PLACE_ELEM_F8'
    from nemoflux_amd._lib import lib
    d = (ctypes.c_longlong * 3)(1, 1, 4)
    zero = (ctypes.c_longlong * 3)(1, 0, 4)
    f = ctypes.c_int()
    assert lib.nf_inflater_place_form(4, 0, d, d, None) == 1 and lib.nf_inflater_place_form(4, 0, None, d, ctypes.byref(f)) == 1
    assert lib.nf_inflater_place_form(2, 0, d, d, ctypes.byref(f)) == 1 and b'element size' in lib.nf_last_error()
    assert lib.nf_inflater_place_form(1, 1, d, d, ctypes.byref(f)) == 1 and lib.nf_inflater_place_form(4, 0, zero, d, ctypes.byref(f)) == 1


def test_geometry_table_reaches_every_placement_form():
    by_form = {}
    for dtype, shuffled, slab, chunk in geometries():
        by_form.setdefault(place_form(numpy.dtype(dtype).itemsize, shuffled, chunk, slab), []).append((dtype, shuffled, slab, chunk))
    assert set(by_form) == set(FORMS), set(FORMS) - set(by_form)
    for es in ('F4', 'F8'):
        rows = by_form['NF_PLACE_ROWS4_' + es]
        # row starts that are not 16-byte aligned and a last quad across nx: nx % 4 = 1, 2, 3 with cx % 4 == 0
        assert {s[2] % 4 for _, _, s, c in rows if c[2] % 4 == 0 and s[2] > c[2]} >= {1, 2, 3}
        assert any(s[0] % c[0] and s[1] % c[1] for _, _, s, c in rows)                     # overhang in z and y at once
    for form, sizes in (('NF_PLACE_PLANES16_F4', {16, 32, 48}), ('NF_PLACE_PLANES4_F4', {4, 20, 36}),
                        ('NF_PLACE_PLANES4_F8', {4, 20, 36, 16, 32, 48})):
        cases = by_form[form]
        assert {s[1] * s[2] for _, _, s, c in cases} >= sizes
        assert {c[0] for _, _, s, c in cases if s[0] % c[0]} >= {2, 3}                     # whole planes, cz > 1, over nz
    for form in ('NF_PLACE_ELEM_F4_SHUFFLED', 'NF_PLACE_ELEM_F8_SHUFFLED'):
        assert {s[1] * s[2] for _, _, s, c in by_form[form] if c[1:] == s[1:]} >= {6, 10}
    # rank 2 and rank 3 variables
    assert any(s[:2] == (1, 1) for _, _, s, _ in geometries()) and any(s[0] == 1 and s[1] > 1 for _, _, s, _ in geometries())


def test_place_reference_is_the_host_readers_answer():
    """hdf5min.LazyVariable.read_step (inflate + un-shuffle + placement on the host, itself pinned to h5py's read-back by
    tests/test_hdf5min.py) on conftest.deflated_dataset's in-memory variables = place_reference on zlib's bytes of the
    same chunks"""
    rng = numpy.random.default_rng(21)
    done = 0
    for dtype, shuffled, slab, chunk in geometries():
        if numpy.dtype(dtype).itemsize == 1:
            continue                                   # raw bytes are no HDF5 variable of the device path
        a = rng.integers(0, 256, (2,) + slab + (numpy.dtype(dtype).itemsize,), dtype=numpy.uint8).view(dtype)[..., 0]
        lv, _ = deflated_dataset(a, 'uo', (1,) + chunk, level=1, shuffle=bool(shuffled), threads=1)
        for t in (1, 0):
            plan = lv.device_plan(t)
            assert plan is not None and plan['chunk_dims'] == chunk and plan['slab_dims'] == slab and plan['shuffled'] == shuffled
            raw = lv.raw_bytes()
            blocks = [zlib.decompress(bytes(raw[addr:addr + size])) for addr, size, _ in plan['chunks']]
            got = place_reference(blocks, plan)
            host = numpy.ascontiguousarray(lv.read_step(t))
            assert numpy.array_equal(got, host.view(numpy.uint8).reshape(got.shape)), (dtype, shuffled, slab, chunk, t)
            assert numpy.array_equal(got, numpy.ascontiguousarray(a[t]).view(numpy.uint8).reshape(got.shape))
            done += 1
    assert done == 2 * (len(geometries()) - 3)
