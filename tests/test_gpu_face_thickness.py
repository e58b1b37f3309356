"""Face thicknesses derived from e3t on the GPU, the raw ABI: nf_face_thickness against the numpy restatement of
tests/face_thickness_reference.py bit for bit -- every operation of the definition is one correctly rounded IEEE float64
operation in a fixed order -- on the inputs whose branch coverage tests/test_face_thickness_cpu.py asserts: (ny, nx) = (36, 72)
and (37, 73), nz = 1 and 7, one launch of (nz, ny, nx) = (3, 1, 5), both dtypes, the three rules, wrapX on and off, thicknesses
on the lattice of the multiples of 1/8 in [0.25, 4] with exact zeros, both markers and NaN scattered, guard words around both
outputs, every base pointer in turn moved by one element (no 16-byte alignment: one value per lane).  Past one column chunk of
256 lanes (WIDE_SHAPES there: nx = 512 to 2052) in both lane forms: two, three and more chunks, a full last chunk and one of a
single lane, the east neighbour that another chunk holds.  Then the Python call, and a static e3t given as (1, nz, ny, nx)."""
import numpy
import pytest

import face_thickness_reference as ref

pytestmark = pytest.mark.gpu

NF_F64, NF_F32 = 0, 1
GUARD = -7.0
PAD = 16
CASES = ref.raw_cases()
WIDE = ref.wide_cases()
EM, SM = (ref.EFILL, ref.EMISSING), (ref.SFILL, ref.SMISSING)


def _device(a, shift):
    """a host array on the device behind `shift` leading elements: (tensor that owns it, address of a's first element)"""
    import torch
    host = numpy.full(a.size + shift + 4, 3.25, a.dtype)
    host[shift:shift + a.size] = a.reshape(-1)
    t = torch.from_numpy(host).cuda()
    return t, t.data_ptr() + shift * a.dtype.itemsize


def _call(e3t, rule, statics=(None, None, None), wrap=True, shifts=(0,) * 6, markers=True):
    """nf_face_thickness on host inputs: (e3u, e3v), with the guard words around both outputs checked.  shifts: the number of
    elements by which e3u_out, e3v_out, e3t, e3t0, e3u0, e3v0 are moved off their allocation's base"""
    import torch
    from nemoflux_amd._lib import lib
    nz, ny, nx = e3t.shape
    real, n = e3t.dtype, e3t.size
    ins = [(None, None) if a is None else _device(a, s) for a, s in zip((e3t,) + tuple(statics), shifts[2:])]
    tdt = ins[0][0].dtype
    outs = [torch.full((n + 2 * PAD + s,), GUARD, dtype=tdt, device='cuda') for s in shifts[:2]]
    optr = [o.data_ptr() + (PAD + s) * real.itemsize for o, s in zip(outs, shifts[:2])]
    em, sm = (EM, SM) if markers else ((numpy.nan,) * 2,) * 2
    rc = lib.nf_face_thickness(optr[0], optr[1], *[p for _, p in ins], nz, ny, nx, NF_F32 if real == numpy.float32 else NF_F64,
                               rule, 1 if wrap else 0, em[0], em[1], sm[0], sm[1], None)
    assert rc == 0, lib.nf_last_error()
    assert lib.nf_synchronize() == 0
    res = []
    for o, s in zip(outs, shifts[:2]):
        got = o.cpu().numpy()
        assert (got[:PAD + s] == GUARD).all() and (got[PAD + s + n:] == GUARD).all(), 'an output was written outside its array'
        res.append(got[PAD + s:PAD + s + n].reshape(nz, ny, nx))
    for (keep, _), a, s in zip(ins, (e3t,) + tuple(statics), shifts[2:]):        # the inputs are only read
        if keep is not None:
            assert ref.same_bits(keep.cpu().numpy()[s:s + a.size], a.reshape(-1))
    return res


def _report(got, want, label, vec=None):
    """vec: the values a lane holds in this launch; the report then names the chunk and the lane of the first differing column"""
    bad = ~((got == want) | (numpy.isnan(got) & numpy.isnan(want)))
    if bad.any():
        z, y, x = (int(i[0]) for i in numpy.nonzero(bad))
        where = '' if vec is None else ' = chunk %d of %d, lane %d at %d per lane' % (
            ref.chunk_and_lane(x, vec)[0], ref.chunks_of(got.shape[-1], vec), ref.chunk_and_lane(x, vec)[1], vec)
        print(f'{label}: {int(bad.sum())} of {got.size} values differ; first: face ({z}, {y}, {x}){where} got {got[z, y, x]!r} '
              f'want {want[z, y, x]!r}')
    return not bad.any()


@pytest.mark.parametrize('case', CASES, ids=[ref.case_id(c) for c in CASES])
def test_raw_abi_is_the_restatement_bit_for_bit(case):
    """the bases as the allocator gives them, then each of them in turn moved by one element (4 or 8 bytes)"""
    real, nz, ny, nx, rule, wrap = case
    e3t, *statics = ref.case_arrays(case)
    want = ref.face_thickness(e3t, rule, *statics, wrap=wrap, markers=EM, static_markers=SM)
    npointers = 6 if rule == ref.ANOMALY else 3
    for moved in [None] + list(range(npointers)):
        shifts = tuple(1 if k == moved else 0 for k in range(6))
        got = _call(e3t, rule, statics, wrap, shifts)
        for g, w, name in zip(got, want, ('e3u', 'e3v')):
            label = f'{ref.case_id(case)} {name} moved={moved}'
            assert _report(g, w, label), label
            assert ref.same_bits(g, w), label


@pytest.mark.parametrize('case', WIDE, ids=[ref.wide_id(c) for c in WIDE])
def test_raw_abi_past_one_column_chunk(case):
    """rows of two and more chunks of 256 lanes, a full last chunk and one of a single lane (tests/face_thickness_reference.py,
    WIDE_SHAPES): the bases as the allocator gives them -- 16-byte lanes where nx allows -- and e3u_out moved by one element
    -- one value per lane, more chunks; where a last chunk holds one lane, every base in turn"""
    real, nz, ny, nx, rule, wrap = case
    e3t, *statics = ref.case_arrays(case)
    want = ref.face_thickness(e3t, rule, *statics, wrap=wrap, markers=EM, static_markers=SM)
    npointers = 6 if rule == ref.ANOMALY else 3
    for moved in [None] + (list(range(npointers)) if nx in (514, 1028) else [0]):
        shifts = tuple(1 if k == moved else 0 for k in range(6))
        vec = ref.lane_width(nx, e3t.dtype.itemsize, moved is not None)
        got = _call(e3t, rule, statics, wrap, shifts)
        for g, w, name in zip(got, want, ('e3u', 'e3v')):
            label = f'{ref.wide_id(case)} {name} moved={moved}'
            assert _report(g, w, label, vec), label
            assert ref.same_bits(g, w), label


@pytest.mark.parametrize('real', ['float64', 'float32'])
def test_markers_off_and_the_python_call(real):
    import torch
    from nemoflux_amd._lib import DeviceArray
    from nemoflux_amd.thickness import face_thickness
    e3t, e3t0, e3u0, e3v0 = ref.make_case(real, 7, 37, 73, ref.ANOMALY, seed=3)
    # without markers the marker values are data
    want = ref.face_thickness(e3t, ref.MIN, wrap=False)
    assert not ref.same_bits(want[0], ref.face_thickness(e3t, ref.MIN, wrap=False, markers=EM)[0])
    got = _call(e3t, ref.MIN, wrap=False, markers=False)
    assert ref.same_bits(got[0], want[0]) and ref.same_bits(got[1], want[1])
    # the Python call: tensors with new outputs, DeviceArrays with out=
    d = [torch.from_numpy(a).cuda() for a in (e3t, e3t0, e3u0, e3v0)]
    u, v = face_thickness(d[0], 'anomaly', d[1], d[2], d[3], wrapX=True, markers=EM, static_markers=SM)
    torch.cuda.synchronize()
    want = ref.face_thickness(e3t, 'anomaly', e3t0, e3u0, e3v0, markers=EM, static_markers=SM)
    assert ref.same_bits(u.cpu().numpy(), want[0]) and ref.same_bits(v.cpu().numpy(), want[1])
    outs = [torch.empty_like(d[0]) for _ in range(2)]
    arrs = [DeviceArray(x.data_ptr(), x.shape, real, keepalive=x) for x in [d[0]] + outs]
    res = face_thickness(arrs[0], 'mean', wrapX=False, markers=(ref.EFILL, None), out=(arrs[1], arrs[2]))
    assert res[0] is arrs[1] and res[1] is arrs[2]
    torch.cuda.synchronize()
    want = ref.face_thickness(e3t, 'mean', wrap=False, markers=(ref.EFILL,))
    assert ref.same_bits(outs[0].cpu().numpy(), want[0]) and ref.same_bits(outs[1].cpu().numpy(), want[1])
    with pytest.raises(RuntimeError, match='needs out='):
        face_thickness(arrs[0])
    with pytest.raises(RuntimeError, match='e3t0 is'):
        face_thickness(d[0], 'anomaly', d[1][:-1], d[2], d[3])
    with pytest.raises(RuntimeError, match='need .nz, ny, nx.'):
        face_thickness(d[0][0])
    with pytest.raises(RuntimeError, match='overlaps'):
        face_thickness(d[0], out=(d[0], outs[1]))


@pytest.mark.parametrize('rule', ['min', 'anomaly'])
@pytest.mark.parametrize('real', ['float64', 'float32'])
def test_a_static_e3t_with_a_leading_one_equals_the_plain_form(real, rule):
    """Field.setCellThickness(FaceThickness(e3t)) with e3t (1, nz, ny, nx) and (nz, ny, nx), on the host and in HBM: the same
    static thickness, the restatement's bits, in the engine's own buffers"""
    from gpu_helpers import _on
    from nemoflux_amd._lib import lib, check
    from nemoflux_amd.thickness import FaceThickness
    from test_gpu_depth_remap import _make
    from test_gpu_gross import GRIDS, NZ
    grid = GRIDS[1]
    e3t, *statics = ref.make_case(real, NZ, grid[1], grid[0], rule, seed=11)
    want = ref.want_series(e3t, rule, statics)
    rows = []
    for lead in (False, True):
        for resident in (True, False):
            f = _make(real, grid, True)
            f.setCellThickness(FaceThickness(_on(e3t[None] if lead else e3t, resident), rule,
                                             *[None if s is None else _on(s, resident) for s in statics],
                                             fill_value=EM[0], missing_value=EM[1], static_fill_value=SM[0],
                                             static_missing_value=SM[1]))
            assert f._e3['nt'] == 1 and not f._cell_thickness_lazy()
            for a, w in zip(f._e3['arrays'], want):
                host = numpy.empty(a.shape, a.dtype)
                check(lib.nf_memcpy_d2h(host.ctypes.data, a.ptr, host.nbytes))
                assert ref.same_bits(host, w)
            rows.append(f.computeFluxProfile(1)[1])
    assert numpy.abs(rows[0]).max() > 0 and all(numpy.array_equal(r, rows[0]) for r in rows[1:])
