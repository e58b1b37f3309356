"""z* thicknesses from the sea surface height on the GPU, the raw ABI: nf_ssh_thickness and nf_column_depth against the numpy
restatement of tests/ssh_thickness_reference.py bit for bit -- every operation of the definition is one correctly rounded IEEE
float64 operation in a fixed order -- on the inputs whose branch shares tests/test_ssh_thickness_cpu.py asserts: (nz, ny, nx) =
(7, 36, 72), (7, 37, 73) (one value per lane), (1, 36, 72) and one launch of (3, 1, 5); nz = 7 and nz = 1 end in a short level
group; both dtypes, with and without areas, wrapX on and off, supplied and computed column depths, guard words around both
outputs and around h_out, every base pointer in turn moved by one element.  Past one column chunk of 256 lanes (WIDE_SHAPES
of tests/face_thickness_reference.py: nx = 512 to 2052, nz = 9 in two level groups) in both lane forms, nf_column_depth too:
two, three and more chunks, a full last chunk and one of a single lane, the east neighbour that another chunk holds.  Then the
three exact closed forms on the device, and the Python calls."""
import numpy
import pytest

import face_thickness_reference as fref
import ssh_thickness_reference as ref

pytestmark = pytest.mark.gpu

NF_F64, NF_F32 = 0, 1
GUARD = -7.0
PAD = 16
CASES = ref.raw_cases()
WIDE = ref.wide_cases()
EM, SM = ref.EM, ref.SM
NAN2 = (numpy.nan, numpy.nan)


def _device(a, shift):
    """a host array on the device behind `shift` leading elements: (tensor that owns it, address of a's first element)"""
    import torch
    host = numpy.full(a.size + shift + 4, 3.25, a.dtype)
    host[shift:shift + a.size] = a.reshape(-1)
    t = torch.from_numpy(host).cuda()
    return t, t.data_ptr() + shift * a.dtype.itemsize


def _guarded(n, shift, dtype):
    import torch
    t = torch.full((n + 2 * PAD + shift,), GUARD, dtype=dtype, device='cuda')
    return t, t.data_ptr() + (PAD + shift) * t.element_size()


def _inside(t, n, shift, what):
    got = t.cpu().numpy()
    assert (got[:PAD + shift] == GUARD).all() and (got[PAD + shift + n:] == GUARD).all(), f'{what} was written outside its array'
    return got[PAD + shift:PAD + shift + n]


def _depth(e3_0, shifts=(0, 0), markers=SM):
    """nf_column_depth on a host input, the guard words around h_out checked; shifts: of h_out and of e3_0"""
    import torch
    from nemoflux_amd._lib import lib
    nz, ny, nx = e3_0.shape
    keep, ptr = _device(e3_0, shifts[1])
    h, hptr = _guarded(ny * nx, shifts[0], torch.float64)
    rc = lib.nf_column_depth(hptr, ptr, nz, ny, nx, NF_F32 if e3_0.dtype == numpy.float32 else NF_F64, markers[0], markers[1],
                             None)
    assert rc == 0, lib.nf_last_error()
    assert lib.nf_synchronize() == 0
    assert ref.same_bits(keep.cpu().numpy()[shifts[1]:shifts[1] + e3_0.size], e3_0.reshape(-1))
    return _inside(h, ny * nx, shifts[0], 'h_out').reshape(ny, nx)


def _call(ssh, e3u0, e3v0, hu0=None, hv0=None, areas=None, wrap=True, markers=EM, static_markers=SM, shifts=(0,) * 10):
    """nf_ssh_thickness on host inputs: (e3u, e3v), with the guard words around both outputs checked; column depths that are
    not supplied come from nf_column_depth.  shifts: the number of elements by which e3u_out, e3v_out, ssh, e3u0, e3v0, hu0,
    hv0, area_t, area_u, area_v are moved off their allocation's base"""
    import torch
    from nemoflux_amd._lib import lib
    nz, ny, nx = e3u0.shape
    real, n = e3u0.dtype, e3u0.size
    if hu0 is None:
        hu0, hv0 = _depth(e3u0, markers=static_markers), _depth(e3v0, markers=static_markers)
    arrays = (ssh, e3u0, e3v0, numpy.asarray(hu0, numpy.float64), numpy.asarray(hv0, numpy.float64)) + \
        ((None, None, None) if areas is None else tuple(numpy.asarray(a, numpy.float64) for a in areas))
    ins = [(None, None) if a is None else _device(a, s) for a, s in zip(arrays, shifts[2:])]
    outs = [_guarded(n, s, ins[1][0].dtype) for s in shifts[:2]]
    rc = lib.nf_ssh_thickness(outs[0][1], outs[1][1], *[p for _, p in ins], nz, ny, nx, NF_F32 if real == numpy.float32 else NF_F64,
                              1 if wrap else 0, markers[0], markers[1], static_markers[0], static_markers[1], None)
    assert rc == 0, lib.nf_last_error()
    assert lib.nf_synchronize() == 0
    res = [_inside(t, n, s, 'an output').reshape(nz, ny, nx) for (t, _), s in zip(outs, shifts[:2])]
    for (keep, _), a, s in zip(ins, arrays, shifts[2:]):        # the inputs are only read
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
    real, nz, ny, nx, areas, wrap, supplied = case
    ssh, e3u0, e3v0, kw = ref.case_inputs(case)
    want = ref.ssh_thickness(ssh, e3u0, e3v0, **kw)
    pointers = list(range(7)) + ([7, 8, 9] if areas else [])
    for moved in [None] + pointers:
        shifts = tuple(1 if k == moved else 0 for k in range(10))
        got = _call(ssh, e3u0, e3v0, shifts=shifts, **kw)
        for g, w, name in zip(got, want, ('e3u', 'e3v')):
            label = f'{ref.case_id(case)} {name} moved={moved}'
            assert _report(g, w, label), label
            assert ref.same_bits(g, w), label


@pytest.mark.parametrize('case', WIDE, ids=[ref.wide_id(c) for c in WIDE])
def test_raw_abi_past_one_column_chunk(case):
    """rows of two and more chunks of 256 lanes, a full last chunk and one of a single lane (tests/face_thickness_reference.py,
    WIDE_SHAPES), nz = 9 in two level groups: the bases as the allocator gives them -- 16-byte lanes where nx allows -- and
    e3u_out moved by one element -- one value per lane, more chunks; where a last chunk holds one lane, every base in turn.
    The column depths that are not supplied come from nf_column_depth on the same rows."""
    real, nz, ny, nx, areas, wrap, supplied = case
    ssh, e3u0, e3v0, kw = ref.case_inputs(case)
    want = ref.ssh_thickness(ssh, e3u0, e3v0, **kw)
    pointers = list(range(7)) + ([7, 8, 9] if areas else [])
    for moved in [None] + (pointers if nx in (514, 1028) else [0]):
        shifts = tuple(1 if k == moved else 0 for k in range(10))
        vec = ref.lane_width(nx, e3u0.dtype.itemsize, moved is not None)
        got = _call(ssh, e3u0, e3v0, shifts=shifts, **kw)
        for g, w, name in zip(got, want, ('e3u', 'e3v')):
            label = f'{ref.wide_id(case)} {name} moved={moved}'
            assert _report(g, w, label, vec), label
            assert ref.same_bits(g, w), label


@pytest.mark.parametrize('real', ['float64', 'float32'])
def test_full_level_groups_and_a_short_last_one(real):
    """nz = 17: two full groups of the kernel's 8 levels and a last one of 1 (the shapes above end in their first group)"""
    c = ref.make_case(real, 17, 5, 40, seed=6)
    for areas in (None, c['areas']):
        want = ref.ssh_thickness(c['ssh'], c['e3u0'], c['e3v0'], areas=areas, markers=EM, static_markers=SM)
        for shifts in ((0,) * 10, (1,) + (0,) * 9):
            got = _call(c['ssh'], c['e3u0'], c['e3v0'], areas=areas, shifts=shifts)
            assert ref.same_bits(got[0], want[0]) and ref.same_bits(got[1], want[1])
            assert (want[0][16] != 0).any() and (want[0][8] != want[0][0]).any()


@pytest.mark.parametrize('shape', ref.SHAPES, ids=lambda s: 'x'.join(str(n) for n in s))
@pytest.mark.parametrize('real', ['float64', 'float32'])
def test_column_depth_is_the_restatement_bit_for_bit(real, shape):
    nz, ny, nx = shape
    c = ref.make_case(real, nz, ny, nx, seed=21)
    for e3_0 in (c['e3u0'], c['e3v0']):
        want = ref.column_depth(e3_0, SM)
        assert (want == 0).any() and (want > 0).any()
        for shifts in ((0, 0), (1, 0), (0, 1)):
            assert ref.same_bits(_depth(e3_0, shifts), want), shifts
    # without markers the marker values are data: they are added as they come
    want = ref.column_depth(c['e3u0'])
    assert not ref.same_bits(want, ref.column_depth(c['e3u0'], SM))
    assert ref.same_bits(_depth(c['e3u0'], markers=NAN2), want)


WIDE_DEPTH = [(real, shape) for real in ('float64', 'float32') for shape in ref.WIDE_SHAPES[real]]


@pytest.mark.parametrize('real,shape', WIDE_DEPTH, ids=[
    f'{r}-{"x".join(str(n) for n in s)}-{ref.lane_forms(s[2], numpy.dtype(r).itemsize)}' for r, s in WIDE_DEPTH])
def test_column_depth_past_one_column_chunk(real, shape):
    """rows of two and more chunks: e3_0 as the allocator gives it, h_out moved (the lane form of e3_0 stays), e3_0 moved (one
    value per lane, more chunks)"""
    nz, ny, nx = shape
    c = ref.make_case(real, nz, ny, nx, seed=21)
    for e3_0 in (c['e3u0'], c['e3v0']):
        want = ref.column_depth(e3_0, SM)
        assert (want == 0).any() and (want > 0).any()
        for shifts in ((0, 0), (1, 0), (0, 1)):
            vec = ref.lane_width(nx, e3_0.dtype.itemsize, shifts[1] != 0)
            got = _depth(e3_0, shifts)
            label = f'{real} {shape} h_out shifts={shifts}'
            assert _report(got[None], want[None], label, vec), label
            assert ref.same_bits(got, want), label


@pytest.mark.parametrize('real', ['float64', 'float32'])
def test_closed_forms_on_the_device(real):
    # ssh = 0: the statics where they are present
    c = ref.make_case(real, 7, 37, 73, seed=3)
    zero = numpy.zeros((37, 73), real)
    for areas in (None, c['areas']):
        got = _call(zero, c['e3u0'], c['e3v0'], areas=areas)
        for g, F0 in zip(got, (c['e3u0'], c['e3v0'])):
            assert numpy.array_equal(g, numpy.where(ref.present(F0, SM), F0, 0))
    # columns that sum to 8 on the lattice of 1/8: F0 + F0 s / 8, every step exact
    ssh, e3u0, e3v0 = ref.flat_bottom_case(real, 5, 36, 72)
    for wrap in (True, False):
        got = _call(ssh, e3u0, e3v0, wrap=wrap, markers=NAN2)
        Se, Sn = fref._neighbours(ssh, wrap)
        for g, F0, Sb in zip(got, (e3u0, e3v0), (Se, Sn)):
            F = F0.astype(numpy.float64)
            with numpy.errstate(all='ignore'):
                want = numpy.where(ref.present(F0, SM), F + F * (0.5 * (ssh.astype(numpy.float64) + Sb)) / 8., 0.0)
            assert numpy.array_equal(g.astype(numpy.float64), want)
    # areas all equal to one power of two: the rows without areas
    c = ref.make_case(real, 7, 36, 72, seed=4)
    plain = _call(c['ssh'], c['e3u0'], c['e3v0'])
    for a in (0.25, 4096.0):
        got = _call(c['ssh'], c['e3u0'], c['e3v0'], areas=tuple(numpy.full((36, 72), a) for _ in range(3)))
        assert ref.same_bits(got[0], plain[0]) and ref.same_bits(got[1], plain[1])


@pytest.mark.parametrize('real', ['float64', 'float32'])
def test_markers_off_and_the_python_calls(real):
    import torch
    from nemoflux_amd._lib import DeviceArray
    from nemoflux_amd.thickness import column_depth, ssh_thickness
    c = ref.make_case(real, 7, 37, 73, seed=5)
    ssh, e3u0, e3v0 = c['ssh'], c['e3u0'], c['e3v0']
    # without markers the marker values are data
    want = ref.ssh_thickness(ssh, e3u0, e3v0, c['hu0'], c['hv0'], wrap=False)
    assert not ref.same_bits(want[0], ref.ssh_thickness(ssh, e3u0, e3v0, c['hu0'], c['hv0'], wrap=False, markers=EM)[0])
    with numpy.errstate(all='ignore'):
        got = _call(ssh, e3u0, e3v0, c['hu0'], c['hv0'], wrap=False, markers=NAN2, static_markers=NAN2)
    assert ref.same_bits(got[0], want[0]) and ref.same_bits(got[1], want[1])
    # the Python calls: tensors with new outputs and computed column depths, DeviceArrays with out=
    d = {k: torch.from_numpy(numpy.ascontiguousarray(c[k])).cuda() for k in ('ssh', 'e3u0', 'e3v0', 'hu0', 'hv0')}
    areas = tuple(torch.from_numpy(a).cuda() for a in c['areas'])
    h = column_depth(d['e3u0'], SM)
    torch.cuda.synchronize()
    assert ref.same_bits(h.cpu().numpy(), ref.column_depth(e3u0, SM))
    u, v = ssh_thickness(d['ssh'], d['e3u0'], d['e3v0'], areas=areas, wrapX=True, markers=EM, static_markers=SM)
    torch.cuda.synchronize()
    want = ref.ssh_thickness(ssh, e3u0, e3v0, areas=c['areas'], markers=EM, static_markers=SM)
    assert ref.same_bits(u.cpu().numpy(), want[0]) and ref.same_bits(v.cpu().numpy(), want[1])
    outs = [torch.empty_like(d['e3u0']) for _ in range(2)]
    arr = {k: DeviceArray(x.data_ptr(), x.shape, x.cpu().numpy().dtype, keepalive=x) for k, x in d.items()}
    oarr = [DeviceArray(x.data_ptr(), x.shape, real, keepalive=x) for x in outs]
    res = ssh_thickness(arr['ssh'], arr['e3u0'], arr['e3v0'], arr['hu0'], arr['hv0'], wrapX=False, markers=(ref.EFILL, None),
                        static_markers=SM, out=oarr)
    assert res[0] is oarr[0] and res[1] is oarr[1]
    torch.cuda.synchronize()
    want = ref.ssh_thickness(ssh, e3u0, e3v0, c['hu0'], c['hv0'], wrap=False, markers=(ref.EFILL,), static_markers=SM)
    assert ref.same_bits(outs[0].cpu().numpy(), want[0]) and ref.same_bits(outs[1].cpu().numpy(), want[1])
    with pytest.raises(RuntimeError, match='needs out='):
        ssh_thickness(arr['ssh'], arr['e3u0'], arr['e3v0'], arr['hu0'], arr['hv0'])
    with pytest.raises(RuntimeError, match='needs hu0= and hv0='):
        ssh_thickness(arr['ssh'], arr['e3u0'], arr['e3v0'], out=oarr)
    with pytest.raises(RuntimeError, match='e3v0 is'):
        ssh_thickness(d['ssh'], d['e3u0'], d['e3v0'][:-1])
    with pytest.raises(RuntimeError, match='ssh is'):
        ssh_thickness(d['ssh'][:-1], d['e3u0'], d['e3v0'])
    with pytest.raises(RuntimeError, match='hu0 is'):
        ssh_thickness(d['ssh'], d['e3u0'], d['e3v0'], d['hu0'].float(), d['hv0'])
    with pytest.raises(RuntimeError, match='overlaps'):
        ssh_thickness(d['ssh'], d['e3u0'], d['e3v0'], d['hu0'], d['hv0'], out=(d['e3u0'], outs[1]))
    with pytest.raises(RuntimeError, match='out is'):
        column_depth(d['e3u0'], out=d['hu0'][:-1])
