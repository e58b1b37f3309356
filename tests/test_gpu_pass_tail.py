"""The tail of a per-step pass (nf_field_compute_all_async with one launch per time step): inner steps store only the two
signed planes ("pass_inner_signed") and whole steps are reduced two at a time ("pass_k3_pairs").  Both knobs on against
both off must give the same bits: rows, the resident planes and |.| arrays of the last step, the running max, a
computeFlux read-back after the pass, compact mode, sharded slab ranges and a replayed hipGraph."""
import contextlib
import ctypes
import io

import numpy
import pytest

from conftest import transect_xyz

pytestmark = pytest.mark.gpu

PSI_ZT = "(1+10*z)*(t+1)*(cos(2*pi*y/360) + sin(2*pi*x/360))"
T_TRI = "(-100,-80),(100,-80),(0,80),(-100,-80)"
T_OPEN = "(-100,-80),(100,-80),(0,80)"
NX, NY, NZ = 72, 36, 7
KNOBS = (b'pass_inner_signed', b'pass_k3_pairs')


def _case(nt, real):
    from nemoflux_amd.datagen import DataGen
    dg = DataGen(real=real)
    dg.setSizes(NX, NY, NZ, nt)
    dg.setBoundingBox(-180., 180., -90., 90., 0., 1.)
    dg.build()
    dg.applyStreamFunction(PSI_ZT)
    dg.computeUVFromPotential()
    tr = [transect_xyz(T_OPEN), transect_xyz(T_TRI)]
    return dg, (dg.bounds_lon, dg.bounds_lat, dg.deptht_bounds, dg.u, dg.v, tr)


def _field(args, **kw):
    from nemoflux_amd.field import Field
    with contextlib.redirect_stdout(io.StringIO()):
        return Field.fromArrays(*args, **kw)


@contextlib.contextmanager
def _tuning(on, field_split=-1):
    """batch_steps = 0: the per-step path; field_split = 0 forces the two-field kernel that the big grids run."""
    from nemoflux_amd._lib import lib, check
    try:
        check(lib.nf_tuning_set(b'batch_steps', 0))
        check(lib.nf_tuning_set(b'field_split', field_split))
        for k in KNOBS:
            check(lib.nf_tuning_set(k, 1 if on else 0))
        yield
    finally:
        for k in KNOBS:
            check(lib.nf_tuning_set(k, 1))
        check(lib.nf_tuning_set(b'field_split', -1))
        check(lib.nf_tuning_set(b'batch_steps', 1))


def _resident(f):
    """What read_step returns after a pass: the (ncell,4) planes, |eU|, |eV| and the running max."""
    from nemoflux_amd import _lib
    from nemoflux_amd._lib import lib, check
    iV = numpy.zeros((NY * NX, 4))
    eU = numpy.zeros(NY * NX)
    eV = numpy.zeros(NY * NX)
    m = ctypes.c_double()
    check(lib.nf_field_read_step(ctypes.byref(f._h), _lib.dptr(iV), _lib.dptr(eU), _lib.dptr(eV), ctypes.byref(m)))
    return iV, eU, eV, m.value


def _pass(args, on, field_split=-1, **kw):
    with _tuning(on, field_split):
        f = _field(args, **kw)
        tot, seg = f.computeAll()
        res = _resident(f)
    return f, (tot, seg) + res


def _same(a, b, what):
    for x, y in zip(a, b):
        assert numpy.array_equal(x, y), what


@pytest.mark.parametrize('field_split', [-1, 0])
@pytest.mark.parametrize('nt', [1, 2, 5, 8])
@pytest.mark.parametrize('real', ['float64', 'float32'])
def test_pass_tail_knobs_bit_identical(real, nt, field_split):
    """Whole passes and sharded ranges: partial at both ends, whole steps only, inside one step, partial at one end."""
    dg, args = _case(nt, real)
    total = nt * NZ
    ranges = [None, (3, total - 2), (NZ, total), (8, 13) if nt > 1 else (2, 5), (3, total), (0, total - 4)]
    for sr in ranges:
        kw = {} if sr is None else {'slab_range': sr}
        f_off, off = _pass(args, False, field_split, **kw)
        f_on, on = _pass(args, True, field_split, **kw)
        _same(on, off, (real, nt, field_split, sr))
        if sr is None:
            for t in sorted({0, nt - 1, nt // 2}):    # a single step after the pass: the step's own form
                with _tuning(True, field_split):
                    a = f_on.computeFlux(t, readback=True)
                with _tuning(False, field_split):
                    b = f_off.computeFlux(t, readback=True)
                assert a == b, (real, nt, t)
                assert numpy.array_equal(f_on.integratedVelocity, f_off.integratedVelocity)
                assert numpy.array_equal(f_on.edgeFluxesUArray, f_off.edgeFluxesUArray)
                assert numpy.array_equal(f_on.edgeFluxesVArray, f_off.edgeFluxesVArray)


@pytest.mark.parametrize('real', ['float64', 'float32'])
def test_pass_tail_last_step_planes_are_whole(real):
    """After a pass the resident planes are the last step's, complete: the neighbour copies and |.| agree with the signed
    planes (field.py:219-232), and they equal a single computeFlux of that step."""
    dg, args = _case(5, real)
    f, (tot, seg, iV, eU, eV, m) = _pass(args, True, 0)
    p = iV.reshape(NY, NX, 4)
    assert numpy.array_equal(p[1:, :, 0], p[:-1, :, 2]) and numpy.all(p[0, :, 0] == 0)
    assert numpy.array_equal(p[:, 1:, 3], p[:, :-1, 1]) and numpy.array_equal(p[:, 0, 3], p[:, -1, 1])
    assert numpy.array_equal(eU, numpy.abs(p[..., 1]).ravel()) and numpy.array_equal(eV, numpy.abs(p[..., 2]).ravel())
    with _tuning(False, 0):
        ref = _field(args)
        ref.computeFlux(4, readback=True)
    assert numpy.array_equal(ref.integratedVelocity, iV)


@pytest.mark.parametrize('real', ['float64', 'float32'])
def test_pass_tail_compact_mode(real):
    dg, args = _case(5, real)
    for sr in (None, (3, 31)):
        kw = {'compact': True} if sr is None else {'compact': True, 'slab_range': sr}
        _, off = _pass(args, False, **kw)
        _, on = _pass(args, True, **kw)
        _same(on, off, (real, sr))


@pytest.mark.parametrize('nt', [2, 5, 8])
def test_pass_tail_graph_replay_equals_direct(nt):
    """computeAll on a non-null stream captures the pass with both knobs on and replays it: the rows and the resident
    planes are those of direct launches with both knobs off; flipping a knob re-captures."""
    import torch
    from nemoflux_amd._lib import lib, check
    dg, args = _case(nt, 'float64')
    _, ref = _pass(args, False, readback=False)
    st = torch.cuda.Stream()
    torch.cuda.synchronize()
    with torch.cuda.stream(st):
        with _tuning(True, 0):
            g = _field(args, readback=False, stream=st.cuda_stream)
            out = torch.zeros((nt, g._rowlen), dtype=torch.float64, device='cuda')
            for rep in range(3):                    # capture, then two replays
                tot, seg = g.computeAll(out=out)
                assert numpy.array_equal(tot, ref[0]) and numpy.array_equal(seg, ref[1]), rep
            _same(_resident(g)[:3], ref[2:5], 'graph replay')
            check(lib.nf_tuning_set(b'pass_k3_pairs', 0))
            tot, seg = g.computeAll(out=out)
            assert numpy.array_equal(tot, ref[0]) and numpy.array_equal(seg, ref[1])
    torch.cuda.synchronize()


def test_pass_tail_timing_counts_one_launch_per_step():
    """nf_field_timing_read: one timed launch per flux launch, whatever the pairing; the K3 time is summed over all of it."""
    dg, args = _case(5, 'float64')
    for on in (False, True):
        with _tuning(on, 0):
            f = _field(args, readback=False)
            f.enableKernelTiming(True)
            f.computeAll()
            n, ms = f.readKernelTiming()
            k3 = f.readTransectTiming()
            f.enableKernelTiming(False)
        assert n == 5 and ms > 0 and k3 > 0, (on, n, ms, k3)
