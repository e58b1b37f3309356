"""Time means over selected, weighted steps on the GPU: nf_time_mean_steps and nf_time_mean_weighted_steps against the numpy
restatement of tests/selected_mean_reference.py bit for bit (both dtypes; the 16-byte form, the one-value form through odd
offsets and through a single odd offset in an aligned table; tables of 1 .. 33 steps from a source of 24, the table travels in
launches of B = 16 steps; ascending, strided, shuffled and repeated offsets; month-length and random weights; both rules; guard
words; every cut into two and three calls; unit and power-of-two weights against nf_time_mean / nf_time_mean_weighted on the
same memory; the argument errors); Field.timeMean(select=, weights=) in HBM, on the host and from .npz bundles against a Field
of the restatement's arrays, with and without a time-varying cell thickness; unselected steps of a file-backed source are never
read; Field.meanEddySplit: the split closes for the products that are linear in (uo, vo), does not for a tracer that varies with
the flow, and is assembled as documented.

Grids 72 x 36 x 7 x 7 and 73 x 37 x 7 x 7 (odd: every other step of an array is not 16-byte aligned).  computeClassTransport
refuses a cell thickness, so under a thickness the Field test checks the four other products and that refusal.

Bars.  An anchor's bar is that of tests/test_gpu_weighted_mean.py, 1e-12 x (mean over the visited steps of sum |terms| + sum
|terms| of the mean state).  With weights the error of sum w_j rows_j / sum w_j is bounded by the weighted mean of the steps' sum
|terms|; the tests take the smaller of the weighted and the plain mean over the visited steps, so the bar is never wider than
either reading.

Measured on an MI355X: the rows of the mean state 1.2e-4 of their bar at worst; the eddy part of the linear products 0.038 of
it (the remapped class rows at float64, 3.4e-3 or less elsewhere); the eddy part of a tracer that varies with the flow 4e9 x
the bar; 56 tests in 3.8 s."""
import numpy
import pytest

from conftest import transect_xyz, write_classic_triple
from class_remap_reference import ClassRemapReference
from depth_remap_reference import DepthRemapReference
from gpu_helpers import _field, _on, _quiet, _rows
from resolved_reference import array_values
import selected_mean_reference as smr
import timemean_reference as tmr

pytestmark = pytest.mark.gpu

PSI_ZT = "(1+10*z)*(t+1)*(cos(2*pi*y/360) + sin(2*pi*x/360))"
LINES = ["(-100,-80),(100,-80),(0,80)", "(-100,-80),(100,-80),(0,80),(-100,-80)", "(150,-30),(179.5,-20),(179.9,10),(175,40)"]
NZ, NT = 7, 7
GRIDS = [(72, 36), (73, 37)]
FILL, MISSING = 1.e20, -999.             # uo / vo
TFILL, TMISSING = -32768., 12345.        # tracers
THFILL, THMISSING = -1.e30, 9999.        # e3u / e3v
REF = 4.25
EDGES = [4.2, 4.4, 4.6, 4.8]
DEPTH_EDGES, DEPTH_TOP = [0.5, 1.0, 2.0, 3.0], 0.0
BAR = 1e-12
TH = numpy.array([0.125, 0.25, 0.5, 0.375, 0.75, 1.0, 0.625])
DB = numpy.stack([numpy.concatenate([[0.], numpy.cumsum(TH)[:-1]]), numpy.cumsum(TH)], axis=1)
NF_F64, NF_F32 = 0, 1
NF_ERR_ARG = 1
B = 16                                   # kTmTable of nf_timemean.hip: the steps of the table one launch takes
SOURCE_STEPS = 24
SELECT = [0, 2, 3, 6]
WEIGHTS = [float(smr.MONTHS[t]) for t in SELECT]      # January, March, April, July


def _row(f):
    return numpy.array(f._row[:f._rowlen])


def _bits(a):
    return numpy.ascontiguousarray(a, dtype=numpy.float64).view(numpy.uint64)


# ---- 1. the raw ABI --------------------------------------------------------------------------------------------------------
def _windows(real, nwin, n, seed, thickness=False):
    """(nwin, n) values: velocities / tracers with NaN, both markers, -0.0 and a value missing in every window -- and, not for
    the weighted form (0 x inf), +inf and -inf, each in every window of its value (no +inf + -inf, whose NaN has no defined
    sign); or thicknesses in [0.2, 3] with NaN, both markers, exact zeros and a value that is never there"""
    rng = numpy.random.default_rng(seed)
    dt = numpy.dtype(real).type
    if thickness:
        win, marks = rng.uniform(0.2, 3., (nwin, n)).astype(real), (numpy.nan, THFILL, THMISSING, 0.0)
    else:
        win, marks = rng.standard_normal((nwin, n)).astype(real), (numpy.nan, FILL, MISSING, -0.0)
    flat = win.reshape(-1)
    for m in marks:
        flat[rng.choice(flat.size, (flat.size + 7) // 8, replace=False)] = dt(m)
    return win


def _special_columns(win, hwin, inf):
    nwin, n = win.shape
    dt = win.dtype.type
    if n < 3:
        return
    win[:, 0] = [(dt(FILL), numpy.nan, dt(MISSING))[t % 3] for t in range(nwin)]          # missing in every window
    if hwin is not None:
        hwin[:, 0] = dt(1.5)
        win[:, 1] = dt(0.75)
        hwin[:, 1] = [(dt(0.0), numpy.nan, dt(THFILL))[t % 3] for t in range(nwin)]       # never any water
    if inf and n >= 8:
        win[:, 5], win[:, 6] = numpy.inf, -numpy.inf


def _buffer(win, offsets):
    """a buffer that holds window t at element offsets[t]; what lies between the windows is never read"""
    nwin, n = win.shape
    buf = numpy.full(max(offsets) + n + 4, 7.25, win.dtype)
    for t in range(nwin):
        buf[offsets[t]:offsets[t] + n] = win[t]
    return buf


def _guards():
    import torch
    return (lambda n: torch.full((n + 4,), -7.0, dtype=torch.float64, device='cuda'),
            lambda n: torch.full((n + 8,), 77, dtype=torch.int32, device='cuda'))


def _acc_of(acc, n):
    a = acc.cpu().numpy()
    assert (a[:2] == -7.0).all() and (a[n + 2:] == -7.0).all(), 'acc / wsum was written outside its n values'
    return a[2:n + 2]


def _cnt_of(cnt, n):
    c = cnt.cpu().numpy()
    assert (c[:4] == 77).all() and (c[n + 4:] == 77).all(), 'cnt was written outside its n values'
    return c[4:n + 4].view(numpy.uint32)


def _tables(offsets, weights):
    import ctypes
    off = (ctypes.c_longlong * len(offsets))(*[int(x) for x in offsets])
    w = None if weights is None else (ctypes.c_double * len(weights))(*[float(x) for x in weights])
    return off, w


def _steps_call(dev, offsets, weights, n, code, first, last, rule, total, fill_out, acc, wsum, cnt, expect=0):
    """nf_time_mean_steps on the device buffer `dev`; acc / wsum / cnt: tensors with two (four) guard values on each side"""
    from nemoflux_amd._lib import lib, check
    off, w = _tables(offsets, weights)
    rc = lib.nf_time_mean_steps(acc.data_ptr() + 16, None if wsum is None else wsum.data_ptr() + 16,
                                None if cnt is None else cnt.data_ptr() + 16, dev.data_ptr(), off, w, len(offsets), n, code, FILL,
                                MISSING, first, last, rule, total, fill_out, None)
    if expect:
        assert rc == expect, rc
        return lib.nf_last_error()
    check(rc)
    check(lib.nf_synchronize())


def _wsteps_call(devs, offsets, hoffsets, weights, n, code, first, last, total, fill_out, accf, acch, cnt, expect=0):
    from nemoflux_amd._lib import lib, check
    off, w = _tables(offsets, weights)
    hoff, _ = _tables(hoffsets, None)
    rc = lib.nf_time_mean_weighted_steps(accf.data_ptr() + 16, acch.data_ptr() + 16, None if cnt is None else cnt.data_ptr() + 16,
                                         devs[0].data_ptr(), off, devs[1].data_ptr(), hoff, w, len(offsets), n, code, FILL,
                                         MISSING, THFILL, THMISSING, first, last, total, fill_out, None)
    if expect:
        assert rc == expect, rc
        return lib.nf_last_error()
    check(rc)
    check(lib.nf_synchronize())


def _patterns(nsteps, rng):
    """the window indices of a table of nsteps entries from SOURCE_STEPS windows: ascending, strided, shuffled, one repeated"""
    S = SOURCE_STEPS
    asc = sorted(rng.choice(S, nsteps, replace=False)) if nsteps <= S else sorted(rng.integers(0, S, nsteps))
    out = {'ascending': list(asc), 'strided': [(2 * j) % S for j in range(nsteps)],
           'shuffled': list(rng.permutation(S)[:nsteps]) if nsteps <= S else list(rng.integers(0, S, nsteps))}
    if nsteps >= 2:
        rep = list(asc)
        rep[nsteps // 2] = rep[0]
        out['repeated'] = rep
    return out


def _weights_of(kind, nsteps, rng):
    return numpy.resize(smr.MONTHS, nsteps) if kind == 'months' else rng.uniform(0.5, 4., nsteps)


# n, the stride of the windows: 4096 the 16-byte form; 4099 one value per lane through odd offsets; 1 and 3 with the windows
# back to back (one value) and 16 bytes apart in both dtypes (the 16-byte form: one lane that holds fewer values than it takes)
SHAPES = [(4096, 4096), (4099, 4099), (1, 1), (1, 4), (3, 3), (3, 4)]
NSTEPS = [1, 2, 9, 17, B, 2 * B + 1]     # B + 1 is 17


@pytest.mark.parametrize('real', ['float64', 'float32'])
def test_raw_abi_is_the_restatement_bit_for_bit(real):
    """one call that finishes under both rules (no wsum, no cnt: a chain of launches allocates what it carries) and one that
    carries (s, wp and c, and nothing in wsum under the velocity rule)"""
    import torch
    code = NF_F64 if real == 'float64' else NF_F32
    fill_out = float(numpy.dtype(real).type(FILL))
    new_acc, new_cnt = _guards()
    rng = numpy.random.default_rng(11)
    for n, stride in SHAPES:
        win = _windows(real, SOURCE_STEPS, n, 1000 + n + stride)
        _special_columns(win, None, inf=True)
        where = [t * stride for t in range(SOURCE_STEPS)]
        dev = torch.from_numpy(_buffer(win, where)).cuda()
        for k, nsteps in enumerate(NSTEPS):
            for name, idx in _patterns(nsteps, rng).items():
                w = _weights_of(('months', 'random')[(k + len(name)) % 2], nsteps, rng)
                offsets, rows = [where[t] for t in idx], win[idx]
                total = smr.total_weight(w) + 0.25          # not the sum: the divisor is the argument
                label = (n, stride, nsteps, name)
                s, wp, c = smr.accumulate(rows, w, (FILL, MISSING))
                for rule in (smr.OVER_STEPS, smr.OVER_PRESENT):
                    acc = new_acc(n)
                    _steps_call(dev, offsets, w, n, code, 1, 1, rule, total, fill_out, acc, None, None)
                    assert smr.same_bits(_acc_of(acc, n), smr.finish(s, wp, c, rule, total, fill_out)), (label, rule)
                    acc, wsum, cnt = new_acc(n), new_acc(n), new_cnt(n)
                    _steps_call(dev, offsets, w, n, code, 1, 0, rule, total, fill_out, acc, wsum, cnt)
                    assert smr.same_bits(_acc_of(acc, n), s) and numpy.array_equal(_cnt_of(cnt, n), c), (label, rule)
                    if rule == smr.OVER_PRESENT:
                        assert smr.same_bits(_acc_of(wsum, n), wp), label
                    else:
                        assert (_acc_of(wsum, n) == -7.0).all(), label       # not written under the velocity rule
                if n >= 8:
                    assert (c == 0).any() and numpy.isinf(s).any() and 0 < (c == nsteps).sum() < n


@pytest.mark.parametrize('real', ['float64', 'float32'])
def test_raw_abi_of_the_thickness_weighted_form_is_the_restatement_bit_for_bit(real):
    """the thicknesses lie in a buffer of their own, their windows in reverse order: the two offset tables differ"""
    import torch
    code = NF_F64 if real == 'float64' else NF_F32
    fill_out = float(numpy.dtype(real).type(FILL))
    new_acc, new_cnt = _guards()
    rng = numpy.random.default_rng(12)
    for n, stride in SHAPES:
        win, hwin = _windows(real, SOURCE_STEPS, n, 2000 + n + stride), _windows(real, SOURCE_STEPS, n, 3000 + n + stride, True)
        _special_columns(win, hwin, inf=False)
        where = [t * stride for t in range(SOURCE_STEPS)]
        hwhere = [(SOURCE_STEPS - 1 - t) * stride for t in range(SOURCE_STEPS)]
        devs = [torch.from_numpy(_buffer(win, where)).cuda(), torch.from_numpy(_buffer(hwin, hwhere)).cuda()]
        for k, nsteps in enumerate(NSTEPS):
            for name, idx in _patterns(nsteps, rng).items():
                w = _weights_of(('random', 'months')[(k + len(name)) % 2], nsteps, rng)
                offsets, hoffsets = [where[t] for t in idx], [hwhere[t] for t in idx]
                total = smr.total_weight(w) + 0.25
                label = (n, stride, nsteps, name)
                sF, sH, c = smr.accumulate_weighted(win[idx], hwin[idx], w, (FILL, MISSING), (THFILL, THMISSING))
                want, want_h = smr.finish_weighted(sF, sH, c, total, fill_out)
                accf, acch = new_acc(n), new_acc(n)
                _wsteps_call(devs, offsets, hoffsets, w, n, code, 1, 1, total, fill_out, accf, acch, None)
                assert smr.same_bits(_acc_of(accf, n), want) and smr.same_bits(_acc_of(acch, n), want_h), label
                accf, acch, cnt = new_acc(n), new_acc(n), new_cnt(n)
                _wsteps_call(devs, offsets, hoffsets, w, n, code, 1, 0, total, fill_out, accf, acch, cnt)
                assert smr.same_bits(_acc_of(accf, n), sF) and smr.same_bits(_acc_of(acch, n), sH), label
                assert numpy.array_equal(_cnt_of(cnt, n), c), label
                assert numpy.isfinite(want).all() and numpy.isfinite(want_h).all()
                if n >= 3:
                    assert (c == 0).any() and (want[c == 0] == fill_out).all()
                    assert ((sH == 0) & (c > 0)).any() and (want[(sH == 0) & (c > 0)] == 0).all()


@pytest.mark.parametrize('real', ['float64', 'float32'])
def test_one_odd_offset_in_an_aligned_table(real):
    """windows 16-byte aligned but for one, which begins one element late: the whole call takes one value per lane, in every
    launch of a chain, and gives the restatement's bits; so it does with acc, wsum or cnt off by one value instead"""
    import torch
    code, size = (NF_F64, 8) if real == 'float64' else (NF_F32, 4)
    n, nwin = 4096, 2 * B + 1
    new_acc, new_cnt = _guards()
    win, hwin = _windows(real, nwin, n, 41), _windows(real, nwin, n, 42, True)
    _special_columns(win, hwin, inf=False)
    w = _weights_of('random', nwin, numpy.random.default_rng(43))
    total = smr.total_weight(w)
    s, wp, c = smr.accumulate(win, w, (FILL, MISSING))
    sF, sH, _ = smr.accumulate_weighted(win, hwin, w, (FILL, MISSING), (THFILL, THMISSING))
    for odd in (0, B - 1, 2 * B):                 # in the first launch, at its end, alone in the last one
        where = [t * (n + 8) + (1 if t == odd else 0) for t in range(nwin)]
        hwhere = [t * (n + 8) for t in range(nwin)]
        devs = [torch.from_numpy(_buffer(win, where)).cuda(), torch.from_numpy(_buffer(hwin, hwhere)).cuda()]
        acc, wsum, cnt = new_acc(n), new_acc(n), new_cnt(n)
        _steps_call(devs[0], where, w, n, code, 1, 0, smr.OVER_PRESENT, total, numpy.nan, acc, wsum, cnt)
        assert smr.same_bits(_acc_of(acc, n), s) and smr.same_bits(_acc_of(wsum, n), wp) and numpy.array_equal(_cnt_of(cnt, n), c)
        accf, acch, cnt = new_acc(n), new_acc(n), new_cnt(n)
        _wsteps_call(devs, where, hwhere, w, n, code, 1, 0, total, numpy.nan, accf, acch, cnt)
        assert smr.same_bits(_acc_of(accf, n), sF) and smr.same_bits(_acc_of(acch, n), sH)
        _wsteps_call([devs[1], devs[0]], hwhere, where, w, n, code, 1, 0, total, numpy.nan, accf, acch, cnt)   # the odd one in thk
        swapped = smr.accumulate_weighted(hwin, win, w, (FILL, MISSING), (THFILL, THMISSING))
        assert smr.same_bits(_acc_of(accf, n), swapped[0]) and smr.same_bits(_acc_of(acch, n), swapped[1])
    # an aligned table, one of the carried arrays off by one value (8 or 4 bytes)
    from nemoflux_amd._lib import lib, check
    where = [t * (n + 8) for t in range(nwin)]
    dev = torch.from_numpy(_buffer(win, where)).cuda()
    off, wt = _tables(where, w)
    for shift in ((8, 0, 0), (0, 8, 0), (0, 0, 4)):
        acc, wsum = (torch.full((n + 8,), -7.0, dtype=torch.float64, device='cuda') for _ in range(2))
        cnt = new_cnt(n + 4)
        check(lib.nf_time_mean_steps(acc.data_ptr() + 16 + shift[0], wsum.data_ptr() + 16 + shift[1], cnt.data_ptr() + 16 + shift[2],
                                     dev.data_ptr(), off, wt, nwin, n, code, FILL, MISSING, 1, 0, smr.OVER_PRESENT, total, numpy.nan,
                                     None))
        check(lib.nf_synchronize())
        a, ws, cn = acc.cpu().numpy(), wsum.cpu().numpy(), cnt.cpu().numpy()
        ia, iw, ic = 2 + shift[0] // 8, 2 + shift[1] // 8, 4 + shift[2] // 4
        assert smr.same_bits(a[ia:ia + n], s) and (a[:ia] == -7.0).all() and (a[ia + n:] == -7.0).all(), shift
        assert smr.same_bits(ws[iw:iw + n], wp) and (ws[:iw] == -7.0).all() and (ws[iw + n:] == -7.0).all(), shift
        assert numpy.array_equal(cn[ic:ic + n].view(numpy.uint32), c) and (cn[:ic] == 77).all() and (cn[ic + n:] == 77).all(), shift


@pytest.mark.parametrize('real', ['float64', 'float32'])
def test_every_cut_into_two_and_three_calls_is_one_call_bit_for_bit(real):
    """a shuffled table of 9 entries with one repeated; first on the first call only, last on the last only"""
    import torch
    code = NF_F64 if real == 'float64' else NF_F32
    nsteps = 9
    new_acc, new_cnt = _guards()
    rng = numpy.random.default_rng(21)
    cuts = [(k, nsteps - k) for k in range(1, nsteps)] + [(i, j - i, nsteps - j) for i in range(1, nsteps) for j in range(i + 1, nsteps)]
    assert len(cuts) == 8 + 28
    for n, stride in ((4096, 4096), (4099, 4099), (3, 3)):
        win, hwin = _windows(real, SOURCE_STEPS, n, 51 + n), _windows(real, SOURCE_STEPS, n, 52 + n, True)
        _special_columns(win, hwin, inf=False)
        where = [t * stride for t in range(SOURCE_STEPS)]
        devs = [torch.from_numpy(_buffer(win, where)).cuda(), torch.from_numpy(_buffer(hwin, where)).cuda()]
        idx = list(rng.permutation(SOURCE_STEPS)[:nsteps])
        idx[6] = idx[1]
        off = [where[t] for t in idx]
        w = _weights_of('months', nsteps, rng)
        total = smr.total_weight(w)
        want = {rule: smr.selected_mean(win[idx], w, (FILL, MISSING), rule, total, numpy.nan) for rule in (0, 1)}
        wantw = smr.selected_weighted_mean(win[idx], hwin[idx], w, (FILL, MISSING), (THFILL, THMISSING), total, numpy.nan)
        for cut in cuts:
            for rule in (smr.OVER_STEPS, smr.OVER_PRESENT):
                acc, wsum, cnt = new_acc(n), new_acc(n), new_cnt(n)
                t = 0
                for k in cut:
                    _steps_call(devs[0], off[t:t + k], w[t:t + k], n, code, 1 if t == 0 else 0, 1 if t + k == nsteps else 0, rule,
                                total, numpy.nan, acc, wsum, cnt)
                    t += k
                assert smr.same_bits(_acc_of(acc, n), want[rule]), (n, cut, rule)
            accf, acch, cnt = new_acc(n), new_acc(n), new_cnt(n)
            t = 0
            for k in cut:
                _wsteps_call(devs, off[t:t + k], off[t:t + k], w[t:t + k], n, code, 1 if t == 0 else 0, 1 if t + k == nsteps else 0,
                             total, numpy.nan, accf, acch, cnt)
                t += k
            assert smr.same_bits(_acc_of(accf, n), wantw[0]) and smr.same_bits(_acc_of(acch, n), wantw[1]), (n, cut)
        assert numpy.isnan(want[1]).any() and numpy.isfinite(want[1]).any()


@pytest.mark.parametrize('real', ['float64', 'float32'])
def test_unit_and_power_of_two_weights_give_the_bits_of_the_existing_calls(real):
    """no weights, weights all 1 and weights all 4 on the offsets j * stride, total_weight = (1 or 4) x nsteps, against
    nf_time_mean / nf_time_mean_weighted on the same memory: numpy.array_equal on the bit patterns"""
    import torch
    from nemoflux_amd._lib import lib, check
    code = NF_F64 if real == 'float64' else NF_F32
    new_acc, _ = _guards()
    for n, stride in ((4096, 4096), (4099, 4099), (4096, 4100), (3, 3)):
        for nsteps in (1, 9, B + 1, SOURCE_STEPS):
            win, hwin = _windows(real, nsteps, n, 61 + n + nsteps), _windows(real, nsteps, n, 62 + n + nsteps, True)
            _special_columns(win, None, inf=True)
            where = [t * stride for t in range(nsteps)]
            dev, hdev = torch.from_numpy(_buffer(win, where)).cuda(), torch.from_numpy(_buffer(hwin, where)).cuda()
            for rule in (smr.OVER_STEPS, smr.OVER_PRESENT):
                old = new_acc(n)
                check(lib.nf_time_mean(old.data_ptr() + 16, None, dev.data_ptr(), nsteps, stride, n, code, FILL, MISSING, 1, 1, rule,
                                       nsteps, numpy.nan, None))
                check(lib.nf_synchronize())
                for w, total in ((None, float(nsteps)), ([1.0] * nsteps, float(nsteps)), ([4.0] * nsteps, 4.0 * nsteps)):
                    acc = new_acc(n)
                    _steps_call(dev, where, w, n, code, 1, 1, rule, total, numpy.nan, acc, None, None)
                    assert numpy.array_equal(_bits(_acc_of(acc, n)), _bits(_acc_of(old, n))), (n, stride, nsteps, rule, w and w[0])
            # the weighted pair: no +-inf beside a thickness that may be 0
            win = numpy.where(numpy.isinf(win), win.dtype.type(0.5), win)
            dev = torch.from_numpy(_buffer(win, where)).cuda()
            oldf, oldh = new_acc(n), new_acc(n)
            check(lib.nf_time_mean_weighted(oldf.data_ptr() + 16, oldh.data_ptr() + 16, None, dev.data_ptr(), stride, hdev.data_ptr(),
                                            stride, nsteps, n, code, FILL, MISSING, THFILL, THMISSING, 1, 1, nsteps, numpy.nan, None))
            check(lib.nf_synchronize())
            for w, total in ((None, float(nsteps)), ([1.0] * nsteps, float(nsteps)), ([4.0] * nsteps, 4.0 * nsteps)):
                accf, acch = new_acc(n), new_acc(n)
                _wsteps_call([dev, hdev], where, where, w, n, code, 1, 1, total, numpy.nan, accf, acch, None)
                assert numpy.array_equal(_bits(_acc_of(accf, n)), _bits(_acc_of(oldf, n))), (n, stride, nsteps, w and w[0])
                assert numpy.array_equal(_bits(_acc_of(acch, n)), _bits(_acc_of(oldh, n))), (n, stride, nsteps, w and w[0])


def test_argument_errors_on_a_device():
    import torch
    n = 64
    new_acc, new_cnt = _guards()
    dev = torch.zeros(4 * n, dtype=torch.float64, device='cuda')
    acc, wsum, cnt = new_acc(n), new_acc(n), new_cnt(n)
    good = [0, n, 2 * n]
    for w in ([1., 0., 1.], [1., -2., 1.], [numpy.nan, 1., 1.], [1., 1., numpy.inf]):
        err = _steps_call(dev, good, w, n, NF_F64, 1, 1, 0, 3., numpy.nan, acc, wsum, cnt, expect=NF_ERR_ARG)
        assert err.startswith(b'nf_time_mean_steps:') and b'weight' in err, err
        err = _wsteps_call([dev, dev], good, good, w, n, NF_F64, 1, 1, 3., numpy.nan, acc, wsum, cnt, expect=NF_ERR_ARG)
        assert err.startswith(b'nf_time_mean_weighted_steps:') and b'weight' in err, err
    err = _steps_call(dev, [0, -n, n], None, n, NF_F64, 1, 1, 0, 3., numpy.nan, acc, wsum, cnt, expect=NF_ERR_ARG)
    assert b'offset' in err
    for offs in (([0, -1, n], good), (good, [-n, 0, n])):
        err = _wsteps_call([dev, dev], offs[0], offs[1], None, n, NF_F64, 1, 1, 3., numpy.nan, acc, wsum, cnt, expect=NF_ERR_ARG)
        assert b'offset' in err
    assert (_acc_of(acc, n) == -7.0).all() and (_acc_of(wsum, n) == -7.0).all() and (_cnt_of(cnt, n) == 77).all()


# ---- 2. Field.timeMean(select=, weights=) ----------------------------------------------------------------------------------
_CASES = {}


def _case(real, grid):
    """bounds; host u, v (nt, nz, ny, nx) with a land block and markers of all three kinds that come and go with time; a
    carried tracer and a class field (NaN and both markers, some varying in time; the tracer also with a trend in time, which
    the velocities have too: tau_trend); e3u, e3v: independent, time-varying, in [0.2, 3], with their own markers, NaN and
    exact zeros that come and go"""
    key = (real, grid)
    if key not in _CASES:
        from nemoflux_amd.datagen import DataGen
        nx, ny = grid
        dg = DataGen(real=real)
        dg.setSizes(nx, ny, NZ, NT)
        dg.setBoundingBox(-180., 180., -90., 90., 0., 1.)
        dg.build()
        dg.applyStreamFunction(PSI_ZT)
        dg.computeUVFromPotential()
        u, v = dg.u.cpu().numpy().copy(), dg.v.cpu().numpy().copy()
        v[:, :, -1, :] = 0                     # the generator's pole row is 1e13-sized garbage
        dt = u.dtype.type
        rng = numpy.random.default_rng(5)
        u[:, 3:, 4:9, 10:20] = dt(FILL)        # land: missing at every step
        v[:, 3:, 4:9, 10:20] = numpy.nan
        for a in (u, v):                       # and markers that come and go with time
            flat = a.reshape(-1)
            for m in (FILL, MISSING, numpy.nan):
                flat[rng.choice(flat.size, flat.size // 25, replace=False)] = dt(m)

        def tracer(trend):
            a = (4. + rng.random((NT, NZ, ny, nx)) + trend * numpy.arange(NT)[:, None, None, None]).astype(real)
            a[:, 1::3, 3:-2:3, 2:-2:4] = numpy.nan
            a[:, :, 10:14, 50:60] = dt(TFILL)
            a[:, 2:, 25:28, 5:12] = dt(TMISSING)
            flat = a.reshape(-1)
            flat[rng.choice(flat.size, flat.size // 20, replace=False)] = numpy.nan
            return a

        tau, sig, tau_trend = tracer(0.), tracer(0.), tracer(0.05)
        e3 = []
        for _ in range(2):
            a = rng.uniform(0.2, 3., (NT, NZ, ny, nx)).astype(real)
            flat = a.reshape(-1)
            for m in (THFILL, THMISSING, numpy.nan, 0.0):
                flat[rng.choice(flat.size, flat.size // 25, replace=False)] = dt(m)
            a[:, 5:, 20:24, 30:45] = dt(0.0)             # below the bottom: never any water
            e3.append(a)
        _CASES[key] = dict(blon=dg.bounds_lon.cpu().numpy(), blat=dg.bounds_lat.cpu().numpy(), uo=u, vo=v, tau=tau, sig=sig,
                           tau_trend=tau_trend, e3u=e3[0], e3v=e3[1])
    return _CASES[key]


def _lines():
    return [transect_xyz(s) for s in LINES]


def _source(real, grid, resident, thick=False, **arrays):
    """a Field of the case (or of `arrays` in place of the case's): tracer, class field, class and depth edges; thick: a
    time-varying cell thickness"""
    c = dict(_case(real, grid), **arrays)
    f = _field(c['blon'], c['blat'], DB, _on(c['uo'], resident), _on(c['vo'], resident), _lines(), readback=False,
               fill_value=FILL, missing_value=MISSING)
    f.setTracer(_on(c['tau'], resident), fill_value=TFILL, missing_value=TMISSING, reference=REF)
    f.setClassTracer(_on(c['sig'], resident), fill_value=TFILL, missing_value=TMISSING)
    f.setClassEdges(EDGES)
    f.setDepthEdges(DEPTH_EDGES, DEPTH_TOP)
    if thick:
        f.setCellThickness(_on(c['e3u'], resident), _on(c['e3v'], resident), fill_value=THFILL, missing_value=THMISSING)
    return f


CLASS_REFUSAL = 'nf_field_compute_class_transport: this form does not take per-cell thicknesses'


def _products(f, thick):
    """the rows of the five products of step 0 as [segments | transects]; under a cell thickness computeClassTransport
    refuses, with its own words"""
    f.computeFlux(0)
    out = {'computeFlux': _row(f), 'computeFluxProfile': _rows(f.computeFluxProfile(0)),
           'computeTracerFlux': _rows(f.computeTracerFlux(0)), 'computeDepthTransport': _rows(f.computeDepthTransport(0))}
    if thick:
        with pytest.raises(RuntimeError, match=CLASS_REFUSAL):
            f.computeClassTransport(0)
    else:
        out['computeClassTransport'] = _rows(f.computeClassTransport(0))
    return out


def _mean_arrays(real, grid, select, weights, thick, **arrays):
    """the restatement's arrays of the mean state over `select` with `weights`: {'uo', 'vo', 'tracer', 'class'[, 'e3u', 'e3v']}
    (1, nz, ny, nx) float64 and the fills (velocities, tracer, class field)"""
    c = dict(_case(real, grid), **arrays)
    (um, vm, fill), ((taum, tfill), (sigm, sfill)), hs = smr.field_selected_mean_arrays(
        c['uo'], c['vo'], (FILL, MISSING), select, weights, [(c['tau'], (TFILL, TMISSING)), (c['sig'], (TFILL, TMISSING))],
        (c['e3u'], c['e3v']) if thick else None, (THFILL, THMISSING))
    out = {'uo': um, 'vo': vm, 'tracer': taum, 'class': sigm}
    if thick:
        out['e3u'], out['e3v'] = hs
    return out, (fill, tfill, sfill)


def _want_field(real, grid, arrays, fills, thick):
    """fromArrays of the restatement's arrays"""
    c = _case(real, grid)
    fill, tfill, sfill = fills
    f = _field(c['blon'], c['blat'], DB, _on(arrays['uo'], True), _on(arrays['vo'], True), _lines(), readback=False, fill_value=fill)
    f.setTracer(_on(arrays['tracer'], True), fill_value=None if tfill != tfill else tfill, reference=REF)
    f.setClassTracer(_on(arrays['class'], True), fill_value=None if sfill != sfill else sfill)
    f.setClassEdges(EDGES)
    f.setDepthEdges(DEPTH_EDGES, DEPTH_TOP)
    if thick:
        f.setCellThickness(_on(arrays['e3u'], True), _on(arrays['e3v'], True))
    return f


def _write_npz(tmp_path, real, grid):
    c = _case(real, grid)
    paths = {k: str(tmp_path / f'{k}.npz') for k in 'TUV'}
    fv = lambda name, a, b: {f'_FillValue_{name}': numpy.array(a), f'_missing_value_{name}': numpy.array(b)}   # noqa: E731
    numpy.savez(paths['T'], bounds_lon=c['blon'], bounds_lat=c['blat'], deptht_bounds=DB, tau=c['tau'], sig=c['sig'],
                **fv('tau', TFILL, TMISSING), **fv('sig', TFILL, TMISSING))
    numpy.savez(paths['U'], uo=c['uo'], e3u=c['e3u'], **fv('uo', FILL, MISSING), **fv('e3u', THFILL, THMISSING))
    numpy.savez(paths['V'], vo=c['vo'], e3v=c['e3v'], **fv('vo', FILL, MISSING), **fv('e3v', THFILL, THMISSING))
    return paths


_WANT = {}


def _want_rows(real, grid, thick):
    """the rows of the Field of the restatement's arrays: computed once per (dtype, grid, thickness), shared by the homes"""
    key = (real, grid, thick)
    if key not in _WANT:
        arrays, fills = _mean_arrays(real, grid, SELECT, WEIGHTS, thick)
        assert fills == (float(numpy.dtype(real).type(FILL)), TFILL, TFILL)
        assert (arrays['uo'] == fills[0]).any() and (arrays['tracer'] == TFILL).any()
        _WANT[key] = _products(_want_field(real, grid, arrays, fills, thick), thick)
    return _WANT[key]


@pytest.mark.parametrize('thick', [False, True], ids=['plain', 'thickness'])
@pytest.mark.parametrize('home', ['hbm', 'host', 'npz'])
@pytest.mark.parametrize('grid', GRIDS, ids=lambda g: f'{g[0]}x{g[1]}')
@pytest.mark.parametrize('real', ['float64', 'float32'])
def test_selected_weighted_time_mean_against_a_field_of_the_restatement(real, grid, home, thick, tmp_path):
    from nemoflux_amd.field import Field
    if home == 'npz':
        paths = _write_npz(tmp_path, real, grid)
        src = _quiet(Field, paths['T'], paths['U'], paths['V'], _lines(), readback=False, unsupportedCells='refuse')
        src.setTracer((paths['T'], 'tau'), reference=REF)
        src.setClassTracer((paths['T'], 'sig'))
        src.setClassEdges(EDGES)
        src.setDepthEdges(DEPTH_EDGES, DEPTH_TOP)
        if thick:
            src.setCellThickness((paths['U'], 'e3u'), (paths['V'], 'e3v'))
    else:
        src = _source(real, grid, home == 'hbm', thick)
        if grid == GRIDS[1]:
            src._MEAN_STAGE_BYTES = 1          # host arrays go up one selected step at a time, everything carried between calls
    got = _quiet(src.timeMean, select=SELECT, weights=WEIGHTS, thicknessWeighted=thick)
    assert (got.nt, got.nz, got.ny, got.nx) == (1, NZ, grid[1], grid[0]) and got._uv_code == NF_F64
    rows, wrows = _products(got, thick), _want_rows(real, grid, thick)
    assert sorted(rows) == sorted(wrows)
    for k in rows:
        assert numpy.abs(rows[k]).max() > 0, k
        assert numpy.array_equal(rows[k], wrows[k]), k


@pytest.mark.parametrize('resident', [True, False], ids=['hbm', 'host'])
@pytest.mark.parametrize('real', ['float64', 'float32'])
def test_select_of_a_range_without_weights_is_the_range(real, resident):
    """select=range(2, 6) equals steps=(2, 6) bit for bit, with and without the thickness weighting; weights='bounds' takes the
    step lengths of the Field's time object"""
    from nemoflux_amd.timeobj import TimeObj
    grid = GRIDS[1]
    for thick in (False, True):
        f = _source(real, grid, resident, thick)
        a = _products(_quiet(f.timeMean, select=range(2, 6), thicknessWeighted=thick), thick)
        b = _products(_quiet(f.timeMean, (2, 6), thick), thick)
        for k in a:
            assert numpy.abs(a[k]).max() > 0 and numpy.array_equal(a[k], b[k]), (thick, k)
    edges = numpy.concatenate([[0.], numpy.cumsum(smr.MONTHS[:NT])])
    f.timeObj = TimeObj(0.5 * (edges[:-1] + edges[1:]), 'days since 2001-01-01', 'noleap', 'time_counter',
                        bounds=numpy.stack([edges[:-1], edges[1:]], axis=1))
    a = _products(_quiet(f.timeMean, select=SELECT, weights='bounds', thicknessWeighted=True), True)
    b = _products(_quiet(f.timeMean, select=SELECT, weights=WEIGHTS, thicknessWeighted=True), True)
    c = _products(_quiet(f.timeMean, select=SELECT, thicknessWeighted=True), True)
    for k in a:
        assert numpy.array_equal(a[k], b[k]) and not numpy.array_equal(a[k], c[k]), k


class _Ref(ClassRemapReference, DepthRemapReference):
    """the model of tests/resolved_reference.py with the remapped class rows and the depth bins"""


def _reference(f, uv_markers, tracer_markers, class_markers):
    ce, w, sg = f.getWeights()
    return _Ref(ce, w, sg, f.arcLengths, f.thickness, f._tr_off, f.nx, f.ny, uv_markers=uv_markers, tracer_markers=tracer_markers,
                class_markers=class_markers, reference=REF, wrap=True)


def _all_rows(ref, values):
    """(value, sum |terms|) of every product of one state, keyed by (method, carry)"""
    st = ref.step(values, edge_sets=[EDGES])
    rm = ref.remap_step(values, EDGES)
    dp = ref.depth_step(values, DEPTH_EDGES, DEPTH_TOP)
    return {('computeFlux', False): st['volume'], ('computeTracerFlux', False): st['tracer'],
            ('computeFluxProfile', False): st['volume_profile'], ('computeTracerProfile', False): st['tracer_profile'],
            ('computeClassTransport', False): st['volume_classes', 0], ('computeClassTracerTransport', False): st['tracer_classes', 0],
            ('computeClassRemap', False): rm['volume'], ('computeClassRemap', True): rm['carried'],
            ('computeDepthTransport', False): dp['volume'], ('computeDepthTransport', True): dp['carried']}


def _bars(f, real, grid, select, weights, **arrays):
    """per product: BAR x (the smaller of the plain and the weighted mean over the visited steps of sum |terms| of the source
    + sum |terms| of the mean state), on the host from getWeights()"""
    c = dict(_case(real, grid), **arrays)
    src = _reference(f, (FILL, MISSING), (TFILL, TMISSING), (TFILL, TMISSING))
    both = dict(uo=c['uo'], vo=c['vo'], tracer=c['tau'], **{'class': c['sig']})
    steps = [_all_rows(src, array_values(both, t)) for t in select]
    mean_arrays, fills = _mean_arrays(real, grid, select, weights, False, **arrays)
    mean = _all_rows(_reference(f, (fills[0],), (fills[1],), (fills[2],)), array_values(mean_arrays, 0))
    w = numpy.ones(len(select)) if weights is None else numpy.asarray(weights, dtype=numpy.float64)
    bars = {}
    for k in mean:
        mags = numpy.array([s[k][1] for s in steps])
        wmean = numpy.tensordot(w / w.sum(), mags, axes=1)
        bars[k] = BAR * (numpy.minimum(mags.mean(axis=0), wmean) + mean[k][1])
    return bars


@pytest.mark.parametrize('resident', [True, False], ids=['hbm', 'host'])
@pytest.mark.parametrize('grid', GRIDS, ids=lambda g: f'{g[0]}x{g[1]}')
@pytest.mark.parametrize('real', ['float64', 'float32'])
def test_volume_rows_of_the_mean_state_are_the_weighted_mean_of_the_rows(real, grid, resident):
    """missing velocities count as 0 at every step and in the mean, so the volume rows are linear in uo / vo although their
    markers vary in time: the volume row and the profile rows of the mean state are sum w_j rows_j / sum w_j"""
    f = _source(real, grid, resident)
    w = numpy.array(WEIGHTS)
    series = _rows(f.computeAll())[SELECT]
    profiles = numpy.array([_rows(f.computeFluxProfile(t)) for t in SELECT])
    m = _quiet(f.timeMean, select=SELECT, weights=WEIGHTS)
    m.computeFlux(0)
    bars = _bars(f, real, grid, SELECT, WEIGHTS)
    for k, got, rows in ((('computeFlux', False), _row(m), series), (('computeFluxProfile', False), _rows(m.computeFluxProfile(0)), profiles)):
        want = numpy.tensordot(w, rows, axes=1) / w.sum()
        err, bar = numpy.abs(got - want), bars[k]
        print(f'{real} {grid} {k[0]}: max |err| / bar = {float((err / numpy.maximum(bar, 1e-300)).max()):.3g} x 1e-12')
        assert got.shape == want.shape == bar.shape and numpy.abs(want).max() > 0
        assert bar[..., -3:].min() > 0 and numpy.all(err <= bar), k


def test_unselected_steps_of_a_file_backed_source_are_never_read(tmp_path):
    """float32 record variables of NetCDF-3 files, read one step at a time: every variable is wrapped so that read_step of a
    step that is not selected raises; the rows are those of the same arrays in memory"""
    from nemoflux_amd.field import Field
    real, grid = 'float32', GRIDS[1]
    c = _case(real, grid)
    f32 = numpy.float32
    u, v = c['uo'], c['vo']
    g = dict(u=numpy.where(numpy.isnan(u) | (u == f32(MISSING)), f32(FILL), u),
             v=numpy.where((v == f32(FILL)) | (v == f32(MISSING)), f32(numpy.nan), v),
             bounds_lon=c['blon'], bounds_lat=c['blat'], deptht_bounds=DB)
    paths, uf, vf = write_classic_triple(tmp_path, g)
    ff = _quiet(Field, paths['T'], paths['U'], paths['V'], _lines(), readback=False, unsupportedCells='refuse')
    assert ff._lazy is not None
    ff.setTracer((paths['U'], 'uo'), reference=0.5)
    read = []

    class Guarded(object):
        def __init__(self, var):
            self._var, self.dtype, self.shape = var, var.dtype, var.shape

        def read_step(self, t, out=None):
            if t not in SELECT:
                raise AssertionError(f'step {t} is not selected and was read')
            read.append(t)
            return self._var.read_step(t, out=out)

    assert all(hasattr(x, 'read_step') for x in ff._uv) and hasattr(ff._tracer['keep'], 'read_step')
    ff._uv = tuple(Guarded(x) for x in ff._uv)
    ff._tracer['keep'] = Guarded(ff._tracer['keep'])
    a = _quiet(ff.timeMean, select=SELECT, weights=WEIGHTS)
    assert read == SELECT * 3                      # uo, vo and the tracer, each selected step once, in order
    with pytest.raises(AssertionError, match='step 1 is not selected'):
        _quiet(ff.timeMean, select=[0, 1], weights=[1., 2.])
    blon, blat = c['blon'].astype(f32), c['blat'].astype(f32)       # as the T file holds them
    mem = _field(blon, blat, DB.astype(f32), uf, vf, _lines(), readback=False, fill_value=FILL)
    mem.setTracer(uf, fill_value=FILL, reference=0.5)
    b = _quiet(mem.timeMean, select=SELECT, weights=WEIGHTS)
    for f in (a, b):
        f.computeFlux(0)
    assert numpy.abs(_row(b)).max() > 0 and numpy.array_equal(_row(a), _row(b))
    assert numpy.array_equal(_rows(a.computeTracerFlux(0)), _rows(b.computeTracerFlux(0)))
    assert numpy.array_equal(_rows(a.computeFluxProfile(0)), _rows(b.computeFluxProfile(0)))


# ---- 3. Field.meanEddySplit ------------------------------------------------------------------------------------------------
LINEAR = [('computeFluxProfile', False), ('computeClassTransport', False), ('computeClassRemap', False),
          ('computeDepthTransport', False), ('computeTracerProfile', False), ('computeClassTracerTransport', False),
          ('computeClassRemap', True), ('computeDepthTransport', True)]


def _split(f, method, carry, **kw):
    if method in ('computeClassRemap', 'computeDepthTransport'):
        kw['carry'] = carry
    return _quiet(f.meanEddySplit, method, **kw)


@pytest.mark.parametrize('grid', GRIDS, ids=lambda g: f'{g[0]}x{g[1]}')
@pytest.mark.parametrize('real', ['float64', 'float32'])
def test_split_closes_for_the_products_that_are_linear_in_the_velocities(real, grid):
    """a class field and a carried tracer constant in time, velocities that vary (their markers too): the class, remap, depth
    and profile products, volume and carried, are linear in (uo, vo), so eddy is rounding in every value of every row.  With
    a tracer that varies with the velocities the eddy part of computeTracerFlux is at least 1e3 x its bar."""
    c = _case(real, grid)
    const = {k: numpy.ascontiguousarray(numpy.broadcast_to(c[k][1], c[k].shape)) for k in ('tau', 'sig')}
    f = _source(real, grid, True, **const)
    bars = _bars(f, real, grid, SELECT, WEIGHTS, **const)
    for method, carry in LINEAR:
        d = _split(f, method, carry, select=SELECT, weights=WEIGHTS)
        eddy, total, bar = _rows(d['eddy']), _rows(d['total']), bars[method, carry]
        print(f'{real} {grid} {method} carry={carry}: max |eddy| / bar = '
              f'{float((numpy.abs(eddy) / numpy.maximum(bar, 1e-300)).max()):.3g} x 1e-12')
        assert eddy.shape == bar.shape and numpy.abs(total).max() > 0 and bar.max() > 0
        assert numpy.all(numpy.abs(eddy) <= bar), (method, carry)
    d = _split(f, 'computeTracerFlux', False, select=SELECT, weights=WEIGHTS)
    bar = bars['computeTracerFlux', False][-3:]
    assert bar.min() > 0 and numpy.all(numpy.abs(d['eddy'][0]) <= bar)
    g = _source(real, grid, True, tau=c['tau_trend'])
    e = _split(g, 'computeTracerFlux', False, select=SELECT, weights=WEIGHTS)
    gbar = _bars(g, real, grid, SELECT, WEIGHTS, tau=c['tau_trend'])['computeTracerFlux', False][-3:]
    print(f'{real} {grid}: a tracer that varies with the flow, min |eddy| / bar = {float((numpy.abs(e["eddy"][0]) / gbar).min()):.3g}')
    assert gbar.min() > 0 and numpy.all(numpy.abs(e['eddy'][0]) >= 1e3 * gbar), (e['eddy'][0], gbar)


@pytest.mark.parametrize('resident', [True, False], ids=['hbm', 'host'])
def test_split_is_assembled_as_documented(resident):
    """total is the explicit float64 loop over the per-step rows; mean is the product on timeMean(...); eddy their
    difference; with default keywords computeTracerFlux gives meanEddyTracerTransport() bit for bit, and with a selection
    meanEddyTracerTransport is the split reduced to the totals"""
    real, grid = 'float32', GRIDS[1]
    f = _source(real, grid, resident)
    for method, carry in (('computeTracerFlux', False), ('computeClassRemap', True), ('computeGrossProfile', False)):
        kw = dict(carry=carry) if method != 'computeTracerFlux' else {}
        d = _quiet(f.meanEddySplit, method, select=SELECT, weights=WEIGHTS, **kw)
        assert sorted(d) == ['eddy', 'mean', 'meanField', 'total']
        total, wsum = None, 0.0
        for t, w in zip(SELECT, WEIGHTS):
            rows = [w * numpy.asarray(r, dtype=numpy.float64) for r in getattr(f, method)(t, **kw)]
            total = rows if total is None else [a + b for a, b in zip(total, rows)]
            wsum = wsum + w
        total = [a / wsum for a in total]
        mean = getattr(_quiet(f.timeMean, select=SELECT, weights=WEIGHTS), method)(0, **kw)
        for k in range(2):
            assert numpy.abs(total[k]).max() > 0
            assert numpy.array_equal(d['total'][k], total[k]) and numpy.array_equal(d['mean'][k], mean[k]), (method, k)
            assert numpy.array_equal(d['eddy'][k], total[k] - mean[k]), (method, k)
        assert d['meanField'].nt == 1 and numpy.array_equal(getattr(d['meanField'], method)(0, **kw)[0], mean[0])
    for steps in (None, (1, 4)):
        a, b = _quiet(f.meanEddySplit, 'computeTracerFlux', steps), _quiet(f.meanEddyTracerTransport, steps)
        for k in ('total', 'mean', 'eddy'):
            assert b[k].shape == (3,) and numpy.abs(b[k]).min() > 0 and numpy.array_equal(a[k][0], b[k]), (steps, k)
    a = _quiet(f.meanEddySplit, 'computeTracerFlux', select=SELECT, weights=WEIGHTS)
    b = _quiet(f.meanEddyTracerTransport, select=SELECT, weights=WEIGHTS)
    c = _quiet(f.meanEddyTracerTransport)
    for k in ('total', 'mean', 'eddy'):
        assert numpy.array_equal(a[k][0], b[k]) and not numpy.array_equal(b[k], c[k]), k


def test_split_keeps_the_refusals_of_the_products():
    real, grid = 'float64', GRIDS[0]
    f = _source(real, grid, True, thick=True)
    for method, kw in (('computeClassRemap', {}), ('computeClassTransport', {}), ('computeTracerProfile', {}),
                       ('computeClassTracerTransport', {})):
        name = {'computeClassRemap': 'class_remap', 'computeClassTransport': 'class_transport',
                'computeTracerProfile': 'tracer_profile', 'computeClassTracerTransport': 'class_tracer_transport'}[method]
        with pytest.raises(RuntimeError, match=f'nf_field_compute_{name}: this form does not take per-cell thicknesses'):
            _quiet(f.meanEddySplit, method, select=SELECT, weights=WEIGHTS, thicknessWeighted=True, **kw)
    d = _quiet(f.meanEddySplit, 'computeDepthTransport', select=SELECT, weights=WEIGHTS, thicknessWeighted=True, carry=True)
    assert numpy.abs(d['total'][0]).max() > 0 and d['meanField']._e3['nt'] == 1
    with pytest.raises(RuntimeError, match='the mean state of a time-varying cell thickness is not defined here'):
        _quiet(f.meanEddySplit, 'computeDepthTransport', select=SELECT, weights=WEIGHTS)


# ---- 4. the command line ---------------------------------------------------------------------------------------------------
def test_fluxplot_eddy_with_time_weights_and_time_select_writes_the_three_parts(tmp_path):
    from nemoflux_amd import fluxplot
    from nemoflux_amd.field import Field
    real, grid = 'float32', GRIDS[0]
    paths = _write_npz(tmp_path, real, grid)
    lines = "[" + "],[".join(LINES) + "]"
    tr = fluxplot.readTargets(lines)[0]
    f = _quiet(Field, paths['T'], paths['U'], paths['V'], tr, True, readback=False, compact=True)
    f.setTracer((paths['T'], 'tau'), reference=REF)
    d = _quiet(f.meanEddyTracerTransport, select=SELECT, weights=WEIGHTS)
    want = numpy.array([d[k] for k in ('total', 'mean', 'eddy')]) * 2.5
    out = str(tmp_path / 'eddy.csv')
    kw = dict(tFile=paths['T'], uFile=paths['U'], vFile=paths['V'], lonLatPoints=lines, sverdrup=True, tracer='tau',
              tracerRef=REF, tracerScale=2.5, eddy=True, output=out)
    got = _quiet(fluxplot.main, timeSelect='0,2,3,6', timeWeights='31,31,30,31', **kw)
    assert numpy.array_equal(got, want) and numpy.abs(want).min() > 0
    with open(out) as fh:
        text = fh.read().splitlines()
    assert text[0].startswith('# mean transport of tau over 4 time steps, weighted, its mean-flow and eddy parts')
    assert text[1] == 'part,line0,line1,line2' and [ln.split(',')[0] for ln in text[2:]] == ['total', 'mean', 'eddy']
    plain = _quiet(fluxplot.main, **kw)                 # without the options: all steps, as before
    assert plain.shape == got.shape and not numpy.array_equal(plain, got)
    with pytest.raises(RuntimeError, match='4 weights for 7 steps'):
        _quiet(fluxplot.main, timeWeights='31,31,30,31', **kw)
    with pytest.raises(RuntimeError, match='needs a time variable with decodable units'):
        _quiet(fluxplot.main, timeSelect='months:1,2', **kw)
    with pytest.raises(RuntimeError, match="weights='bounds' needs the bounds of the time variable"):
        _quiet(fluxplot.main, timeWeights='bounds', **kw)
