"""Section area and area-weighted tracer with a real column: 363 x 291 (odd, no multiple of 16 or 64) x 75 levels x 2 steps,
periodic with wrapX, the 69 transects of tests/test_gpu_resolved_levels.py, against tests/section_reference.py.  75 levels are
18 chunks of 4 and a ragged one of 3 at float64, 9 chunks of 8 and one of 3 at float32 (the `rows + zc * row_length` offsets of
both blocks, the scratch reused chunk after chunk); segments of more than 256 records beside segments inside one wave.  Both
dtypes, HBM and host inputs, the scalar thickness and a time-varying cell thickness; the other chunk length of each dtype (the
"area_chunk" knob) gives the same bits.  Bar: 1e-12 x sum |terms| per value, every row and column.  Each test prints its worst
|err| / mag (-s); DESIGN.md section 4 quotes them."""
import contextlib

import numpy
import pytest

from gpu_helpers import _rows
from section_reference import SectionReference, array_values
from test_gpu_resolved_levels import (CFILL, CMISSING, FILL, MISSING, NT, NX, NY, NZ, REF, TFILL, THREADS, TMISSING, _data, _make,
                                      _on)

pytestmark = pytest.mark.gpu

BAR = 1e-12
THFILL, THMISSING = -1.e30, 9.e9


def _thickness(real):
    """time-varying e3u, e3v in [0.2, 3] with both markers, NaN and zeros, kept with the data of the dtype"""
    d = _data(real)
    if 'e3u' not in d:
        rng = numpy.random.default_rng(7591)
        dt = numpy.dtype(real).type
        for name in ('e3u', 'e3v'):
            a = rng.uniform(0.2, 3., (NT, NZ, NY, NX)).astype(dt)
            for m, share in ((THFILL, 15), (THMISSING, 17), (numpy.nan, 19), (0., 23)):
                a.reshape(-1)[rng.choice(a.size, a.size // share, replace=False)] = dt(m)
            d[name] = a
    return d


def _area(f, t):
    a, tr = f.computeAreaProfile(t)
    return numpy.stack([_rows(a), _rows(tr)])


@contextlib.contextmanager
def _chunk(levels):
    from nemoflux_amd._lib import lib, check
    check(lib.nf_tuning_set(b'area_chunk', int(levels)))
    try:
        yield
    finally:
        check(lib.nf_tuning_set(b'area_chunk', 0))


@pytest.mark.parametrize('thick', ['scalar', 'cellthick'])
@pytest.mark.parametrize('real,resident', [('float64', True), ('float64', False), ('float32', True), ('float32', False)],
                         ids=['float64-hbm', 'float64-host', 'float32-hbm', 'float32-host'])
def test_area_profile_at_75_levels_against_the_reference(real, resident, thick):
    d = _thickness(real)
    f = _make(real, resident)
    # the scalar form carries the random tracer, the cell-thickness form the class field of that file: +-inf in it, so faces
    # whose value is not finite
    name, marks = ('sig', (TFILL, TMISSING)) if thick == 'cellthick' else ('tau', (CFILL, CMISSING))
    arrays = {'uo': d['uo'], 'vo': d['vo'], 'tracer': d[name]}
    assert thick != 'cellthick' or numpy.isinf(d[name]).any()
    if thick == 'cellthick':
        f.setCellThickness(_on(d, 'e3u', resident), _on(d, 'e3v', resident), fill_value=THFILL, missing_value=THMISSING)
        arrays.update(e3u=d['e3u'], e3v=d['e3v'])
    f.setTracer(_on(d, name, resident), fill_value=marks[0], missing_value=marks[1], reference=REF, wrapX=True)
    ce, w, sg = f.getWeights()
    per_seg = numpy.bincount(sg, minlength=f._nseg) // 4
    assert per_seg.max() > 256 and per_seg.sum() > 500_000
    r = SectionReference(ce, w, sg, f.arcLengths, f.thickness, f._tr_off, NX, NY, uv_markers=(FILL, MISSING),
                         tracer_markers=marks, thick_markers=(THFILL, THMISSING), reference=REF, wrap=True,
                         cell_thickness=thick == 'cellthick')
    tag = f'{real} {"hbm" if resident else "host"} {thick}'
    other = 2 if real == 'float64' else 4          # the candidate that is not the default (4 and 8)
    worst = 0.0
    for t in range(NT):
        want = r.area_step(array_values(arrays, t), threads=THREADS)
        got = _area(f, t)
        assert got.shape == (2, NZ, f._rowlen)
        for k, key in enumerate(('area_profile', 'tracer_area_profile')):
            w_, mag = want[key]
            assert (mag.max(axis=1) > 0).all(), f'{key}: every level must have an area in some column'
            ratio = float((numpy.abs(got[k] - w_) / numpy.maximum(mag, 1e-300)).max())
            worst = max(worst, ratio)
            print(f'{tag} t={t} {key}: max |err| / mag = {ratio:.3g}')
            assert numpy.all(numpy.abs(got[k] - w_) <= BAR * mag), (tag, t, key, ratio)
        assert (got[1] < 0).any() and (got[1] > 0).any()
        with _chunk(other):
            assert numpy.array_equal(_area(f, t), got), (tag, t, 'area_chunk')
    print(f'{tag}: worst |err| / mag = {worst:.3g}')


def test_an_unbuilt_chunk_length_is_refused():
    from nemoflux_amd._lib import lib, NemofluxError
    assert lib.nf_tuning_set(b'area_chunk', 3) == 1
    real = 'float64'
    d = _data(real)
    f = _make(real, True)
    f.setTracer(_on(d, 'tau', True), fill_value=CFILL, missing_value=CMISSING, reference=REF)
    with _chunk(8):                                     # built for float32 only
        with pytest.raises(NemofluxError, match='area_chunk'):
            f.computeAreaProfile(0)
    assert numpy.abs(_area(f, 0)).max() > 0
