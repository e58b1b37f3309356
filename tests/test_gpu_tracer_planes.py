"""Every face of K1tau (k_tracer_flux, nemoflux_amd/csrc/nf_tracer.hip) and of the per-record tracer gathers against the
reference model, through the dense probe of tests/tracer_probe.py: one zig-zag transect per grid row, so that every east and
every north face of the grid -- wrap faces and the neighbourless north faces of the last row included -- has a weight of at
least 0.05 in some per-segment value.  The older tracer tests see the planes only where three lines pass.

The shapes put a row end at every position of a lane, in inner lanes and in lane 63 of a wavefront, at tile seams, across XCD
bands, and take every launch form (VEC 1 / 2 / 4, north stream aligned or not, per-level or per-cell thickness with one full
and one short level batch each); tests/test_tracer_planes_cpu.py states the index rules and pins what each shape reaches.

Bar: 1e-12 x sum |terms| of every single value (the project's bar for tree against sequential summation and fma against
separate rounding), on the `mag` of tests/resolved_reference.py; no segment is left out.  Each test prints its worst
|err| / mag (-s); the docstrings of the tests carry what was measured on an MI355X."""
import numpy
import pytest

from gpu_helpers import _field, _on, _rows
from gross_reference import THFILL, THMISSING
from resolved_reference import ResolvedReference, array_values
from tracer_probe import (FILL, MISSING, NT, NZ, REALS, REFERENCE, SHAPES, TFILL, TMISSING, probe_box, probe_condition,
                          probe_inputs, probe_lines, probe_thickness, shape_id)

pytestmark = pytest.mark.gpu

BAR = 1e-12
TIME_VARYING = (11, 256)                 # the shape whose cell thickness changes from step to step; static on the others
TIE_SHAPES = [(7, 128), (129, 64)]       # one narrow and the wide shape
GATHER_SHAPES = [(11, 256), (129, 64)]
THICK = ['scalar', 'cell']


def _sverdrup(real, wrap):
    return real == 'float32' and wrap    # once per shape and thickness form


_GRIDS, _INPUTS, _WANT = {}, {}, {}


def _grid(real, nx, ny):
    if (real, nx, ny) not in _GRIDS:
        from nemoflux_amd.datagen import DataGen
        dg = DataGen(real=real)
        dg.setSizes(nx, ny, NZ, NT)
        dg.setBoundingBox(*probe_box(nx, ny), 0., 1.)
        dg.build()
        _GRIDS[real, nx, ny] = (dg.bounds_lon.cpu().numpy(), dg.bounds_lat.cpu().numpy(), dg.deptht_bounds)
    return _GRIDS[real, nx, ny]


def _inputs(real, nx, ny):
    """host arrays {'uo', 'vo', 'tracer', 'e3u', 'e3v'} of the shape, made once and left unchanged"""
    if (real, nx, ny) not in _INPUTS:
        u, v, tau = probe_inputs(real, nx, ny)
        e3u, e3v = probe_thickness(real, nx, ny, NT if (nx, ny) == TIME_VARYING else 1)
        _INPUTS[real, nx, ny] = {'uo': u, 'vo': v, 'tracer': tau, 'e3u': e3u, 'e3v': e3v}
    return _INPUTS[real, nx, ny]


def _make(real, grid, wrap, thick, resident=True, tau=None):
    nx, ny = grid
    a = _inputs(real, nx, ny)
    f = _field(*_grid(real, nx, ny), _on(a['uo'], resident), _on(a['vo'], resident), probe_lines(nx, ny),
               sverdrup=_sverdrup(real, wrap), readback=False, fill_value=FILL, missing_value=MISSING, periodX=0.)
    if thick == 'cell':
        f.setCellThickness(_on(a['e3u'], resident), _on(a['e3v'], resident), fill_value=THFILL, missing_value=THMISSING)
    f.setTracer(_on(a['tracer'] if tau is None else tau, resident), fill_value=TFILL, missing_value=TMISSING,
                reference=REFERENCE, wrapX=wrap)
    return f


def _reference(f, real, grid, wrap, thick):
    """the reference's step dicts [t] for the weights of f, computed once per case; the probe condition is asserted on the way"""
    key = (real, grid, wrap, thick)
    nx, ny = grid
    ce, w, sg = f.getWeights()
    if key not in _WANT:
        assert probe_condition(ce, w, f.getCoverage(), nx, ny, wrap) == []
        ref = ResolvedReference(ce, w, sg, f.arcLengths, f.thickness, f._tr_off, nx, ny, uv_markers=(FILL, MISSING),
                                tracer_markers=(TFILL, TMISSING), thick_markers=(THFILL, THMISSING), reference=REFERENCE,
                                wrap=wrap, sverdrup=_sverdrup(real, wrap), cell_thickness=thick == 'cell')
        a = _inputs(real, nx, ny)
        _WANT[key] = ((ce, w, sg), [ref.step(array_values(a, t)) for t in range(NT)])
    assert all(numpy.array_equal(x, y) for x, y in zip(_WANT[key][0], (ce, w, sg)))
    return _WANT[key][1]


def _check(label, got, pair):
    """every value within BAR x its own mag; returns the worst |err| / mag"""
    want, mag = pair
    assert got.shape == want.shape == mag.shape, label
    err = numpy.abs(got - want)
    ratio = float((err / numpy.maximum(mag, 1e-300)).max())
    print(f'{label}: max |err| / mag = {ratio:.3g}')
    bad = numpy.argwhere(~(err <= BAR * mag))
    assert bad.size == 0, (label, ratio, len(bad), bad[:8].tolist())
    return ratio


def _id(real, grid, wrap, thick):
    return f'{real} {shape_id(grid)} {"wrap" if wrap else "nowrap"} {thick}'


# ---- every face of K1tau ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('thick', THICK)
@pytest.mark.parametrize('wrap', [True, False], ids=['wrap', 'nowrap'])
@pytest.mark.parametrize('grid', SHAPES, ids=shape_id)
@pytest.mark.parametrize('real', REALS)
def test_every_face_against_the_reference(real, grid, wrap, thick):
    """computeTracerFlux, every per-segment value and every transect total of every step, and computeTracerAll.
    Measured on an MI355X: worst |err| / mag 3.4e-16 with the per-level thickness, 3.6e-16 with the per-cell one."""
    f = _make(real, grid, wrap, thick)
    want = _reference(f, real, grid, wrap, thick)
    nseg = f._nseg
    assert nseg == grid[1] * (grid[0] - 1) and f._rowlen == nseg + grid[1]
    allrows = _rows(f.computeTracerAll())
    for t in (1, 0):
        mag = want[t]['tracer'][1]
        assert (mag[:nseg] > 0).mean() >= 0.99 and (mag[nseg:] > 0).all()
        got = _rows(f.computeTracerFlux(t))
        _check(f'{_id(real, grid, wrap, thick)} t={t} tracer row', got, want[t]['tracer'])
        assert numpy.array_equal(allrows[t], got), t


# ---- exact ties ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('thick', THICK)
@pytest.mark.parametrize('wrap', [True, False], ids=['wrap', 'nowrap'])
@pytest.mark.parametrize('grid', TIE_SHAPES, ids=shape_id)
@pytest.mark.parametrize('real', REALS)
def test_unit_tracer_gives_the_volume_rows_on_the_probe(real, grid, wrap, thick):
    """tau == reference + 1 makes every face value exactly 1: the tracer rows are the computeFlux rows of the same thickness
    form bit for bit, per step and for all steps"""
    nx, ny = grid
    tau = numpy.full((NT, NZ, ny, nx), REFERENCE + 1., dtype=real)
    f = _make(real, grid, wrap, thick, tau=tau)
    for t in (1, 0):
        got = _rows(f.computeTracerFlux(t))
        f.computeFlux(t)
        want = numpy.array(f._row[:f._rowlen])
        assert (want[:f._nseg] != 0).mean() >= 0.99
        assert numpy.array_equal(got, want), t
    assert numpy.array_equal(_rows(f.computeTracerAll()), _rows(f.computeAll()))


@pytest.mark.parametrize('thick', THICK)
@pytest.mark.parametrize('grid', TIE_SHAPES, ids=shape_id)
@pytest.mark.parametrize('real', REALS)
def test_host_inputs_give_the_bits_of_hbm_inputs(real, grid, thick):
    hbm, host = _make(real, grid, True, thick), _make(real, grid, True, thick, resident=False)
    for t in (1, 0):
        a = _rows(hbm.computeTracerFlux(t))
        assert (a[:hbm._nseg] != 0).mean() >= 0.99
        assert numpy.array_equal(a, _rows(host.computeTracerFlux(t))), t
    assert numpy.array_equal(_rows(hbm.computeTracerAll()), _rows(host.computeTracerAll()))


# ---- the per-record tracer gathers -----------------------------------------------------------------------------------------
@pytest.mark.parametrize('thick', THICK)
@pytest.mark.parametrize('wrap', [True, False], ids=['wrap', 'nowrap'])
@pytest.mark.parametrize('grid', GATHER_SHAPES, ids=shape_id)
@pytest.mark.parametrize('real', REALS)
def test_tracer_profile_against_the_reference(real, grid, wrap, thick):
    """the per-level tracer rows, which gather the second cell of every face per record: a record sits on the last column, on
    the last row and on column 0's west slot of every row.  With the per-level thickness computeTracerProfile; that call
    refuses a cell thickness, and the per-record form that takes one is the carried gross profile, whose P + N is the same
    row (one more rounding of |P| + |N| <= mag).  Their sum over z is the K1tau row within the bar on sum |terms|.
    Measured on an MI355X: worst |err| / mag 3.7e-16 (computeTracerProfile), 3.8e-16 (P + N with a cell thickness)."""
    f = _make(real, grid, wrap, thick)
    want = _reference(f, real, grid, wrap, thick)
    for t in (1, 0):
        if thick == 'cell':
            parts = _rows(f.computeGrossProfile(t, carry=True))
            assert parts.shape == (2, NZ, f._rowlen)
            prof = parts[0] + parts[1]
        else:
            prof = _rows(f.computeTracerProfile(t))
        pwant, pmag = want[t]['tracer_profile']
        assert (pmag[:, :f._nseg] > 0).mean() >= 0.99 and (pmag[:, f._nseg:] > 0).all()
        _check(f'{_id(real, grid, wrap, thick)} t={t} tracer profile', prof, (pwant, pmag))
        row = _rows(f.computeTracerFlux(t))
        assert numpy.all(numpy.abs(prof.sum(axis=0) - row) <= BAR * pmag.sum(axis=0)), t
