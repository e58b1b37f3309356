"""The CPU twin of tests/test_gpu_tracer_planes.py: what that file relies on, checked without a GPU.

1. The index rules of k_tracer_flux (nemoflux_amd/csrc/nf_tracer.hip) restated in numpy -- c0, i0, kend, lane, tid, own_next,
   north_all, has_n, cwrap, ntiles, the XCD band of a tile -- and, for every shape and dtype of the GPU test, the launch form
   (VEC, NAL, tiles, grid) and the set of neighbour situations that one launch holds, pinned to what was worked out when the
   shapes were chosen.  A re-tuned tile size or vector width makes this file fail instead of silently emptying the GPU test.
   (The launcher also wants 16-byte aligned fields; device and pinned allocations are, and with ncell % VEC == 0 so is every
   level and step of them.)
2. The probe condition of tests/tracer_probe.py on the CPU oracle's weights of the probe lines, for every shape.
3. The inputs: at least 99 % of the segments carry flux in the reference (mag > 0), and the rim faces -- the wrap faces of
   column nx - 1, the faces below the last row, the last row's own north faces -- come with both, one and no side present.
4. The reference's summed tracer rows on the probe (7 x 128) against a naive math.fsum loop, at 4 eps x mag.

Why these shapes (cells are counted flat, a lane owns VEC cells, 64 lanes a wavefront, 256 a tile):
    7 x 128    896 cells: float64 takes VEC = 2 with an unaligned north stream, 2 tiles; the smallest grid at which one launch
               has a row end at lane position 0 and 1, each in an inner lane and in lane 63, lane 63 without a row end,
               thread 255 taking its east neighbour from the next workgroup, a row end in the last lane of a tile, the lanes
               that straddle the start of the last row, and a last lane that is lane 63
    11 x 256   2816 cells: the same for float32 (VEC = 4, positions 0 .. 3), 3 tiles
    129 x 64   8256 cells, 17 / 9 tiles in 24 / 16 workgroups: the XCD map is no identity, dead workgroups sit between live ones,
               row ends and wrap sources lie in other tiles and other bands; VEC > 1 and unaligned in both dtypes
    61 x 35    odd: one cell per lane, 9 tiles, so that form meets bands too
    128 x 34   the aligned north load (nx % VEC == 0) with VEC > 1 and several tiles
"""
import math

import numpy
import pytest

from resolved_reference import ResolvedReference, array_values
from gross_reference import THFILL, THMISSING
from tracer_probe import (FILL, MISSING, NT, NZ, REALS, REFERENCE, SHAPES, TFILL, TMISSING, face_presence, probe_box,
                          probe_condition, probe_inputs, probe_lines, probe_thickness, shape_id)

EPS = numpy.finfo(numpy.float64).eps
TILE, WAVE, XCDS = 256, 64, 8            # threads per workgroup, lanes per wavefront, kXcds


# ---- 1. the index rules ------------------------------------------------------------------------------------------------------
def launch_form(nx, ny, real):
    """(VEC, NAL, ntiles, workgroups) of launch_tracer_flux for 16-byte aligned fields"""
    ncell = nx * ny
    vec = 16 // numpy.dtype(real).itemsize
    if not (ncell % vec == 0 and nx >= vec):
        vec = 1
    per_tile = TILE * vec
    ntiles = (ncell + per_tile - 1) // per_tile
    return vec, nx % vec == 0, ntiles, (ntiles + XCDS - 1) // XCDS * XCDS


def situations(nx, ny, vec):
    """the neighbour situations that the lanes of one launch are in, by name"""
    ncell = nx * ny
    per_tile = TILE * vec
    ntiles = (ncell + per_tile - 1) // per_tile
    grid = (ntiles + XCDS - 1) // XCDS * XCDS
    band = grid // XCDS                                     # xcd_tile: workgroup b runs tile (b % 8) * band + b // 8
    g = numpy.arange(ntiles * TILE, dtype=numpy.int64)      # tile * 256 + tid
    tile, tid = g // TILE, g % TILE
    lane = tid & (WAVE - 1)
    c0 = g * vec
    on = c0 < ncell
    cs = numpy.where(on, c0, 0)
    i0 = cs % nx
    kend = numpy.where(nx - 1 - i0 < vec, nx - 1 - i0, -1)
    cwrap = cs + kend + 1 - nx
    own_next = on & (lane == WAVE - 1) & (kend != vec - 1) & (c0 + vec < ncell)
    north_all = on & (c0 + vec - 1 + nx < ncell)
    has_n = on[:, None] & (c0[:, None] + numpy.arange(vec)[None, :] + nx < ncell)
    assert numpy.array_equal(north_all, has_n.all(axis=1))
    # what the rules promise: a lane's cells hold at most one row end, and every address lies inside the level
    assert ((cwrap >= 0) | (kend < 0)).all() and (cwrap[kend >= 0] % nx == 0).all()
    assert (c0[own_next] + vec < ncell).all() and (c0[north_all] + vec - 1 + nx < ncell).all()
    out = set()
    for k in range(vec):
        if (on & (kend == k) & (lane < WAVE - 1)).any():
            out.add(f'row end at position {k}, inner lane')
        sel = on & (kend == k) & (lane == WAVE - 1)
        if sel.any():
            out.add(f'row end at position {k}, lane 63')
            # the lane's last cell needs its east neighbour from the next lane unless it is the row end itself
            assert (own_next[sel] == (k < vec - 1)).all() or not (c0[sel] + vec < ncell).all()
    if (own_next & (kend == -1)).any():
        out.add('lane 63 without a row end')
    if (own_next & (tid == TILE - 1)).any():
        out.add('thread 255 reads the next workgroup')
    if (on & (tid == TILE - 1) & (kend >= 0)).any():
        out.add('row end in the last lane of a tile')
    if (on & ~north_all & has_n.any(axis=1)).any():
        out.add('lanes straddle the start of the last row')
    if g[on][-1] % WAVE == WAVE - 1:
        out.add('the last lane is lane 63')
    src = kend >= 0
    if (src & (cwrap // (vec * WAVE) != c0 // (vec * WAVE))).any():
        out.add('wrap source in another wavefront')
    if (src & (cwrap // per_tile != tile)).any():
        out.add('wrap source in another tile')
    if band > 1 and (src & (cwrap // per_tile // band != tile // band)).any():
        out.add('wrap source in another band')
    if band > 1 and (own_next & (tid == TILE - 1) & ((tile + 1) // band != tile // band)).any():
        out.add('thread 255 reads another band')
    b = numpy.arange(grid)
    tile_of = (b % XCDS) * band + b // XCDS
    assert sorted(tile_of.tolist()) == list(range(grid))
    if (tile_of != b).any():
        out.add('the XCD map is no identity')
    live = numpy.flatnonzero(tile_of < ntiles)
    if (tile_of[live[0]:live[-1] + 1] >= ntiles).any():
        out.add('dead workgroups between live ones')
    return out


def _row_ends(vec, lane63=True):
    where = ('inner lane', 'lane 63') if lane63 else ('inner lane',)
    return {f'row end at position {k}, {w}' for k in range(vec) for w in where}


NEXT = {'lane 63 without a row end', 'thread 255 reads the next workgroup', 'wrap source in another wavefront'}
TILE_END = {'row end in the last lane of a tile'}
LAST_ROW = {'lanes straddle the start of the last row'}
LAST_63 = {'the last lane is lane 63'}
OTHER_TILE = {'wrap source in another tile'}
BANDS = OTHER_TILE | {'wrap source in another band', 'thread 255 reads another band', 'the XCD map is no identity',
                      'dead workgroups between live ones'}
# everything at once, as the two narrow shapes were chosen to have it
NARROW = NEXT | TILE_END | LAST_ROW | LAST_63 | OTHER_TILE

# (nx, ny), dtype -> ((VEC, NAL, tiles, workgroups), the situations of one launch: all of them, and no other)
CLAIMS = {
    ((7, 128), 'float64'): ((2, False, 2, 8), _row_ends(2) | NARROW),
    # one tile of 224 lanes: no tile seam, and of the row ends only position 2 meets lane 63
    ((7, 128), 'float32'): ((4, False, 1, 8), _row_ends(4, lane63=False) | LAST_ROW | {
        'row end at position 2, lane 63', 'lane 63 without a row end', 'wrap source in another wavefront'}),
    ((11, 256), 'float64'): ((2, False, 6, 8), _row_ends(2) | NARROW),
    ((11, 256), 'float32'): ((4, False, 3, 8), _row_ends(4) | NARROW),
    # row r ends in lane r // 2 (r // 4) of its wavefront: never lane 63, which the narrow shapes supply
    ((129, 64), 'float64'): ((2, False, 17, 24), _row_ends(2, lane63=False) | NEXT | LAST_ROW | BANDS),
    ((129, 64), 'float32'): ((4, False, 9, 16), _row_ends(4, lane63=False) | NEXT | LAST_ROW | BANDS),
    ((61, 35), 'float64'): ((1, True, 9, 16), _row_ends(1, lane63=False) | NEXT | BANDS),
    ((61, 35), 'float32'): ((1, True, 9, 16), _row_ends(1, lane63=False) | NEXT | BANDS),
    # a row is one wavefront (half of one): every row end is the lane's last cell, the next lane is never read past a wave
    ((128, 34), 'float64'): ((2, True, 9, 16), {'row end at position 1, lane 63', 'the XCD map is no identity',
                                                 'dead workgroups between live ones'} | TILE_END | LAST_63),
    ((128, 34), 'float32'): ((4, True, 5, 8), {'row end at position 3, inner lane', 'row end at position 3, lane 63'}
                             | TILE_END | LAST_63),
}


@pytest.mark.parametrize('real', REALS)
@pytest.mark.parametrize('grid', SHAPES, ids=shape_id)
def test_launch_form_and_situations_are_the_claimed_ones(grid, real):
    form, claimed = CLAIMS[grid, real]
    nx, ny = grid
    assert launch_form(nx, ny, real) == form
    found = situations(nx, ny, form[0])
    assert found == claimed, (sorted(claimed - found), sorted(found - claimed))


def test_the_narrow_shapes_hold_every_seam_situation_at_once():
    """7 x 128 at float64 and 11 x 256 at float32: a row end at every lane position, in an inner lane and in lane 63; lane 63
    without one; thread 255 reading the next workgroup; a row end in the last lane of a tile; the straddled last row; a last
    lane that is lane 63"""
    for grid, real, vec in (((7, 128), 'float64', 2), ((11, 256), 'float32', 4)):
        assert launch_form(*grid, real)[:2] == (vec, False)
        assert _row_ends(vec) | NARROW <= situations(*grid, vec)


def test_every_gpu_case_is_claimed():
    assert sorted(CLAIMS) == sorted((g, r) for g in SHAPES for r in REALS)


# ---- 2., 3. the probe on the oracle's weights, and the inputs --------------------------------------------------------------
_PROBES = {}


def _probe(oracle, nx, ny):
    """weights of the probe lines from the CPU oracle: (cell_slot, weight, segment, coverage, arc, tr_off)"""
    if (nx, ny) not in _PROBES:
        x0, x1, y0, y1 = probe_box(nx, ny)
        o = oracle.DataGen(nx, ny, NZ, NT, x0, x1, y0, y1, lat_uses_dx=False)
        pts = oracle.assemble_points(o.bounds_lon, o.bounds_lat)
        ws = [oracle.polyline_weights(pts, xyz, periodX=0.) for xyz in probe_lines(nx, ny)]
        tr_off = numpy.concatenate([[0], numpy.cumsum([w.nseg for w in ws])])
        _PROBES[nx, ny] = (numpy.concatenate([w.cell_edge for w in ws]), numpy.concatenate([w.weight for w in ws]),
                           numpy.concatenate([w.seg + tr_off[p] for p, w in enumerate(ws)]), [w.coverage for w in ws],
                           oracle.arc_lengths(pts), tr_off)
    return _PROBES[nx, ny]


@pytest.mark.parametrize('grid', SHAPES, ids=shape_id)
def test_probe_condition_holds_on_the_oracle_weights(oracle, grid):
    nx, ny = grid
    ce, w, sg, cov, arc, tr_off = _probe(oracle, nx, ny)
    assert tr_off[-1] == ny * (nx - 1)
    for wrap in (True, False):
        assert probe_condition(ce, w, cov, nx, ny, wrap) == []
    # the condition bites: without the last column's own pieces its wrap faces are not carried
    keep = (ce // 4) % nx != nx - 1
    assert probe_condition(ce[keep], w[keep], cov, nx, ny, True) != []


@pytest.mark.parametrize('real', REALS)
@pytest.mark.parametrize('grid', SHAPES, ids=shape_id)
def test_inputs_carry_flux_and_every_kind_of_rim_face(oracle, grid, real):
    nx, ny = grid
    ce, w, sg, cov, arc, tr_off = _probe(oracle, nx, ny)
    u, v, tau = probe_inputs(real, nx, ny)
    east, below, last = face_presence(tau, nx, ny, True)
    assert set(numpy.unique(east)) == {0, 1, 2} and set(numpy.unique(below)) == {0, 1, 2} and set(numpy.unique(last)) == {0, 1}
    assert set(numpy.unique(face_presence(tau, nx, ny, False)[0])) == {0, 1}
    e3u, e3v = probe_thickness(real, nx, ny, NT if grid == (11, 256) else 1)
    arrays = {'uo': u, 'vo': v, 'tracer': tau, 'e3u': e3u, 'e3v': e3v}
    for e3 in (e3u, e3v):
        ok = ~numpy.isnan(e3)
        assert (e3 == 0).any() and (e3 == e3.dtype.type(THFILL)).any() and (e3 == e3.dtype.type(THMISSING)).any() and not ok.all()
    th = numpy.full(NZ, 1. / NZ)
    for wrap in (True, False):
        for cell in (False, True):
            ref = ResolvedReference(ce, w, sg, arc, th, tr_off, nx, ny, uv_markers=(FILL, MISSING),
                                    tracer_markers=(TFILL, TMISSING), thick_markers=(THFILL, THMISSING), reference=REFERENCE,
                                    wrap=wrap, cell_thickness=cell)
            for t in range(NT):
                got = ref.step(array_values(arrays, t))
                mag, pmag = got['tracer'][1][:ref.nseg], got['tracer_profile'][1][:, :ref.nseg]
                assert (mag > 0).mean() >= 0.99 and (pmag > 0).mean() >= 0.99, (wrap, cell, t)
                assert (got['tracer'][1][ref.nseg:] > 0).all() and (got['tracer_profile'][1][:, ref.nseg:] > 0).all()


# ---- 4. the reference on the probe against a naive loop ---------------------------------------------------------------------
def _naive_tracer_rows(ce, w, sg, arc, th, tr_off, nx, ny, u, v, tau, t, wrap, sverdrup):
    """every value of the tracer row as math.fsum of its terms, one (entry, level) at a time, Python scalars"""
    dt = tau.dtype.type
    nseg, ntr = int(tr_off[-1]), len(tr_off) - 1
    tr_of = numpy.searchsorted(tr_off, numpy.arange(nseg), side='right') - 1

    def present(x, marks):
        return not math.isnan(x) and all(x != dt(m) for m in marks)

    terms = [[] for _ in range(nseg + ntr)]
    for e in range(len(ce)):
        c, slot, s = int(ce[e]) // 4, int(ce[e]) % 4, int(sg[e])
        j, i = divmod(c, nx)
        if slot == 0:
            if j == 0:
                continue
            ca, cb = c - nx, c
        elif slot == 1:
            ca, cb = c, (c + 1 if i < nx - 1 else (c + 1 - nx if wrap else None))
        elif slot == 2:
            ca, cb = c, (c + nx if j < ny - 1 else None)
        else:
            ca = c - 1 if i > 0 else c - 1 + nx
            cb = c if (i > 0 or wrap) else None
        for z in range(NZ):
            x = (u if slot in (1, 3) else v)[t, z].reshape(-1)[ca]
            vel = float(x) if present(x, (FILL, MISSING)) else 0.0
            flat = tau[t, z].reshape(-1)
            pa = present(flat[ca], (TFILL, TMISSING))
            pb = cb is not None and present(flat[cb], (TFILL, TMISSING))
            if pa and pb:
                tf = 0.5 * (float(flat[ca]) + float(flat[cb])) - REFERENCE
            elif pa or pb:
                tf = float(flat[ca] if pa else flat[cb]) - REFERENCE
            else:
                tf = 0.0
            al = float(arc[ca, 1]) if slot in (1, 3) else -float(arc[ca, 2])
            d = (float(th[z]) * (vel * tf)) * al
            if sverdrup:
                d = d * (6371000.0 / 1.e6)
            for col in (s, nseg + int(tr_of[s])):
                terms[col].append(float(w[e]) * d)
    return (numpy.array([math.fsum(x) for x in terms]), numpy.array([math.fsum(abs(y) for y in x) for x in terms]))


@pytest.mark.parametrize('wrap', [True, False], ids=['wrap', 'nowrap'])
@pytest.mark.parametrize('real', REALS)
def test_reference_rows_on_the_probe_are_the_naive_loop(oracle, real, wrap):
    nx, ny = 7, 128
    ce, w, sg, cov, arc, tr_off = _probe(oracle, nx, ny)
    u, v, tau = probe_inputs(real, nx, ny)
    th = numpy.array([0.5, 0.25, 2.0, 0.125, 1.5])
    sverdrup = real == 'float32'
    ref = ResolvedReference(ce, w, sg, arc, th, tr_off, nx, ny, uv_markers=(FILL, MISSING), tracer_markers=(TFILL, TMISSING),
                            reference=REFERENCE, wrap=wrap, sverdrup=sverdrup)
    for t in range(NT):
        got, gmag = ref.step(array_values({'uo': u, 'vo': v, 'tracer': tau}, t))['tracer']
        want, mag = _naive_tracer_rows(ce, w, sg, arc, th, tr_off, nx, ny, u, v, tau, t, wrap, sverdrup)
        assert got.shape == want.shape == (ny * (nx - 1) + ny,) and mag.max() > 0
        assert numpy.all(numpy.abs(got - want) <= 4 * EPS * mag), (t, float((numpy.abs(got - want) / numpy.maximum(mag, 1e-300)).max()))
        assert numpy.all(numpy.abs(gmag - mag) <= 4 * EPS * mag), t
