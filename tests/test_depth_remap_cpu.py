"""Transports in true-depth bins (nf_field_compute_depth_transport, Field.computeDepthTransport, fluxplot --depth-bins), the
part that needs no GPU: the reference of tests/depth_remap_reference.py pinned to a naive scalar loop with math.fsum at
4 eps x sum |share| per value, on a 12 x 9 x 3 case with land, both markers, NaN and exact zeros in the velocities and the
thicknesses, in both forms (volume, carried tracer), with the scalar, a static and a time-varying thickness, with `top` 0 and
-1.5, and for a rank's slab; the fractions of every spread term add up to 1 within 4 eps; the rows add up to the profile rows;
the fallbacks one by one; the conditions on the inputs of tests/test_gpu_depth_remap.py -- terms spread over more than one row,
terms with lo == hi and interface depths exactly on an edge all occur; the Field methods; the fluxplot argument checks."""
import math
import subprocess
import sys

import numpy
import pytest

from class_remap_reference import shares
from conftest import ROOT, transect_xyz
from depth_remap_reference import EDGES as GPU_EDGES, GPU_E3_SEED, GPU_TH, DepthRemapReference, depth_intervals, depth_thickness
from gross_reference import FILL, MISSING, THFILL, THMISSING, array_values, gross_velocities
from test_class_remap_cpu import _tracer
from test_gross_cpu import GPU_GRIDS, GPU_NT, GPU_NZ, GPU_UV_SEED, LINES, NT, NX, NY, NZ, REF, TFILL, TH, TMISSING, _weights  # noqa: F401

EPS = numpy.finfo(numpy.float64).eps
SV = 6371000.0 / 1.e6
EDGES = numpy.array([0.25, 0.5, 1., 2.75, 4., 6.5, 9.])
# the three transects of tests/test_gpu_class_remap.py
GPU_LINES = ["(-100,-80),(100,-80),(0,80)", "(-100,-80),(100,-80),(0,80),(-100,-80)", "(150,-30),(179.5,-20),(179.9,10),(175,40)"]


def _naive(ce, w, sg, arc, tr_off, a, t, edges, top, cell_thickness, levels):
    """the rows of both forms as math.fsum of their shares, one (entry, level, row) at a time from the full arrays; also the
    largest |sum of the fractions of a spread term - 1|"""
    dt = a['uo'].dtype.type
    nseg, ntr = int(tr_off[-1]), len(tr_off) - 1
    tr_of = [p for p in range(ntr) for _ in range(tr_off[p], tr_off[p + 1])]
    n = len(edges)
    nz = a['uo'].shape[1]

    def present(x, marks):
        return not math.isnan(x) and all(x != dt(m) for m in marks)

    def val(name, z, c):
        arr = a[name]
        return arr[t if arr.shape[0] > 1 else 0, z].reshape(-1)[c]

    def face(name, z, ca, cb, marks):
        xa = val(name, z, ca)
        pa = present(xa, marks)
        pb = cb is not None and present(val(name, z, cb), marks)
        if pa and pb:
            return True, 0.5 * (float(xa) + float(val(name, z, cb)))
        if pa:
            return True, float(xa)
        if pb:
            return True, float(val(name, z, cb))
        return False, 0.0

    def row(x):
        return sum(1 for ed in edges if ed <= x)

    def fractions(d0, d1):
        """[(row, fraction or None for the whole term)]"""
        if not (math.isfinite(d0) and math.isfinite(d1) and math.isfinite(d1 - d0)):
            return [(n + 1, None)]
        lo, hi = min(d0, d1), max(d0, d1)
        if lo == hi:
            return [(row(lo), None)]
        out = []
        for j in range(row(lo), row(hi) + 1):
            left = lo if j == row(lo) else float(edges[j - 1])
            right = hi if j == row(hi) else float(edges[j])
            if right != left:
                out.append((j, (right - left) / (hi - lo)))
        return out

    terms = {'volume': {}, 'carried': {}}
    worst = 0.0
    for e in range(len(ce)):
        c, slot, s = int(ce[e]) // 4, int(ce[e]) % 4, int(sg[e])
        j, i = divmod(c, NX)
        if slot == 0:
            if j == 0:
                continue
            ca, cb = c - NX, c
        elif slot == 1:
            ca, cb = c, (c + 1 if i < NX - 1 else c + 1 - NX)
        elif slot == 2:
            ca, cb = c, (c + NX if j < NY - 1 else None)
        else:
            ca, cb = (c - 1 if i > 0 else c - 1 + NX), c
        east = slot in (1, 3)
        depth = float(top)
        for z in range(nz):
            if cell_thickness:
                h = val('e3u' if east else 'e3v', z, ca)
                h = float(h) if present(h, (THFILL, THMISSING)) else 0.0
            else:
                h = float(TH[z])
            d0, depth = depth, depth + h
            if not levels[0] <= z < levels[1]:
                continue
            x = val('uo' if east else 'vo', z, ca)
            vel = float(x) if present(x, (FILL, MISSING)) else 0.0
            has_t, xt = face('tracer', z, ca, cb, (TFILL, TMISSING))
            tf = xt - REF if has_t else 0.0
            al = float(arc[ca, 1]) if east else -float(arc[ca, 2])
            q = float(w[e]) * (((h * vel) * al) * SV)
            cc = float(w[e]) * (((h * (vel * tf)) * al) * SV)
            fr = fractions(d0, depth)
            if fr[0][1] is not None:
                worst = max(worst, abs(math.fsum(x for _, x in fr) - 1.0))
            for r, x in fr:
                for col in (s, nseg + tr_of[s]):
                    terms['volume'].setdefault((r, col), []).append(q if x is None else q * x)
                    terms['carried'].setdefault((r, col), []).append(cc if x is None else cc * x)
    out = {'fraction_error': worst}
    for nm in terms:
        want, mag = numpy.zeros((n + 2, nseg + ntr)), numpy.zeros((n + 2, nseg + ntr))
        for idx, xs in terms[nm].items():
            want[idx], mag[idx] = math.fsum(xs), math.fsum(abs(x) for x in xs)
        out[nm] = (want, mag)
    return out


@pytest.mark.parametrize('top', [0.0, -1.5])
@pytest.mark.parametrize('thick', ['scalar', 'static', 'timevarying'])
@pytest.mark.parametrize('real', ['float64', 'float32'])
def test_reference_is_the_naive_loop(oracle, real, thick, top):
    ce, wt, sg, arc, tr_off = _weights(oracle)
    shape = (NT, NZ, NY, NX)
    u, v = gross_velocities(real, shape, seed=5)
    arrays = {'uo': u, 'vo': v, 'tracer': _tracer(real, shape, 7)}
    cell = thick != 'scalar'
    if cell:
        arrays['e3u'], arrays['e3v'] = depth_thickness(real, (NT if thick == 'timevarying' else 1, NZ, NY, NX), seed=9)
        dt = numpy.dtype(real).type
        for a in (arrays['e3u'], arrays['e3v']):
            assert numpy.isnan(a).any() and (a == 0).any() and (a == dt(THFILL)).any() and (a == dt(THMISSING)).any()
            assert not numpy.isinf(a).any()
    kw = dict(uv_markers=(FILL, MISSING), tracer_markers=(TFILL, TMISSING), thick_markers=(THFILL, THMISSING), reference=REF,
              wrap=True, sverdrup=True)
    ref = DepthRemapReference(ce, wt, sg, arc, TH, tr_off, NX, NY, cell_thickness=cell, **kw)
    seen = numpy.zeros(EDGES.size + 2, bool)
    for t in range(NT):
        for levels in ((0, NZ), (1, NZ), (0, 2)):
            got = ref.depth_step(array_values(arrays, t), EDGES, top=top, levels=levels)
            want = _naive(ce, wt, sg, arc, tr_off, arrays, t, EDGES, top, cell, levels)
            for nm in ('volume', 'carried'):
                (g_, gm_), (w_, m_) = got[nm], want[nm]
                assert g_.shape == w_.shape == gm_.shape == (EDGES.size + 2, ref.row_length), nm
                seen |= m_.max(axis=1) > 0
                assert numpy.all(numpy.abs(g_ - w_) <= 4 * EPS * m_), (nm, t, levels)
                assert numpy.all(numpy.abs(gm_ - m_) <= 4 * EPS * m_), (nm, t, levels)
                assert not g_[-1].any() and not gm_[-1].any()              # every depth is finite: the last row is empty
            # the fractions of every spread term add up to 1
            assert got['fraction_error'] <= 4 * EPS and want['fraction_error'] <= 4 * EPS
            assert got['spread_terms'] > 20 or levels[1] < NZ           # (the thin upper levels may each lie inside one row)
        # conservation: the rows add up to the profile rows of ResolvedReference under the same thickness
        got = ref.depth_step(array_values(arrays, t), EDGES, top=top)
        step = ref.step(array_values(arrays, t))
        for nm, key in (('volume', 'volume_profile'), ('carried', 'tracer_profile')):
            (g_, gm_), (w_, wm_) = got[nm], step[key]
            assert numpy.all(numpy.abs(g_.sum(axis=0) - w_.sum(axis=0)) <= 8 * EPS * wm_.sum(axis=0)), (nm, t)
            assert numpy.all(numpy.abs(gm_.sum(axis=0) - wm_.sum(axis=0)) <= 8 * EPS * wm_.sum(axis=0)), (nm, t)
    assert seen[:4].all() and not seen[-1]
    assert cell == bool(seen[5])                                            # the cell thicknesses reach deeper than sum(TH)
    only_volume = ref.depth_step(array_values(arrays, 0), EDGES, top=top, tracer=False)
    assert 'carried' not in only_volume
    assert numpy.array_equal(only_volume['volume'][0], ref.depth_step(array_values(arrays, 0), EDGES, top=top)['volume'][0])


def test_the_interval_rule_one_by_one():
    e = numpy.array([0., 1., 2., 4.])
    n, inf, nan = e.size, numpy.inf, numpy.nan

    def one(a, b):
        ent, row, frac = shares(*depth_intervals([a], [b]), e)
        assert not ent.any()
        return list(zip(row.tolist(), frac.tolist()))

    assert one(1.5, 1.5) == [(2, 1.0)]                                  # a zero (or missing) thickness: lo == hi
    assert one(1., 1.) == [(2, 1.0)]                                    # ... on an edge: the row below the edge
    assert one(-3., -3.) == [(0, 1.0)] and one(7., 7.) == [(n, 1.0)]
    assert one(1.5, inf) == [(n + 1, 1.0)]                              # +inf thickness: the lower interface is not finite
    assert one(inf, inf) == [(n + 1, 1.0)]                              # ... and every level below it
    assert one(inf, nan) == [(n + 1, 1.0)] and one(nan, 1.) == [(n + 1, 1.0)]
    big = numpy.finfo(numpy.float64).max
    assert one(-big, big) == [(n + 1, 1.0)]                             # the difference overflows
    assert one(1.25, 1.75) == [(2, 1.0)]                                # inside one row: (hi - lo) / (hi - lo)
    assert one(1., 2.) == [(2, 1.0)]                                    # lo and hi on edges: the zero-width row 3 gets nothing
    assert one(0.5, 2.5) == [(1, 0.25), (2, 0.5), (3, 0.25)]
    assert one(2.5, 0.5) == [(1, 0.25), (2, 0.5), (3, 0.25)]            # a negative thickness: the same interval
    assert one(-2., 6.) == [(0, 0.25), (1, 0.125), (2, 0.125), (3, 0.25), (4, 0.25)]


def _one_face(e3u, uo, edges, top=0.0, thickness=None):
    """the rows of ONE entry -- the east slot of cell 4 of a 3 x 3 grid, weight 1, arc 1 -- level by level"""
    nz = len(uo)
    full = lambda col: numpy.repeat(numpy.asarray(col, dtype=numpy.float64)[None, :, None], 9, axis=2).reshape(1, nz, 3, 3)  # noqa: E731
    arrays = {'uo': full(uo), 'vo': full(uo)}
    cell = e3u is not None
    if cell:
        arrays['e3u'] = arrays['e3v'] = full(e3u)
    ref = DepthRemapReference([4 * 4 + 1], [1.0], [0], numpy.ones((9, 4)), numpy.ones(nz) if thickness is None else thickness,
                              [0, 1], 3, 3, thick_markers=(THFILL, THMISSING), cell_thickness=cell)
    D = ref.interface_depths(array_values(arrays, 0), top)
    with numpy.errstate(invalid='ignore'):
        out = ref.depth_step(array_values(arrays, 0), edges, top=top, tracer=False)
    return D[:, 0], out['volume'][0][:, 0], out


def test_the_fallbacks_of_the_thickness_one_by_one():
    e = numpy.array([1., 2., 4.])
    inf, nan = numpy.inf, numpy.nan
    # zero, marker and NaN thicknesses count as 0: the depth stands still and the term, +-0, goes whole to row(lo)
    D, rows, out = _one_face([2.0, 0.0, THFILL, THMISSING, nan, 1.0], [1.] * 6, e)
    assert D.tolist() == [0., 2., 2., 2., 2., 2., 3.]
    assert out['flat_terms'] == 4 and out['spread_terms'] == 1
    assert rows.tolist() == [1.0, 1.0, 1.0, 0.0, 0.0]                     # [0, 2]: a half each to rows 0 and 1; [2, 3]: row 2
    # a single level
    D, rows, out = _one_face([4.0], [2.], e)
    assert D.tolist() == [0., 4.] and rows.tolist() == [2.0, 2.0, 4.0, 0.0, 0.0]
    # a negative thickness: the interval is the same one, upside down; the term has the sign of the thickness
    D, rows, out = _one_face([4.0, -2.0], [1., 1.], e)
    assert D.tolist() == [0., 4., 2.] and rows.tolist() == [1.0, 1.0, 2.0 - 2.0, 0.0, 0.0]
    # +inf: that level and every level below it go to row n + 1, whatever they carry; the levels above are untouched
    D, rows, out = _one_face([1.0, inf, 1.0], [1., 0.5, 1.], e)
    assert D.tolist() == [0., 1., inf, inf]
    assert rows[:4].tolist() == [1.0, 0.0, 0.0, 0.0] and rows[4] == inf
    # `top` moves every interface; the scalar thickness takes the same path
    D, rows, out = _one_face(None, [1., 1.], e, top=-1.0, thickness=numpy.array([2.0, 2.0]))
    assert D.tolist() == [-1.0, 1.0, 3.0] and rows.tolist() == [2.0, 1.0, 1.0, 0.0, 0.0]
    assert out['on_edge'] == 1


def _gpu_weights(oracle, grid):
    nx, ny = grid
    o = oracle.DataGen(nx, ny, GPU_NZ, GPU_NT, -180., 180., -90., 90., lat_uses_dx=False)
    pts = oracle.assemble_points(o.bounds_lon, o.bounds_lat)
    arc = oracle.arc_lengths(pts)
    ws = [oracle.polyline_weights(pts, transect_xyz(s), periodX=360.) for s in GPU_LINES]
    tr_off = numpy.concatenate([[0], numpy.cumsum([w.nseg for w in ws])])
    ce = numpy.concatenate([w.cell_edge for w in ws])
    wt = numpy.concatenate([w.weight for w in ws])
    sg = numpy.concatenate([w.seg + tr_off[p] for p, w in enumerate(ws)])
    return ce, wt, sg, numpy.asarray(arc).reshape(-1, 4), tr_off


@pytest.mark.parametrize('thick', ['scalar', 'timevarying'])
@pytest.mark.parametrize('grid', GPU_GRIDS, ids=lambda g: f'{g[0]}x{g[1]}')
@pytest.mark.parametrize('real', ['float64', 'float32'])
def test_generated_inputs_spread_stand_still_and_land_on_edges(oracle, real, grid, thick):
    """conditions on the inputs of tests/test_gpu_depth_remap.py, checked without a GPU: with its thicknesses and edge sets
    terms are spread over more than one row, terms have lo == hi, and interface depths are exactly an edge"""
    nx, ny = grid
    ce, wt, sg, arc, tr_off = _gpu_weights(oracle, grid)
    shape = (GPU_NT, GPU_NZ, ny, nx)
    u, v = gross_velocities(real, shape, seed=GPU_UV_SEED)
    arrays = {'uo': u, 'vo': v}
    cell = thick != 'scalar'
    if cell:
        arrays['e3u'], arrays['e3v'] = depth_thickness(real, shape, seed=GPU_E3_SEED)
        for a in (arrays['e3u'], arrays['e3v']):
            x = a[~numpy.isnan(a)].astype(numpy.float64)
            x = x[(x != numpy.dtype(real).type(THFILL)) & (x != numpy.dtype(real).type(THMISSING))]
            assert numpy.all((x == 0) | ((x >= 0.25) & (x <= 4.))) and numpy.array_equal(8. * x, numpy.round(8. * x))
    ref = DepthRemapReference(ce, wt, sg, arc, GPU_TH, tr_off, nx, ny, uv_markers=(FILL, MISSING),
                              thick_markers=(THFILL, THMISSING), cell_thickness=cell)
    for n, edges in GPU_EDGES.items():
        got = ref.depth_step(array_values(arrays, n % GPU_NT), edges, tracer=False)
        assert got['spread_terms'] > 0 and got['on_edge'] > 0, (n, got['spread_terms'], got['on_edge'])
        assert got['flat_terms'] > 0 or not cell, n              # a scalar thickness > 0 never stands still
        assert got['fraction_error'] <= 4 * EPS


# ---- Python ----------------------------------------------------------------------------------------------------------------
def test_python_methods_check_their_arguments():
    import inspect
    from nemoflux_amd.field import Field
    assert str(inspect.signature(Field.computeDepthTransport)) == '(self, tIndex, carry=False, out=None, prefetch_next=None)'
    assert str(inspect.signature(Field.setDepthEdges)) == '(self, edges, top=0.0)'
    f = Field.__new__(Field)
    f.nt, f.nz, f.ny, f.nx = 2, 3, 4, 5
    f._lazy = None
    f._e3 = None
    with pytest.raises(RuntimeError, match='setDepthEdges first'):
        f.computeDepthTransport(0)
    f._depth_edges = (numpy.array([1., 2.]), 0.0)
    with pytest.raises(RuntimeError, match='out of range'):
        f.computeDepthTransport(2)
    with pytest.raises(RuntimeError, match='setTracer first'):
        f.computeDepthTransport(0, carry=True)
    # the rows go into the class-space helper as they are: the overturning streamfunction in depth
    rows = numpy.random.default_rng(4).standard_normal((6, 3))
    assert numpy.array_equal(Field.classStreamfunction(rows), numpy.cumsum(rows[:4], axis=0))


# ---- fluxplot --------------------------------------------------------------------------------------------------------------
def test_fluxplot_depth_bins_options_are_checked():
    from nemoflux_amd.fluxplot import main
    files = dict(tFile='/nonexistent/T.nc', uFile='/nonexistent/U.nc', vFile='/nonexistent/V.nc', lonLatPoints='(0,0),(1,1)')
    with pytest.raises(RuntimeError, match='--depth-bins needs at least two finite, strictly increasing edges'):
        main(depthBins='100', **files)
    with pytest.raises(RuntimeError, match='--depth-bins must be E0,E1,...,EN'):
        main(depthBins='0,x', **files)
    with pytest.raises(RuntimeError, match='--depth-top needs --depth-bins'):
        main(depthTop=2.0, **files)
    with pytest.raises(RuntimeError, match='--depth-top must be a finite number'):
        main(depthBins='0,100', depthTop=numpy.inf, **files)
    for kw, opt in ((dict(tracer='sigma0', classes='26,27'), '--classes'), (dict(classes2='34,35'), '--classes2'),
                    (dict(grossClasses='26,27'), '--gross-classes'), (dict(classArea='26,27'), '--class-area'),
                    (dict(crossings='x.npz'), '--crossings'), (dict(gross=True), '--gross'), (dict(levels=True), '--levels'),
                    (dict(decompose=True), '--decompose'), (dict(eddy=True), '--eddy'), (dict(show=True), '--show'),
                    (dict(carry='thetao'), '--carry'), (dict(sigma='thetao,so'), '--sigma'), (dict(zrange='0,100'), '--zrange'),
                    (dict(remap='linear'), '--remap'), (dict(thicknessWeighted=True), '--thickness-weighted')):
        with pytest.raises(RuntimeError, match='--depth-bins and ' + opt + ' cannot be combined'):
            main(depthBins='0,100,500', **kw, **files)
    with pytest.raises(RuntimeError, match='--tracer-ref / --tracer-scale need --tracer'):
        main(depthBins='0,100', tracerRef=1.0, **files)
    with pytest.raises(RuntimeError, match='need --cell-thickness'):
        main(depthBins='0,100', e3u='e3u_0', **files)
    # accepted combinations go on to open the files
    for kw in (dict(), dict(sverdrup=True), dict(depthTop=-1.5), dict(tracer='thetao', tracerRef=1.5, tracerScale=4.1e-3),
               dict(cellThickness=True), dict(tracer='thetao', cellThickness=True, e3u='e3u_0')):
        with pytest.raises(RuntimeError, match='no such file'):
            main(depthBins='0,100,500,1000', **kw, **files)


def test_fluxplot_command_line_lists_depth_bins():
    out = subprocess.run([sys.executable, '-m', 'nemoflux_amd.fluxplot', '--help'], cwd=ROOT, capture_output=True, text=True,
                         timeout=120)
    assert out.returncode == 0, out.stderr
    assert '--depth-bins' in out.stdout and '--depth-top' in out.stdout
