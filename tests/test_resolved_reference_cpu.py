"""tests/resolved_reference.py, the sparse float64 reference of the resolved products that the GPU tests at 75 levels and at
the bench size compare the kernels with, checked here without a GPU: on two tiny grids, with weights and arc lengths from
the CPU oracle, it equals a deliberately naive loop over (entry, level) that reads the full arrays with Python scalars and
sums every output value with math.fsum, to 4 eps x sum |terms|."""
import bisect
import math

import numpy
import pytest

from conftest import transect_xyz
from resolved_reference import ResolvedReference, array_values

EPS = numpy.finfo(numpy.float64).eps
FILL, MISSING = 1.e20, -999.                 # markers of uo / vo
TFILL, TMISSING = -32768., 12345.            # markers of the class field
CFILL, CMISSING = 9999., -7777.              # markers of the carried tracer
REF = 3.25
EDGE_SETS = [numpy.array([8., 12.]), numpy.array([0., 5., 8., 10., 12., 15., 20.]), numpy.linspace(2., 18., 16)]
NZ, NT = 3, 2

GRIDS = {
    # periodic, wrap: lines across the +-180 seam and through column 0, along row 0 and the last row
    'periodic': dict(nx=12, ny=6, box=(-180., 180., -90., 90.), periodX=360., wrap=True, sverdrup=True, lines=[
        "(150,-50),(179,-20),(200,35),(160,70)", "(-175,-88),(-100,-62),(-170,20),(-185,75)", "(-20,-89),(175,-89)",
        "(-170,89),(10,88),(10,-10)"]),
    # regional, no wrap: lines inside column 0, the last column, row 0 and the last row
    'regional': dict(nx=9, ny=7, box=(0., 9., 0., 7.), periodX=0., wrap=False, sverdrup=False, lines=[
        "(0.3,0.2),(8.63,4.2),(4.5,6.59)", "(8.63,0.45),(8.61,6.59)", "(0.61,6.59),(8.63,6.56)", "(0.4,6.7),(0.6,0.3),(8.2,0.4)"]),
}


def _arrays(real, nx, ny, seed):
    rng = numpy.random.default_rng(seed)
    dt = numpy.dtype(real).type
    shape = (NT, NZ, ny, nx)

    def plant(a, values, share):
        flat = a.reshape(-1)
        for m in values:
            flat[rng.choice(a.size, max(1, a.size // share), replace=False)] = dt(m)
        return a

    uo = plant(rng.standard_normal(shape).astype(dt), (FILL, MISSING, numpy.nan), 10)
    vo = plant(rng.standard_normal(shape).astype(dt), (FILL, MISSING, numpy.nan), 10)
    tau = plant((7.5 + 2. * rng.standard_normal(shape)).astype(dt), (CFILL, CMISSING, numpy.nan), 12)
    sig = (10. + 5. * rng.standard_normal(shape)).astype(dt)
    sig.reshape(-1)[rng.choice(sig.size, sig.size // 4, replace=False)] = rng.choice([8., 12.], sig.size // 4)   # faces on an edge
    plant(sig, (numpy.inf, -numpy.inf, TFILL, TMISSING, numpy.nan), 9)
    sig[:, :, 1, 1:3] = (numpy.inf, -numpy.inf)                    # a face whose mean is NaN: no class value
    return dict(uo=uo, vo=vo, tracer=tau, **{'class': sig})


def _naive(ce, w, sg, arc, th, tr_off, nx, ny, a, t, wrap, sverdrup, edges):
    """every output value as math.fsum of its terms, one (entry, level) at a time from the full arrays"""
    dt = a['uo'].dtype.type
    nseg, ntr = int(tr_off[-1]), len(tr_off) - 1
    tr_of = [p for p in range(ntr) for _ in range(tr_off[p], tr_off[p + 1])]
    nrow = len(edges) + 2

    def present(x, marks):
        return not math.isnan(x) and all(x != dt(m) for m in marks)

    def face(arr, z, ca, cb, marks):
        xa = arr[t, z].reshape(-1)[ca]
        pa = present(xa, marks)
        pb = cb is not None and present(arr[t, z].reshape(-1)[cb], marks)
        if pa and pb:
            return True, 0.5 * (float(xa) + float(arr[t, z].reshape(-1)[cb]))
        if pa:
            return True, float(xa)
        if pb:
            return True, float(arr[t, z].reshape(-1)[cb])
        return False, 0.0

    names = ('volume', 'tracer', 'volume_profile', 'tracer_profile', 'volume_classes', 'tracer_classes')
    shapes = ((), (), (NZ,), (NZ,), (nrow,), (nrow,))
    terms = {nm: {} for nm in names}

    def put(nm, idx, s, x):
        for col in (s, nseg + tr_of[s]):
            terms[nm].setdefault(idx + (col,), []).append(x)

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
            x = (a['uo'] if slot in (1, 3) else a['vo'])[t, z].reshape(-1)[ca]
            vel = float(x) if present(x, (FILL, MISSING)) else 0.0
            has_t, xt = face(a['tracer'], z, ca, cb, (CFILL, CMISSING))
            tf = xt - REF if has_t else 0.0
            al = float(arc[ca, 1]) if slot in (1, 3) else -float(arc[ca, 2])
            dv, dtau = (float(th[z]) * vel) * al, (float(th[z]) * (vel * tf)) * al
            if sverdrup:
                dv, dtau = dv * (6371000.0 / 1.e6), dtau * (6371000.0 / 1.e6)
            tv, tt = float(w[e]) * dv, float(w[e]) * dtau
            has_s, xs = face(a['class'], z, ca, cb, (TFILL, TMISSING))
            row = bisect.bisect_right(list(edges), xs) if has_s and not math.isnan(xs) else len(edges) + 1
            put('volume', (), s, tv)
            put('tracer', (), s, tt)
            put('volume_profile', (z,), s, tv)
            put('tracer_profile', (z,), s, tt)
            put('volume_classes', (row,), s, tv)
            put('tracer_classes', (row,), s, tt)
    out = {}
    for nm, shape in zip(names, shapes):
        want, mag = numpy.zeros(shape + (nseg + ntr,)), numpy.zeros(shape + (nseg + ntr,))
        for idx, xs in terms[nm].items():
            want[idx], mag[idx] = math.fsum(xs), math.fsum(abs(x) for x in xs)
        out[nm] = (want, mag)
    return out


@pytest.mark.parametrize('grid', sorted(GRIDS))
@pytest.mark.parametrize('real', ['float64', 'float32'])
def test_sparse_reference_is_the_naive_loop(oracle, real, grid):
    g = GRIDS[grid]
    nx, ny = g['nx'], g['ny']
    o = oracle.DataGen(nx, ny, NZ, NT, *g['box'], lat_uses_dx=False)
    pts = oracle.assemble_points(o.bounds_lon, o.bounds_lat)
    arc = oracle.arc_lengths(pts)
    ws = [oracle.polyline_weights(pts, transect_xyz(s), periodX=g['periodX']) for s in g['lines']]
    tr_off = numpy.concatenate([[0], numpy.cumsum([w.nseg for w in ws])])
    ce = numpy.concatenate([w.cell_edge for w in ws])
    wt = numpy.concatenate([w.weight for w in ws])
    sg = numpy.concatenate([w.seg + tr_off[p] for p, w in enumerate(ws)])
    assert ce.size > 40 and set((ce % 4).tolist()) == {0, 1, 2, 3}
    cells = ce // 4
    assert (cells % nx == 0).any() and (cells % nx == nx - 1).any() and (cells // nx == 0).any() and (cells // nx == ny - 1).any()
    th = numpy.array([0.5, 0.25, 2.0])
    a = _arrays(real, nx, ny, seed=nx * 100 + ny)
    ref = ResolvedReference(ce, wt, sg, arc, th, tr_off, nx, ny, uv_markers=(FILL, MISSING), tracer_markers=(CFILL, CMISSING),
                            class_markers=(TFILL, TMISSING), reference=REF, wrap=g['wrap'], sverdrup=g['sverdrup'])
    for t in range(NT):
        got = ref.step(array_values(a, t), EDGE_SETS)
        for k, edges in enumerate(EDGE_SETS):
            want = _naive(ce, wt, sg, arc, th, tr_off, nx, ny, a, t, g['wrap'], g['sverdrup'], edges)
            for nm, (w_, m_) in want.items():
                g_, gm_ = got[(nm, k)] if nm.endswith('classes') else got[nm]
                assert g_.shape == w_.shape == m_.shape, nm
                assert m_.max() > 0, nm
                worst = (numpy.abs(g_ - w_) / numpy.maximum(m_, 1e-300)).max()
                assert numpy.all(numpy.abs(g_ - w_) <= 4 * EPS * m_), (nm, k, t, worst)
                assert numpy.all(numpy.abs(gm_ - m_) <= 4 * EPS * m_), (nm, k, t)
            rows_mag = want['tracer_classes'][1]
            assert rows_mag[-1].max() > 0, 'faces without a class value carry flux'
            if k == 0:
                assert rows_mag[0].max() > 0 and rows_mag[len(edges)].max() > 0, 'the open classes at both ends carry flux'
