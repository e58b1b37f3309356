// nf_integral.hip -- K3: gather of the weighted edge fluxes and their reduction onto target segments.
//
// Replaces  mint.PolylineIntegral.getIntegral(data, mint.CELL_BY_CELL_DATA) as driven by
//           nemoflux/field.py:102 and nemoflux/fluxplot.py:56, for ALL transects of a Field at once.
//
// Records (cell, 4 edge weights, global segment id) are sorted by segment (K2).  Stage A: one lane per record loads it
// (load_record), forms one or more values from the cell's edge values (neighbours, weighted_sum) and runs a WAVEFRONT
// SEGMENTED SCAN keyed by the segment id (seg_scan); the last lane of every run inside the wave stores the run's sums.  The
// five stage-A kernels (gather, pair, unique edges, per-level profile, tracer classes) are made of these same pieces, which is
// why their rows can be compared bit for bit.  Stage B: one wavefront per target segment stitches the run sums of the waves
// the segment spans.  Stage C: one wavefront per transect adds its segments.  No atomics: the summation tree is fixed, so
// results are bitwise reproducible.
//
// Output row: [ per-segment sums (nseg) | per-transect sums (ntransect) ].
#include <type_traits>

#include "nf_common.h"

namespace nf {

// ---- the pieces of stage A: load record -> form value(s) -> scan -> store --------------------------------------------------
typedef double dvec2 __attribute__((ext_vector_type(2)));

// A (cell, 4 weights) record without its key.  The record stream is read once per launch: non-temporal, so that it does not
// push the plane sectors its neighbours gather -- nor the arc lengths the next flux kernel re-reads -- out of the caches
// (-0.7 % per pass).  The key has a load of its own: where it sits among a kernel's gathers decides the kernel's registers.
struct Record {
    long c;         // cell
    dvec2 wa, wb;   // the weights of the south and east slots, of the north and west slots
};
__device__ inline Record load_record(const int *__restrict__ cell, const double *__restrict__ w4, long k)
{
    const dvec2 *pw = reinterpret_cast<const dvec2 *>(w4 + 4 * k);
    return Record{__builtin_nontemporal_load(cell + k), __builtin_nontemporal_load(pw), __builtin_nontemporal_load(pw + 1)};
}
__device__ inline int load_key(const int *__restrict__ seg, long k) { return __builtin_nontemporal_load(seg + k); }

// The neighbour rule of cell c = (j, i) on rows of nx.  The south and west slots of a cell are copies of the neighbours' north
// and east values (field.py:219-223): south = eV(cs), cs = c - nx; west = eU(cw), cw = c - 1.  Row 0's south slot is never
// written (south = false; cs = c may then be read and is discarded), column 0 takes the periodic copy of column nx - 1.
struct Neighbours {
    unsigned j, i;
    bool south;
    long cs, cw;
};
__device__ inline Neighbours neighbours(long c, unsigned nx)
{
    const unsigned j = (unsigned)(c / nx), i = (unsigned)(c - (long)j * nx);
    return Neighbours{j, i, j > 0, j > 0 ? c - nx : c, i > 0 ? c - 1 : c - 1 + nx};
}

// A record's four slot values, in the order the kernels load them, and their sum times the weights (south, east, north, west)
// with K3's association; the library is built with -ffp-contract=off: these rounded products and sums wherever it is used.
struct Slots { double e, n, s, w; };
__device__ inline double weighted_sum(const Record &r, const Slots &d)
{
    return ((r.wa.x * d.s + r.wa.y * d.e) + r.wb.x * d.n) + r.wb.y * d.w;
}

// the slot values from the engine's own planes, read through the two signed ones only (eU, with eV right behind it at + ncell):
// eU[c-1], eU[c] share a sector and eV[c-nx] is the eV[c] of the record one row below -- about half the sectors of four planes
__device__ inline Slots signed_plane_slots(const double *__restrict__ eU, long ncell, long c, const Neighbours &nb)
{
    const double *eV = eU + ncell;
    return Slots{eU[c], eV[c], nb.south ? eV[nb.cs] : 0.0, eU[nb.cw]};
}

// the same slot values from K1's interleaved stream E, E[2c] = eU[c], E[2c + 1] = eV[c]: east and north are ONE 16-byte load,
// the west value sits in the same 64-byte sector three times out of four, and the south value is in the sector that the
// record one row below pulls for its own cell -- three loads per record instead of four
__device__ inline Slots interleaved_slots(const double *__restrict__ E, long c, const Neighbours &nb)
{
    const dvec2 ec = reinterpret_cast<const dvec2 *>(E)[c];
    return Slots{ec.x, ec.y, nb.south ? E[2 * nb.cs + 1] : 0.0, E[2 * nb.cw]};
}

// The wavefront segmented scan keyed by the segment id (key -1: a lane without a record), 6 shuffle steps.  seg_scan_take: the
// lane o below is in the same run -- it depends on the keys only, so it is formed once per step for any number of values;
// seg_scan_step adds the values from o below where it holds; seg_run_end: record k is the last of its run inside the wave.
__device__ inline bool seg_scan_take(int key, int lane, int o)
{
    const int pk = __shfl_up(key, o, kWave);
    return lane >= o && pk == key;
}
template <int N>
__device__ inline void seg_scan_step(double (&val)[N], int o, bool take)
{
#pragma unroll
    for (int l = 0; l < N; ++l) {
        const double pv = __shfl_up(val[l], o, kWave);
        val[l] = take ? val[l] + pv : val[l];
    }
}
__device__ inline bool seg_run_end(int key, int lane, long k, long n)
{
    const int nk = __shfl_down(key, 1, kWave);
    return k < n && (lane == kWave - 1 || k == n - 1 || nk != key);
}
template <int N>
__device__ inline bool seg_scan(double (&val)[N], int key, long k, long n)
{
    const int lane = threadIdx.x & (kWave - 1);
#pragma unroll
    for (int o = 1; o < kWave; o <<= 1) seg_scan_step(val, o, seg_scan_take(key, lane, o));
    return seg_run_end(key, lane, k, n);
}

// One level's slot values from the raw fields, formed as K1 forms them for a field whose only non-zero layer is that level:
// eU(c) = +fma(th, uv_fixed(u[c]), 0) * arcE[c], eV(c) = -fma(th, uv_fixed(v[c]), 0) * arcN[c], times the Sverdrup scale;
// east = eU(c), north = eV(c), south = eV(cs) (0 on row 0), west = eU(cw).  Arcs, LevelUV: what is gathered for them.
struct Arcs { double Ec, Nc, Ns, Ew; };
__device__ inline Arcs load_arcs(const double *__restrict__ arcE, const double *__restrict__ arcN, long c, const Neighbours &nb)
{
    return Arcs{arcE[c], arcN[c], arcN[nb.cs], arcE[nb.cw]};
}
template <typename T>
struct LevelUV {
    T uc, uw, vc, vs;
};
template <typename T>
__device__ inline LevelUV<T> load_level_uv(const T *__restrict__ u, const T *__restrict__ v, long o, long c,
                                           const Neighbours &nb)
{
    return LevelUV<T>{u[o + c], u[o + nb.cw], v[o + c], v[o + nb.cs]};
}
// The carried-tracer form multiplies every masked velocity by the tracer at the slot's own face (FaceTf: east face of c, north
// face of c, north face of cs, east face of cw): fma(th, fixed(x) * tf, 0) * arc, one level of k_tracer_flux's accumulation.
struct FaceTf { double e, n, s, w; };
// The thickness of each slot's term: the level's one number in all four (slot_th), or with per-cell thicknesses the value at
// the slot's own face -- east e3u[c], north e3v[c], south e3v[cs], west e3u[cw] -- masked by thick_fixed (level_th).
struct SlotTh { double e, n, s, w; };
__device__ inline SlotTh slot_th(double th) { return SlotTh{th, th, th, th}; }
template <typename T>
__device__ inline LevelUV<T> load_level_e3(const ThickIn<T> &ct, long o, long c, const Neighbours &nb)
{
    return load_level_uv(ct.e3u, ct.e3v, o, c, nb);
}
template <typename T>
__device__ inline SlotTh level_th(const LevelUV<T> &e3, const ThickIn<T> &ct)
{
    return SlotTh{thick_fixed<T>(e3.uc, ct.m1, ct.m2), thick_fixed<T>(e3.vc, ct.m1, ct.m2), thick_fixed<T>(e3.vs, ct.m1, ct.m2),
                  thick_fixed<T>(e3.uw, ct.m1, ct.m2)};
}
template <typename T, bool TR>
__device__ inline Slots level_slots_tf(const SlotTh &th, const LevelUV<T> &x, const Arcs &arc, T fill, T fill2, bool two, double scale,
                                       int sverdrup, bool south, const FaceTf &tf)
{
    auto term = [&](double th, T x, double a, double f) {
        const double xf = uv_fixed<T>(x, fill, fill2, two);
        return fma(th, TR ? xf * f : xf, 0.0) * a;
    };
    Slots d{+term(th.e, x.uc, arc.Ec, tf.e), -term(th.n, x.vc, arc.Nc, tf.n), -term(th.s, x.vs, arc.Ns, tf.s),
            +term(th.w, x.uw, arc.Ew, tf.w)};
    if (sverdrup) d = Slots{d.e * scale, d.n * scale, d.s * scale, d.w * scale};
    if (!south) d.s = 0.0;
    return d;
}
template <typename T>
__device__ inline Slots level_slots(double th, const LevelUV<T> &x, const Arcs &arc, T fill, T fill2, bool two, double scale,
                                    int sverdrup, bool south)
{
    return level_slots_tf<T, false>(slot_th(th), x, arc, fill, fill2, two, scale, sverdrup, south, FaceTf{});
}

// The neighbour rule with the east and north cells that the faces of a tracer need (ce, cn: c itself where there is none).
//   faces: east(c) = (tau[c], tau[c+1]; column nx-1: tau[c+1-nx] when wrap_x, else none), north(c) = (tau[c], tau[c+nx];
//   last row: none), the west slot is east(cw), the south slot north(cs).
struct ClassNeighbours : Neighbours {
    bool has_e, has_n, has_w;
    long ce, cn;
};
__device__ inline ClassNeighbours class_neighbours(long c, unsigned nx, long ncell, int wrap_x)
{
    ClassNeighbours nb;
    static_cast<Neighbours &>(nb) = neighbours(c, nx);
    nb.has_e = nb.i + 1 < nx || wrap_x;
    nb.has_n = c + (long)nx < ncell;
    nb.has_w = nb.i > 0 || wrap_x;
    nb.ce = nb.i + 1 < nx ? c + 1 : (wrap_x ? c + 1 - (long)nx : c);
    nb.cn = nb.has_n ? c + nx : c;
    return nb;
}

// One level of a tracer around a record's cell: the five values that its four faces need, in the order they are loaded
template <typename T>
struct LevelTau {
    T c, e, n, w, s;
};
template <typename T>
__device__ inline LevelTau<T> load_level_tau(const T *__restrict__ tau, long o, long c, const ClassNeighbours &nb)
{
    return LevelTau<T>{tau[o + c], tau[o + nb.ce], tau[o + nb.cn], tau[o + nb.cw], tau[o + nb.cs]};
}
// the carried tracer of the tracer forms: its step base, its two markers, its reference and the wrap rule of its faces
template <typename T>
struct TauIn {
    const T *tau;
    T m1, m2;
    double ref;
    int wrap_x;
};
template <typename T>
inline TauIn<T> tau_of(const TracerIn &t) { return TauIn<T>{(const T *)t.tau, (T)t.fill, (T)t.fill2, t.ref, t.wrap_x ? 1 : 0}; }
// the trailing arguments of a kernel that has a volume form (none) and a carried-tracer form (one TauIn)
template <typename T>
__device__ inline TauIn<T> tau_in() { return TauIn<T>{}; }
template <typename T>
__device__ inline TauIn<T> tau_in(const TauIn<T> &ti) { return ti; }
// ... and, for the profile, a volume form with per-cell thicknesses (one ThickIn): the other kind of argument is absent
template <typename T>
__device__ inline TauIn<T> tau_in(const ThickIn<T> &) { return TauIn<T>{}; }
template <typename T>
__device__ inline ThickIn<T> thick_arg() { return ThickIn<T>{}; }
template <typename T>
__device__ inline ThickIn<T> thick_arg(const TauIn<T> &) { return ThickIn<T>{}; }
template <typename T>
__device__ inline ThickIn<T> thick_arg(const ThickIn<T> &ct) { return ct; }
// tr_face at the four slots' faces.  Row 0 has no south face: cs = c there and level_slots_tf discards the slot.
template <typename T>
__device__ inline FaceTf level_tf(const LevelTau<T> &t, const ClassNeighbours &nb, const TauIn<T> &ti)
{
    return FaceTf{tr_face<T>(t.c, t.e, nb.has_e, ti.m1, ti.m2, ti.ref), tr_face<T>(t.c, t.n, nb.has_n, ti.m1, ti.m2, ti.ref),
                  tr_face<T>(t.s, t.c, true, ti.m1, ti.m2, ti.ref), tr_face<T>(t.w, t.c, nb.has_w, ti.m1, ti.m2, ti.ref)};
}
// the neighbour rule a form needs: the volume forms' (TR = false) or the one with the tracer's faces
template <bool TR>
__device__ inline auto step_neighbours(long c, unsigned nx, long ncell, int wrap_x)
{
    if constexpr (TR)
        return class_neighbours(c, nx, ncell, wrap_x);
    else
        return neighbours(c, nx);
}

// ---- the pieces of the windowed-row kernels (class, remap, depth, surface, joint bin) -----------------------------------------
// A lane keeps one accumulator per row of the window [r0, r0 + nwin) as a column of LDS, acc[q * STRIDE] with acc already
// offset by the lane (a dynamic row index in registers would go to scratch); STRIDE: the lanes of a workgroup.  The order in
// which a lane adds to a row, and the scan, are what the rows' bit-for-bit identities rest on: they live here only.
// window_add: x to row `row` when it lies in the window.
template <int STRIDE>
__device__ inline void window_add(double *acc, int row, int r0, int nwin, double x)
{
    const int q = row - r0;
    if (q >= 0 && q < nwin) acc[q * STRIDE] += x;
}

// window_scan_store: the flags of all six scan steps formed once and kept as bits, then seg_scan_step once per row of the
// window; the last lane of a run stores row q of the window to runsum[q * n + k].
template <int STRIDE>
__device__ inline void window_scan_store(const double *acc, int key, int lane, long k, long n, int nwin, double *__restrict__ runsum)
{
    unsigned take = 0;
#pragma unroll
    for (int o = 1, b = 0; o < kWave; o <<= 1, ++b)
        if (seg_scan_take(key, lane, o)) take |= 1u << b;
    const bool store = seg_run_end(key, lane, k, n);
    for (int q = 0; q < nwin; ++q) {
        double val[1] = {k < n ? acc[q * STRIDE] : 0.0};
#pragma unroll
        for (int o = 1, b = 0; o < kWave; o <<= 1, ++b) seg_scan_step(val, o, take & (1u << b));
        if (store) runsum[(long)q * n + k] = val[0];
    }
}

// The LDS of a kBlock workgroup with one edge table: the edges (nedges doubles, padded to even), then nwin x kBlock
// accumulators.  window_lds copies the edges, zeroes the lane's column and returns after the barrier (for the edges: every
// lane touches only its own accumulators).
struct WindowLds {
    const double *e;
    double *acc;   // acc[q * kBlock]: this lane's row r0 + q
};
__device__ inline WindowLds window_lds(const double *__restrict__ edges, int nedges, int nwin)
{
    extern __shared__ double class_lds[];
    double *e = class_lds;
    double *acc = class_lds + ((nedges + 1) & ~1) + threadIdx.x;
    for (int q = threadIdx.x; q < nedges; q += kBlock) e[q] = edges[q];
    for (int r = 0; r < nwin; ++r) acc[r * kBlock] = 0.0;
    __syncthreads();
    return WindowLds{e, acc};
}

// Where a term goes among rows bounded by non-decreasing edges: the rows jlo .. jhi of the interval [lo, hi], or (jhi < 0)
// whole to row jlo.  make_span: the interval between a and b; whole to row `none` where !ok or a, b or their difference is not
// finite.  rows(lo, hi): the kernel's row lookup, which returns the span of lo <= hi: whole to the row of lo where lo == hi.
// (The lookup decides how: class_row looks hi up only where lo < hi, the linear count takes both in one pass.)
struct RowSpan {
    double lo, hi;
    int jlo, jhi;
};
template <typename Rows>
__device__ inline RowSpan make_span(bool ok, double a, double b, int none, Rows rows)
{
    if (!(ok && __builtin_isfinite(a) && __builtin_isfinite(b) && __builtin_isfinite(b - a))) return RowSpan{0.0, 0.0, none, -1};
    const double lo = a < b ? a : b, hi = a < b ? b : a;
    return rows(lo, hi);
}

// The share rule: the term t spread uniformly over [lo, hi]; row j gets  t * ((right - left) / (hi - lo))  with [left, right]
// the part of the interval inside the row, rows ascending, the loop clipped to the window [r0, rend] first.  e[j * ESTRIDE]:
// the upper edge of row j.  add_span: that, or the whole term to row jlo.  k_depth_segscan's `put` is a written-out copy of
// add_span<kBlock, 1> (the reason is there): keep the two alike.
template <int STRIDE, int ESTRIDE>
__device__ inline void spread_span(double *acc, const double *e, const RowSpan &p, double t, int r0, int rend)
{
    const double width = p.hi - p.lo;
    const int ja = p.jlo > r0 ? p.jlo : r0, jb = p.jhi < rend ? p.jhi : rend;
    for (int j = ja; j <= jb; ++j) {
        const double left = j == p.jlo ? p.lo : e[(j - 1) * ESTRIDE], right = j == p.jhi ? p.hi : e[j * ESTRIDE];
        if (right != left) acc[(j - r0) * STRIDE] += t * ((right - left) / width);
    }
}
template <int STRIDE, int ESTRIDE>
__device__ inline void add_span(double *acc, const double *e, const RowSpan &p, double t, int r0, int nwin)
{
    if (p.jhi < 0) return window_add<STRIDE>(acc, p.jlo, r0, nwin, t);
    spread_span<STRIDE, ESTRIDE>(acc, e, p, t, r0, r0 + nwin - 1);
}

// The depth walk of a record: D, the depth of the upper interface of the next level at the four faces, starts at `surface`
// and grows by the thickness at each slot's own face -- level_th of the gathered e3u / e3v (CT: four running depths per lane)
// or thickness[z] (one) -- one float64 addition per level.  Levels [0, z0) of a partial slab only move the depths: with
// per-cell thicknesses their four gathers per level are issued kDepthLevels levels at a time, nothing else is read.  Owned
// levels go kDepthLevels at a time too, all gathers of a batch (4 per level, + 4 with CT, + 5 with a carried tracer, TR) issued
// before the first is used; each owned level, z ascending, is handed to  level(D, Dn, d, south):  its upper and lower depths,
// the four slot terms (k_gross_segscan's: level_slots_tf with the thickness at the face) and whether the south slot exists.
// The terms come without their weights: the callee forms each product where it adds it, so that the south product exists
// only under `if (south)` (formed here, ahead of that branch, it costs the surface kernel registers).  The callee adds in
// slot order: south (if there) r.wa.x * d.s, east r.wa.y * d.e, north r.wb.x * d.n, west r.wb.y * d.w.
constexpr int kDepthLevels = 4;
template <typename T, bool TR, bool CT, typename NB, typename F>
__device__ inline void depth_walk(const Record &r, const NB &nb, const Arcs &arc, const T *__restrict__ u, const T *__restrict__ v,
                                  long ncell, int z0, int z1, const double *__restrict__ thickness, T fill, T fill2, int two,
                                  double scale, int sverdrup, const TauIn<T> &ti, const ThickIn<T> &ct, double surface, F level)
{
    constexpr int DL = kDepthLevels;
    SlotTh D = slot_th(surface);
    auto below = [](const SlotTh &d, const SlotTh &th) { return SlotTh{d.e + th.e, d.n + th.n, d.s + th.s, d.w + th.w}; };
    for (int z = 0; z < z0; z += DL) {   // above the owned levels: the depths move, no term
        const int nlev = z0 - z < DL ? z0 - z : DL;
        if constexpr (CT) {
            LevelUV<T> e3[DL];
#pragma unroll
            for (int l = 0; l < DL; ++l)
                if (l < nlev) e3[l] = load_level_e3(ct, (long)(z + l) * ncell, r.c, nb);
#pragma unroll
            for (int l = 0; l < DL; ++l)
                if (l < nlev) D = below(D, level_th(e3[l], ct));
        } else {
            for (int l = 0; l < nlev; ++l) D = below(D, slot_th(thickness[z + l]));
        }
    }
    for (int z = z0; z < z1; z += DL) {
        const int nlev = z1 - z < DL ? z1 - z : DL;
        LevelUV<T> x[DL];
        LevelTau<T> tt[TR ? DL : 1];
        LevelUV<T> e3[CT ? DL : 1];
#pragma unroll
        for (int l = 0; l < DL; ++l)
            if (l < nlev) {
                const long o = (long)(z + l) * ncell;
                x[l] = load_level_uv(u, v, o, r.c, nb);
                if constexpr (CT) e3[l] = load_level_e3(ct, o, r.c, nb);
                if constexpr (TR) tt[l] = load_level_tau(ti.tau, o, r.c, nb);
            }
#pragma unroll
        for (int l = 0; l < DL; ++l)
            if (l < nlev) {
                FaceTf tf{};
                if constexpr (TR) tf = level_tf(tt[l], nb, ti);
                SlotTh th;
                if constexpr (CT)
                    th = level_th(e3[l], ct);
                else
                    th = slot_th(thickness[z + l]);
                const Slots d = level_slots_tf<T, TR>(th, x[l], arc, fill, fill2, two, scale, sverdrup, nb.south, tf);
                const SlotTh Dn = below(D, th);
                level(D, Dn, d, nb.south);
                D = Dn;
            }
    }
}

__global__ __launch_bounds__(kBlock) void k_gather_segscan(const int *__restrict__ cell,
                                                           const double *__restrict__ w4,
                                                           const int *__restrict__ seg, long n,
                                                           const double *__restrict__ data, long ncell,
                                                           int planes, unsigned nx, double *__restrict__ runsum,
                                                           long data_stride)
{
    data += (long)blockIdx.y * data_stride;  // blockIdx.y = time step of a multi-step launch
    runsum += (long)blockIdx.y * n;
    const long k = (long)blockIdx.x * kBlock + threadIdx.x;
    double val[1] = {0.0};
    int key = -1;
    if (k < n) {
        const Record r = load_record(cell, w4, k);
        Slots d;
        if (planes == 2) {   // the engine's own planes
            d = signed_plane_slots(data + ncell, ncell, r.c, neighbours(r.c, nx));
        } else if (planes) {
            d.s = data[r.c], d.e = data[ncell + r.c], d.n = data[2 * ncell + r.c], d.w = data[3 * ncell + r.c];
        } else {
            const double2 *pd = reinterpret_cast<const double2 *>(data + 4 * r.c);
            const double2 da = pd[0], db = pd[1];
            d = Slots{da.y, db.x, da.x, db.y};
        }
        val[0] = weighted_sum(r, d);
        key = load_key(seg, k);
    }
    if (seg_scan(val, key, k, n)) runsum[k] = val[0];
}

// Stage A for TWO time steps of the engine's own planes at once (the per-step pass takes its whole steps in pairs): the record
// is read once and both steps' sums go through seg_scan side by side.  uvA / uvB: a step's [eU | eV], or (A_IL / B_IL) its
// interleaved stream; runsum: 2 * n doubles.  <false, false> is the kernel as it was before the interleaved form existed.
template <bool A_IL, bool B_IL>
__global__ __launch_bounds__(kBlock) void k_gather_segscan_pair(const int *__restrict__ cell, const double *__restrict__ w4,
                                                                const int *__restrict__ seg, long n,
                                                                const double *__restrict__ uvA,
                                                                const double *__restrict__ uvB, long ncell, unsigned nx,
                                                                double *__restrict__ runsum)
{
    const long k = (long)blockIdx.x * kBlock + threadIdx.x;
    double val[2] = {0.0, 0.0};
    int key = -1;
    if (k < n) {
        const Record r = load_record(cell, w4, k);
        const Neighbours nb = neighbours(r.c, nx);
        val[0] = weighted_sum(r, A_IL ? interleaved_slots(uvA, r.c, nb) : signed_plane_slots(uvA, ncell, r.c, nb));
        val[1] = weighted_sum(r, B_IL ? interleaved_slots(uvB, r.c, nb) : signed_plane_slots(uvB, ncell, r.c, nb));
        key = load_key(seg, k);
    }
    if (seg_scan(val, key, k, n)) {
        runsum[k] = val[0];
        runsum[n + k] = val[1];
    }
}

// Unique-edge form of stage A for the engine's own planes (WeightSet::EdgeEntry): one lane per (segment, plane element)
// entry -- ONE 16-byte record load and ONE 8-byte gather from [eU | eV] -- then seg_scan.
// Entries are sorted by (segment, element), so the gathers of neighbouring lanes walk the planes in ascending order.
__global__ __launch_bounds__(kBlock) void k_gather_edges(const WeightSet::EdgeEntry *__restrict__ ent, long n,
                                                         const double *__restrict__ data, long ncell,
                                                         double *__restrict__ runsum, long data_stride)
{
    data += (long)blockIdx.y * data_stride + ncell;   // planes 1 (eU) and 2 (eV) are contiguous: one array of 2*ncell
    runsum += (long)blockIdx.y * n;
    const long k = (long)blockIdx.x * kBlock + threadIdx.x;
    double val[1] = {0.0};
    int key = -1;
    if (k < n) {
        typedef int ivec4 __attribute__((ext_vector_type(4)));
        const ivec4 r = __builtin_nontemporal_load(reinterpret_cast<const ivec4 *>(ent + k));   // read-once stream
        double w;
        const int wbits[2] = {r.z, r.w};
        __builtin_memcpy(&w, wbits, 8);
        val[0] = w * data[(unsigned)r.x];
        key = r.y;
    }
    if (seg_scan(val, key, k, n)) runsum[k] = val[0];
}

// one wavefront per target segment: stitch the per-wave run sums of the segment (one per 64-record wave it
// spans) with a lane-strided sum and a butterfly
__global__ __launch_bounds__(kBlock) void k_finalize_seg(const double *__restrict__ runsum,
                                                         const int *__restrict__ seg_start, int nseg,
                                                         double *__restrict__ row, long nrec, long row_stride)
{
    runsum += (long)blockIdx.y * nrec;
    row += (long)blockIdx.y * row_stride;
    const int s = (blockIdx.x * kBlock + threadIdx.x) / kWave;
    const int lane = threadIdx.x & (kWave - 1);
    if (s >= nseg) return;
    const long lo = seg_start[s], hi = seg_start[s + 1];
    double acc = 0.0;
    if (hi > lo) {
        const long w0 = lo / kWave, w1 = (hi - 1) / kWave;  // waves of stage A touched by this segment
        for (long w = w0 + lane; w <= w1; w += kWave) {
            long e = (w + 1) * kWave;
            if (e > hi) e = hi;
            acc += runsum[e - 1];
        }
    }
    for (int o = 32; o > 0; o >>= 1) acc += __shfl_xor(acc, o, kWave);
    if (lane == 0) row[s] = acc;
}

// one wavefront per transect: sum of its segments
__global__ __launch_bounds__(kBlock) void k_finalize_tr(const int *__restrict__ tr_off, int ntransect, int nseg,
                                                        double *__restrict__ row, long row_stride)
{
    row += (long)blockIdx.y * row_stride;
    const int p = (blockIdx.x * kBlock + threadIdx.x) / kWave;
    const int lane = threadIdx.x & (kWave - 1);
    if (p >= ntransect) return;
    double part = 0.0;
    for (int s = tr_off[p] + lane; s < tr_off[p + 1]; s += kWave) part += row[s];
    for (int o = 32; o > 0; o >>= 1) part += __shfl_xor(part, o, kWave);
    if (lane == 0) row[nseg + p] = part;
}

// stages B and C for nrows rows (blockIdx.y): row r stitches the run sums at runsum + r * nrun over the CSR run_start of
// the nseg segments (seg_start for the records, ent_start for the unique-edge entries) and goes to row + r * row_stride
static void launch_finalize(const Transects &tr, const int *run_start, long nrun, const double *runsum, double *row,
                            long row_stride, unsigned nrows, hipStream_t s)
{
    const int nseg = tr.ws->nseg;
    if (nseg > 0) {
        const unsigned nb = (unsigned)(((long)nseg * kWave + kBlock - 1) / kBlock);
        hipLaunchKernelGGL(k_finalize_seg, dim3(nb, nrows), dim3(kBlock), 0, s, runsum, run_start, nseg, row, nrun, row_stride);
    }
    if (tr.ntransect > 0) {
        const unsigned nb = (unsigned)(((long)tr.ntransect * kWave + kBlock - 1) / kBlock);
        hipLaunchKernelGGL(k_finalize_tr, dim3(nb, nrows), dim3(kBlock), 0, s, tr.tr_offsets_dev, tr.ntransect, nseg, row,
                           row_stride);
    }
}

static dim3 record_grid(const WeightSet &ws, unsigned ny = 1) { return dim3((unsigned)((ws.nrec + kBlock - 1) / kBlock), ny); }

// "edge_weights" tuning knob.  Default 0: measured in-process on the 65-transect bench batch (tools/ab_pass.py,
// profiles/r02_ab_pass_edges.txt) the unique-edge form is 0.4 % SLOWER per pass than the records (90 vs 85.5 us per step): a
// line shares only the edge it crosses with the next cell, so folding leaves 3 entries per record, not 2 -- 48 B of stream
// instead of 40 B -- and the 64-B sectors the gathers pull are the same ones either way.
static int g_use_edges = 0;
void integral_use_edges(int on) { g_use_edges = on; }
int integral_uses_edges() { return g_use_edges; }

int launch_integral(const WeightSet &ws, const double *data, long ncell, int planes, long nx,
                    const int *tr_offsets_dev, int ntransect, double *scratch, double *row, hipStream_t s, int nsteps,
                    long data_stride, long row_stride, const int *rec_cells)
{
    const Transects tr{&ws, tr_offsets_dev, ntransect};
    const unsigned ny = (unsigned)(nsteps > 1 ? nsteps : 1);
    const bool edges = planes == 2 && ws.ent_start.get() && g_use_edges;   // the engine's own planes through the unique edges
    if (edges && ws.nent > 0)
        hipLaunchKernelGGL(k_gather_edges, dim3((unsigned)((ws.nent + kBlock - 1) / kBlock), ny), dim3(kBlock), 0, s,
                           ws.ent.get(), ws.nent, data, ncell, scratch, data_stride);
    if (!edges && ws.nrec > 0)
        hipLaunchKernelGGL(k_gather_segscan, record_grid(ws, ny), dim3(kBlock), 0, s,
                           rec_cells ? rec_cells : ws.cell.get(), ws.w4.get(), ws.seg.get(), ws.nrec, data, ncell, planes,
                           (unsigned)(nx > 0 ? nx : 1), scratch, data_stride);
    launch_finalize(tr, edges ? ws.ent_start.get() : ws.seg_start.get(), edges ? ws.nent : ws.nrec, scratch, row, row_stride,
                    ny, s);
    NF_HIP(hipGetLastError());
    return NF_OK;
}

int launch_integral_pair(const Transects &tr, const double *uvA, const double *uvB, long ncell, long nx, double *scratch,
                         double *row, long row_stride, hipStream_t s, bool a_interleaved, bool b_interleaved)
{
    const WeightSet &ws = *tr.ws;
    NF_REQUIRE(a_interleaved || !b_interleaved, NF_ERR_ARG, "integral: operand B is interleaved only when A is");
    if (ws.nrec > 0) {
        auto *kernel = b_interleaved ? k_gather_segscan_pair<true, true>
                                     : (a_interleaved ? k_gather_segscan_pair<true, false> : k_gather_segscan_pair<false, false>);
        hipLaunchKernelGGL(kernel, record_grid(ws), dim3(kBlock), 0, s, ws.cell.get(), ws.w4.get(), ws.seg.get(), ws.nrec,
                           uvA, uvB, ncell, (unsigned)(nx > 0 ? nx : 1), scratch);
    }
    launch_finalize(tr, ws.seg_start.get(), ws.nrec, scratch, row, row_stride, 2, s);
    NF_HIP(hipGetLastError());
    return NF_OK;
}

// the launchers that read the raw fields check alike: grid sizes, level range, transects, `per_record` run sums of scratch each
static int check_raw_step(const char *what, const StepInput &in, const Transects &tr, size_t scratch_len, size_t per_record)
{
    const std::string w(what);
    NF_REQUIRE(tr.ws && in.ncell > 0 && in.nx > 0 && in.ncell % in.nx == 0 && in.ncell < (1l << 31), NF_ERR_ARG,
               w + ": bad grid sizes");
    NF_REQUIRE(in.z0 >= 0 && in.z1 >= in.z0 && tr.ntransect >= 0, NF_ERR_ARG, w + ": bad arguments");
    NF_REQUIRE(scratch_len >= (size_t)tr.ws->nrec * per_record, NF_ERR_ARG, w + ": scratch too small");
    return NF_OK;
}

// ---- depth-resolved rows: one value per level, straight from the raw fields -------------------------------------------
// A lane owns one record and up to LZ levels: the 40-byte record and the four arc lengths are read once per chunk, the
// 4 x LZ gathers of a lane (4 + 5 with a carried tracer, TR) are all in flight together; then level_slots_tf and weighted_sum
// per level and one seg_scan<LZ>.  runsum: (levels of the launch) x n doubles, level-major.
// The volume form takes no trailing argument, the carried-tracer form (row z = the tracer transport of level z alone) one
// TauIn<T>: TI is empty or TauIn<T>.  The volume form with per-cell thicknesses takes one ThickIn<T> instead: four more
// gathers per level, each slot's term with the thickness at its own face (level_th).
template <typename T, int LZ, typename... TI>
__global__ __launch_bounds__(kBlock) void k_profile_segscan(const int *__restrict__ cell, const double *__restrict__ w4,
                                                            const int *__restrict__ seg, long n, const T *__restrict__ u,
                                                            const T *__restrict__ v, long ncell, unsigned nx, int z0,
                                                            int nlev, const double *__restrict__ thickness,
                                                            const double *__restrict__ arcE,
                                                            const double *__restrict__ arcN, T fill, T fill2, int two,
                                                            double scale, int sverdrup, double *__restrict__ runsum,
                                                            TI... tracer)
{
    constexpr bool TR = (std::is_same<TI, TauIn<T>>::value || ...);
    constexpr bool CT = (std::is_same<TI, ThickIn<T>>::value || ...);
    const TauIn<T> ti = tau_in<T>(tracer...);
    const ThickIn<T> ct = thick_arg<T>(tracer...);
    const long k = (long)blockIdx.x * kBlock + threadIdx.x;
    double val[LZ];
#pragma unroll
    for (int l = 0; l < LZ; ++l) val[l] = 0.0;
    int key = -1;
    if (k < n) {
        const Record r = load_record(cell, w4, k);
        key = load_key(seg, k);
        const auto nb = step_neighbours<TR>(r.c, nx, ncell, ti.wrap_x);
        const Arcs arc = load_arcs(arcE, arcN, r.c, nb);
        LevelUV<T> x[LZ];
        LevelTau<T> tt[TR ? LZ : 1];
        LevelUV<T> e3[CT ? LZ : 1];
#pragma unroll
        for (int l = 0; l < LZ; ++l)
            if (l < nlev) {   // nlev is launch-uniform
                x[l] = load_level_uv(u, v, (long)(z0 + l) * ncell, r.c, nb);
                if constexpr (CT) e3[l] = load_level_e3(ct, (long)(z0 + l) * ncell, r.c, nb);
                if constexpr (TR) tt[l] = load_level_tau(ti.tau, (long)(z0 + l) * ncell, r.c, nb);
            }
#pragma unroll
        for (int l = 0; l < LZ; ++l)
            if (l < nlev) {
                FaceTf tf{};
                if constexpr (TR) tf = level_tf(tt[l], nb, ti);
                SlotTh th;
                if constexpr (CT)
                    th = level_th(e3[l], ct);
                else
                    th = slot_th(thickness[z0 + l]);
                val[l] = weighted_sum(r, level_slots_tf<T, TR>(th, x[l], arc, fill, fill2, two, scale, sverdrup, nb.south, tf));
            }
    }
    if (seg_scan(val, key, k, n)) {
#pragma unroll
        for (int l = 0; l < LZ; ++l)
            if (l < nlev) runsum[(long)l * n + k] = val[l];
    }
}


// FORM: 0 = volume, 1 = carried tracer, 2 = volume with per-cell thicknesses
template <typename T, int FORM>
static int launch_profile_t(const ProfileArgs &a, hipStream_t s)
{
    constexpr bool TR = FORM == 1;
    constexpr int chunk = FORM == 2 ? kCellThickProfileChunk
                                    : !TR ? kProfileChunk : sizeof(T) == 4 ? kTracerProfileChunkF32 : kTracerProfileChunk;
    const WeightSet &ws = *a.tr.ws;
    const StepInput &in = a.in;
    const long row_length = a.tr.row_length();
    const T fill = (T)in.fill, fill2 = (T)in.fill2;
    for (int zc = in.z0; zc < in.z1; zc += chunk) {
        const int nlev = in.z1 - zc < chunk ? in.z1 - zc : chunk;
        if (ws.nrec > 0) {
            if constexpr (TR)
                hipLaunchKernelGGL((k_profile_segscan<T, chunk, TauIn<T>>), record_grid(ws), dim3(kBlock), 0, s, ws.cell.get(),
                                   ws.w4.get(), ws.seg.get(), ws.nrec, (const T *)in.u, (const T *)in.v, in.ncell,
                                   (unsigned)in.nx, zc, nlev, in.thickness, in.arcE, in.arcN, fill, fill2,
                                   (int)uv_two_markers(fill, fill2), in.scale, in.sverdrup, a.scratch,
                                   tau_of<T>(a.t));
            else if constexpr (FORM == 2)
                hipLaunchKernelGGL((k_profile_segscan<T, chunk, ThickIn<T>>), record_grid(ws), dim3(kBlock), 0, s, ws.cell.get(),
                                   ws.w4.get(), ws.seg.get(), ws.nrec, (const T *)in.u, (const T *)in.v, in.ncell,
                                   (unsigned)in.nx, zc, nlev, in.thickness, in.arcE, in.arcN, fill, fill2,
                                   (int)uv_two_markers(fill, fill2), in.scale, in.sverdrup, a.scratch, thick_in<T>(a.th));
            else
                hipLaunchKernelGGL((k_profile_segscan<T, chunk>), record_grid(ws), dim3(kBlock), 0, s, ws.cell.get(),
                                   ws.w4.get(), ws.seg.get(), ws.nrec, (const T *)in.u, (const T *)in.v, in.ncell,
                                   (unsigned)in.nx, zc, nlev, in.thickness, in.arcE, in.arcN, fill, fill2,
                                   (int)uv_two_markers(fill, fill2), in.scale, in.sverdrup, a.scratch);
        }
        launch_finalize(a.tr, ws.seg_start.get(), ws.nrec, a.scratch, a.prof + (long)zc * row_length, row_length,
                        (unsigned)nlev, s);
        NF_HIP(hipGetLastError());
    }
    return NF_OK;
}

int launch_profile(const ProfileArgs &a, hipStream_t s)
{
    const bool tr = a.t.tau != nullptr, ct = a.th.e3u != nullptr;
    NF_REQUIRE(!(tr && ct), NF_ERR_STATE, "profile: the tracer profile does not take per-cell thicknesses");
    NF_REQUIRE(!ct || a.th.e3v, NF_ERR_ARG, "profile: null argument");
    NF_TRY(check_raw_step("profile", a.in, a.tr, a.scratch_len,
                          tr ? tracer_profile_chunk(a.in.dtype) : ct ? kCellThickProfileChunk : kProfileChunk));
    if (a.tr.row_length() == 0) return NF_OK;
    const int form = tr ? 1 : ct ? 2 : 0;
    if (a.in.dtype == NF_F64)
        return form == 1 ? launch_profile_t<double, 1>(a, s) : form == 2 ? launch_profile_t<double, 2>(a, s) : launch_profile_t<double, 0>(a, s);
    if (a.in.dtype == NF_F32)
        return form == 1 ? launch_profile_t<float, 1>(a, s) : form == 2 ? launch_profile_t<float, 2>(a, s) : launch_profile_t<float, 0>(a, s);
    NF_REQUIRE(false, NF_ERR_ARG, "profile: dtype must be NF_F64 or NF_F32");
}

// ---- section area and area-weighted tracer: two values per level, no velocity in them --------------------------------
// The rows that split a tracer transport into throughflow, overturning and gyre parts (nf_field_compute_area_profile): per
// level and slot  alpha = |w| * (th * arc)  where the face counts -- its velocity is present (uv_present: uv_fixed's
// comparison), the carried tracer has a finite face value x (tr_face_raw) and the slot is not row 0's south slot -- else 0, and
// beta = alpha * (x - ref).  No Sverdrup scale.  A lane owns one record and up to LZ levels, as in k_profile_segscan: the 4 + 5
// gathers per level (4 + 4 + 5 with per-cell thicknesses, one trailing ThickIn<T>) of the whole chunk are issued before the
// first is used, the four slots are added in weighted_sum's order, and the 2 * LZ sums go through ONE seg_scan.
// runsum: 2 * LZ rows of n doubles, level-major: rows [0, LZ) the areas, rows [LZ, 2 LZ) the tracer sums.
template <typename T>
__device__ inline bool uv_present(T x, T fill, T fill2, bool two)
{
    return !(x != x || x == fill || (two && x == fill2));
}
template <typename T>
__device__ inline void area_terms(const Record &r, const SlotTh &th, const LevelUV<T> &x, const Arcs &arc, T fill, T fill2,
                                  bool two, const LevelTau<T> &t, const ClassNeighbours &nb, const TauIn<T> &ti, double *area,
                                  double *tsum)
{
    double bs, be, bn, bw;
    auto term = [&](bool slot, double w, double th, T vel, double a, T ta, T tb, bool has_b, double *beta) {
        double f;
        const bool has = tr_face_raw<T>(ta, tb, has_b, ti.m1, ti.m2, &f);
        const bool counts = slot && has && __builtin_isfinite(f) && uv_present<T>(vel, fill, fill2, two);
        const double al = counts ? __builtin_fabs(w) * (th * a) : 0.0;
        *beta = counts ? al * (f - ti.ref) : 0.0;
        return al;
    };
    const double as = term(nb.south, r.wa.x, th.s, x.vs, arc.Ns, t.s, t.c, true, &bs);
    const double ae = term(true, r.wa.y, th.e, x.uc, arc.Ec, t.c, t.e, nb.has_e, &be);
    const double an = term(true, r.wb.x, th.n, x.vc, arc.Nc, t.c, t.n, nb.has_n, &bn);
    const double aw = term(true, r.wb.y, th.w, x.uw, arc.Ew, t.w, t.c, nb.has_w, &bw);
    *area = ((as + ae) + an) + aw;
    *tsum = ((bs + be) + bn) + bw;
}
// One slot's term of area_terms on its own, for the kernel that sends every slot to a row of its own (k_class_area_terms): the
// same expressions, so the same bits.  Returns whether the face counts; *face: the raw face value of the carried tracer (a
// value only where the face counts).
template <typename T>
__device__ inline bool area_slot(bool slot, double w, double th, T vel, double a, T ta, T tb, bool has_b, T fill, T fill2, bool two,
                                 const TauIn<T> &ti, double *alpha, double *beta, double *face)
{
    const bool has = tr_face_raw<T>(ta, tb, has_b, ti.m1, ti.m2, face);
    const bool counts = slot && has && __builtin_isfinite(*face) && uv_present<T>(vel, fill, fill2, two);
    const double al = counts ? __builtin_fabs(w) * (th * a) : 0.0;
    *alpha = al;
    *beta = counts ? al * (*face - ti.ref) : 0.0;
    return counts;
}

template <typename T, int LZ, typename... TI>
__global__ __launch_bounds__(kBlock) void k_area_segscan(const int *__restrict__ cell, const double *__restrict__ w4,
                                                         const int *__restrict__ seg, long n, const T *__restrict__ u,
                                                         const T *__restrict__ v, long ncell, unsigned nx, int z0, int nlev,
                                                         const double *__restrict__ thickness,
                                                         const double *__restrict__ arcE, const double *__restrict__ arcN,
                                                         T fill, T fill2, int two, TauIn<T> ti, double *__restrict__ runsum,
                                                         TI... thick)
{
    constexpr bool CT = sizeof...(TI) > 0;
    const ThickIn<T> ct = thick_arg<T>(thick...);
    const long k = (long)blockIdx.x * kBlock + threadIdx.x;
    double val[2 * LZ];
#pragma unroll
    for (int l = 0; l < 2 * LZ; ++l) val[l] = 0.0;
    int key = -1;
    if (k < n) {
        const Record r = load_record(cell, w4, k);
        key = load_key(seg, k);
        const ClassNeighbours nb = class_neighbours(r.c, nx, ncell, ti.wrap_x);
        const Arcs arc = load_arcs(arcE, arcN, r.c, nb);
        LevelUV<T> x[LZ];
        LevelTau<T> tt[LZ];
        LevelUV<T> e3[CT ? LZ : 1];
#pragma unroll
        for (int l = 0; l < LZ; ++l)
            if (l < nlev) {   // nlev is launch-uniform
                x[l] = load_level_uv(u, v, (long)(z0 + l) * ncell, r.c, nb);
                if constexpr (CT) e3[l] = load_level_e3(ct, (long)(z0 + l) * ncell, r.c, nb);
                tt[l] = load_level_tau(ti.tau, (long)(z0 + l) * ncell, r.c, nb);
            }
#pragma unroll
        for (int l = 0; l < LZ; ++l)
            if (l < nlev) {
                SlotTh th;
                if constexpr (CT)
                    th = level_th(e3[l], ct);
                else
                    th = slot_th(thickness[z0 + l]);
                area_terms<T>(r, th, x[l], arc, fill, fill2, two, tt[l], nb, ti, &val[l], &val[LZ + l]);
            }
    }
    if (seg_scan(val, key, k, n)) {
#pragma unroll
        for (int l = 0; l < LZ; ++l)
            if (l < nlev) {
                runsum[(long)l * n + k] = val[l];
                runsum[(long)(LZ + l) * n + k] = val[LZ + l];
            }
    }
}

// "area_chunk" tuning knob: the levels per chunk, one of the instantiated candidates of the dtype; 0 = area_chunk(dtype)
static int g_area_chunk = 0;
int area_chunk_set(int levels)
{
    if (levels != 0 && levels != 2 && levels != 4 && levels != 8) return -1;
    g_area_chunk = levels;
    return NF_OK;
}
int area_chunk_now(int dtype) { return g_area_chunk ? g_area_chunk : area_chunk(dtype); }

template <typename T, int LZ>
static int launch_area_t(const AreaArgs &a, hipStream_t s)
{
    const WeightSet &ws = *a.tr.ws;
    const StepInput &in = a.in;
    const long row_length = a.tr.row_length();
    const T fill = (T)in.fill, fill2 = (T)in.fill2;
    const TauIn<T> ti = tau_of<T>(a.t);
    double *tsum = a.scratch + (size_t)LZ * ws.nrec;   // the second half of the run sums
    for (int zc = in.z0; zc < in.z1; zc += LZ) {
        const int nlev = in.z1 - zc < LZ ? in.z1 - zc : LZ;
        if (ws.nrec > 0) {
            if (a.th.e3u)
                hipLaunchKernelGGL((k_area_segscan<T, LZ, ThickIn<T>>), record_grid(ws), dim3(kBlock), 0, s, ws.cell.get(),
                                   ws.w4.get(), ws.seg.get(), ws.nrec, (const T *)in.u, (const T *)in.v, in.ncell,
                                   (unsigned)in.nx, zc, nlev, in.thickness, in.arcE, in.arcN, fill, fill2,
                                   (int)uv_two_markers(fill, fill2), ti, a.scratch, thick_in<T>(a.th));
            else
                hipLaunchKernelGGL((k_area_segscan<T, LZ>), record_grid(ws), dim3(kBlock), 0, s, ws.cell.get(), ws.w4.get(),
                                   ws.seg.get(), ws.nrec, (const T *)in.u, (const T *)in.v, in.ncell, (unsigned)in.nx, zc, nlev,
                                   in.thickness, in.arcE, in.arcN, fill, fill2, (int)uv_two_markers(fill, fill2), ti, a.scratch);
        }
        launch_finalize(a.tr, ws.seg_start.get(), ws.nrec, a.scratch, a.rows + (long)zc * row_length, row_length, (unsigned)nlev,
                        s);
        launch_finalize(a.tr, ws.seg_start.get(), ws.nrec, tsum, a.rows + (a.nz + zc) * row_length, row_length, (unsigned)nlev,
                        s);
        NF_HIP(hipGetLastError());
    }
    return NF_OK;
}

int launch_area_profile(const AreaArgs &a, hipStream_t s)
{
    const StepInput &in = a.in;
    const int chunk = area_chunk_now(in.dtype);
    NF_REQUIRE(in.u && in.v && a.t.tau && a.rows && in.thickness && in.arcE && in.arcN, NF_ERR_ARG, "area profile: null argument");
    NF_REQUIRE(!a.th.e3u || a.th.e3v, NF_ERR_ARG, "area profile: null argument");
    NF_REQUIRE(in.z1 <= a.nz, NF_ERR_ARG, "area profile: bad arguments");
    NF_TRY(check_raw_step("area profile", in, a.tr, a.scratch_len, 2 * (size_t)chunk));
    if (a.tr.row_length() == 0) return NF_OK;
    if (in.dtype == NF_F64 && chunk == 2) return launch_area_t<double, 2>(a, s);
    if (in.dtype == NF_F64 && chunk == 4) return launch_area_t<double, 4>(a, s);
    if (in.dtype == NF_F32 && chunk == 4) return launch_area_t<float, 4>(a, s);
    if (in.dtype == NF_F32 && chunk == 8) return launch_area_t<float, 8>(a, s);
    NF_REQUIRE(in.dtype == NF_F64 || in.dtype == NF_F32, NF_ERR_ARG, "area profile: dtype must be NF_F64 or NF_F32");
    NF_REQUIRE(false, NF_ERR_ARG, "area profile: the area_chunk knob names a chunk that is not built for this dtype");
}

// ---- gross transports: the terms of a profile row, split by the direction of the water at their own slot ----------------
// The rows of nf_field_compute_gross_profile: per level and slot  q = w * d  with d of level_slots_tf<T, false> (the water) and
// the carried term  c = q  (volume form) or  c = w * d  with d of level_slots_tf<T, true> (carried form: TauIn<T> among the
// trailing arguments);  P = the sum of c over the slots with q > 0, N = over those with q < 0, a slot with q == 0 in neither.
// A lane owns one record and up to LZ levels, as in k_area_segscan: the 4 gathers per level (+ 5 with a carried tracer, + 4 with
// per-cell thicknesses, ThickIn<T> among the trailing arguments) of the whole chunk are issued before the first is used.  Both
// parts take all four slots in weighted_sum's order into +0.0, a slot that is not theirs as +0.0: the order of the additions
// does not depend on the signs, which is why negating uo / vo swaps and negates the parts bit for bit.  The 2 * LZ sums go
// through ONE seg_scan.  runsum: 2 * LZ rows of n doubles, level-major: rows [0, LZ) P, rows [LZ, 2 LZ) N.
template <typename T>
__device__ inline TauIn<T> tau_in(const TauIn<T> &ti, const ThickIn<T> &) { return ti; }
template <typename T>
__device__ inline ThickIn<T> thick_arg(const TauIn<T> &, const ThickIn<T> &ct) { return ct; }

// q, c: the water and carried terms of the four slots (weights applied), as Slots
__device__ inline Slots weighted_slots(const Record &r, const Slots &d)
{
    Slots t;
    t.s = r.wa.x * d.s, t.e = r.wa.y * d.e, t.n = r.wb.x * d.n, t.w = r.wb.y * d.w;
    return t;
}
__device__ inline void gross_terms(const Slots &q, const Slots &c, double *pos, double *neg)
{
    *pos = (((0.0 + (q.s > 0.0 ? c.s : 0.0)) + (q.e > 0.0 ? c.e : 0.0)) + (q.n > 0.0 ? c.n : 0.0)) + (q.w > 0.0 ? c.w : 0.0);
    *neg = (((0.0 + (q.s < 0.0 ? c.s : 0.0)) + (q.e < 0.0 ? c.e : 0.0)) + (q.n < 0.0 ? c.n : 0.0)) + (q.w < 0.0 ? c.w : 0.0);
}

template <typename T, int LZ, typename... TI>
__global__ __launch_bounds__(kBlock) void k_gross_segscan(const int *__restrict__ cell, const double *__restrict__ w4,
                                                          const int *__restrict__ seg, long n, const T *__restrict__ u,
                                                          const T *__restrict__ v, long ncell, unsigned nx, int z0, int nlev,
                                                          const double *__restrict__ thickness,
                                                          const double *__restrict__ arcE, const double *__restrict__ arcN,
                                                          T fill, T fill2, int two, double scale, int sverdrup,
                                                          double *__restrict__ runsum, TI... extra)
{
    constexpr bool TR = (std::is_same<TI, TauIn<T>>::value || ...);
    constexpr bool CT = (std::is_same<TI, ThickIn<T>>::value || ...);
    const TauIn<T> ti = tau_in<T>(extra...);
    const ThickIn<T> ct = thick_arg<T>(extra...);
    const long k = (long)blockIdx.x * kBlock + threadIdx.x;
    double val[2 * LZ];
#pragma unroll
    for (int l = 0; l < 2 * LZ; ++l) val[l] = 0.0;
    int key = -1;
    if (k < n) {
        const Record r = load_record(cell, w4, k);
        key = load_key(seg, k);
        const auto nb = step_neighbours<TR>(r.c, nx, ncell, ti.wrap_x);
        const Arcs arc = load_arcs(arcE, arcN, r.c, nb);
        LevelUV<T> x[LZ];
        LevelTau<T> tt[TR ? LZ : 1];
        LevelUV<T> e3[CT ? LZ : 1];
#pragma unroll
        for (int l = 0; l < LZ; ++l)
            if (l < nlev) {   // nlev is launch-uniform
                x[l] = load_level_uv(u, v, (long)(z0 + l) * ncell, r.c, nb);
                if constexpr (CT) e3[l] = load_level_e3(ct, (long)(z0 + l) * ncell, r.c, nb);
                if constexpr (TR) tt[l] = load_level_tau(ti.tau, (long)(z0 + l) * ncell, r.c, nb);
            }
#pragma unroll
        for (int l = 0; l < LZ; ++l)
            if (l < nlev) {
                SlotTh th;
                if constexpr (CT)
                    th = level_th(e3[l], ct);
                else
                    th = slot_th(thickness[z0 + l]);
                const Slots q = weighted_slots(
                    r, level_slots_tf<T, false>(th, x[l], arc, fill, fill2, two, scale, sverdrup, nb.south, FaceTf{}));
                Slots c = q;
                if constexpr (TR)
                    c = weighted_slots(r, level_slots_tf<T, true>(th, x[l], arc, fill, fill2, two, scale, sverdrup, nb.south,
                                                                  level_tf(tt[l], nb, ti)));
                gross_terms(q, c, &val[l], &val[LZ + l]);
            }
    }
    if (seg_scan(val, key, k, n)) {
#pragma unroll
        for (int l = 0; l < LZ; ++l)
            if (l < nlev) {
                runsum[(long)l * n + k] = val[l];
                runsum[(long)(LZ + l) * n + k] = val[LZ + l];
            }
    }
}

// "gross_chunk" tuning knob: the levels per chunk, one of the instantiated candidates of the dtype; 0 = gross_chunk(dtype,
// carried, cell)
static int g_gross_chunk = 0;
int gross_chunk_set(int levels)
{
    if (levels != 0 && levels != 2 && levels != 4 && levels != 8) return -1;
    g_gross_chunk = levels;
    return NF_OK;
}
int gross_chunk_now(int dtype, bool carried, bool cell)
{
    return g_gross_chunk ? g_gross_chunk : gross_chunk(dtype, carried, cell);
}

template <typename T, int LZ, typename... TI>
static int launch_gross_t(const GrossArgs &a, hipStream_t s, TI... extra)
{
    const WeightSet &ws = *a.tr.ws;
    const StepInput &in = a.in;
    const long row_length = a.tr.row_length();
    const T fill = (T)in.fill, fill2 = (T)in.fill2;
    double *nsum = a.scratch + (size_t)LZ * ws.nrec;   // the second half of the run sums
    for (int zc = in.z0; zc < in.z1; zc += LZ) {
        const int nlev = in.z1 - zc < LZ ? in.z1 - zc : LZ;
        if (ws.nrec > 0)
            hipLaunchKernelGGL((k_gross_segscan<T, LZ, TI...>), record_grid(ws), dim3(kBlock), 0, s, ws.cell.get(), ws.w4.get(),
                               ws.seg.get(), ws.nrec, (const T *)in.u, (const T *)in.v, in.ncell, (unsigned)in.nx, zc, nlev,
                               in.thickness, in.arcE, in.arcN, fill, fill2, (int)uv_two_markers(fill, fill2), in.scale,
                               in.sverdrup, a.scratch, extra...);
        launch_finalize(a.tr, ws.seg_start.get(), ws.nrec, a.scratch, a.rows + (long)zc * row_length, row_length, (unsigned)nlev,
                        s);
        launch_finalize(a.tr, ws.seg_start.get(), ws.nrec, nsum, a.rows + (a.nz + zc) * row_length, row_length, (unsigned)nlev,
                        s);
        NF_HIP(hipGetLastError());
    }
    return NF_OK;
}

// the four forms of one dtype: volume or carried tracer, each with the scalar or the per-cell thicknesses, as the trailing
// arguments of launch(...); the gross profile's, the depth bins' and the surface bins'
template <typename T, typename F>
static int launch_tracer_thick_form(const TracerIn &t, const CellThick &th, F launch)
{
    const TauIn<T> ti = tau_of<T>(t);
    if (t.tau && th.e3u) return launch(ti, thick_in<T>(th));
    if (t.tau) return launch(ti);
    if (th.e3u) return launch(thick_in<T>(th));
    return launch();
}

template <typename T, int LZ>
static int launch_gross_form(const GrossArgs &a, hipStream_t s)
{
    return launch_tracer_thick_form<T>(a.t, a.th, [&](auto... extra) { return launch_gross_t<T, LZ>(a, s, extra...); });
}

int launch_gross_profile(const GrossArgs &a, hipStream_t s)
{
    const StepInput &in = a.in;
    const int chunk = gross_chunk_now(in.dtype, a.t.tau != nullptr, a.th.e3u != nullptr);
    NF_REQUIRE(in.u && in.v && a.rows && in.thickness && in.arcE && in.arcN, NF_ERR_ARG, "gross profile: null argument");
    NF_REQUIRE(!a.th.e3u || a.th.e3v, NF_ERR_ARG, "gross profile: null argument");
    NF_REQUIRE(in.z1 <= a.nz, NF_ERR_ARG, "gross profile: bad arguments");
    NF_TRY(check_raw_step("gross profile", in, a.tr, a.scratch_len, 2 * (size_t)chunk));
    if (a.tr.row_length() == 0) return NF_OK;
    if (in.dtype == NF_F64 && chunk == 2) return launch_gross_form<double, 2>(a, s);
    if (in.dtype == NF_F64 && chunk == 4) return launch_gross_form<double, 4>(a, s);
    if (in.dtype == NF_F64 && chunk == 8) return launch_gross_form<double, 8>(a, s);
    if (in.dtype == NF_F32 && chunk == 4) return launch_gross_form<float, 4>(a, s);
    if (in.dtype == NF_F32 && chunk == 8) return launch_gross_form<float, 8>(a, s);
    NF_REQUIRE(in.dtype == NF_F64 || in.dtype == NF_F32, NF_ERR_ARG, "gross profile: dtype must be NF_F64 or NF_F32");
    NF_REQUIRE(false, NF_ERR_ARG, "gross profile: the gross_chunk knob names a chunk that is not built for this dtype");
}

// ---- crossings: the per-record, per-level values of the profile kernels, stored without a scan ------------------------------
// The planes of nf_field_compute_crossings.  A lane owns one record and up to LZ levels, as in k_area_segscan: the 4 gathers per
// level (+ 5 in the carried form, + 4 with per-cell thicknesses, one trailing ThickIn<T>) of the whole chunk are issued before
// the first is used.  Then, with the expressions of the profile kernels and hence their bits:
//   q  weighted_sum of level_slots_tf<T, false>          -- the record's term of k_profile_segscan's volume row
//   g  ((gs + ge) + gn) + gw, g_slot = |w| * (th * arc) where the slot's velocity is present (uv_present) and the slot is not
//      row 0's south slot, else 0                          -- volume form only: area_terms without its tracer condition
//   c  weighted_sum of level_slots_tf<T, true>           -- the record's term of the tracer profile / of P + N of the carried
//                                                             gross profile
//   a, b  area_terms' *area, *tsum                         -- the record's terms of k_area_segscan
// No Sverdrup scale in g, a, b.  Nothing crosses lanes: out[(p * nz + z) * n + k], consecutive lanes store consecutive doubles,
// every value is written once and not read again here (non-temporal).  `out` points at level z0 of plane 0.
template <typename T>
__device__ inline double present_area(const Record &r, const SlotTh &th, const LevelUV<T> &x, const Arcs &arc, T fill, T fill2,
                                      bool two, bool south)
{
    auto term = [&](bool slot, double w, double h, T vel, double a) {
        return slot && uv_present<T>(vel, fill, fill2, two) ? __builtin_fabs(w) * (h * a) : 0.0;
    };
    const double gs = term(south, r.wa.x, th.s, x.vs, arc.Ns);
    const double ge = term(true, r.wa.y, th.e, x.uc, arc.Ec);
    const double gn = term(true, r.wb.x, th.n, x.vc, arc.Nc);
    const double gw = term(true, r.wb.y, th.w, x.uw, arc.Ew);
    return ((gs + ge) + gn) + gw;
}

template <typename T, int LZ, bool CARRY, typename... TI>
__global__ __launch_bounds__(kBlock) void k_crossing_terms(const int *__restrict__ cell, const double *__restrict__ w4, long n,
                                                           const T *__restrict__ u, const T *__restrict__ v, long ncell,
                                                           unsigned nx, int z0, int nlev, const double *__restrict__ thickness,
                                                           const double *__restrict__ arcE, const double *__restrict__ arcN,
                                                           T fill, T fill2, int two, double scale, int sverdrup, TauIn<T> ti,
                                                           double *__restrict__ out, long plane, TI... thick)
{
    constexpr bool CT = sizeof...(TI) > 0;
    const ThickIn<T> ct = thick_arg<T>(thick...);
    const long k = (long)blockIdx.x * kBlock + threadIdx.x;
    if (k >= n) return;
    const Record r = load_record(cell, w4, k);
    const auto nb = step_neighbours<CARRY>(r.c, nx, ncell, ti.wrap_x);
    const Arcs arc = load_arcs(arcE, arcN, r.c, nb);
    LevelUV<T> x[LZ];
    LevelTau<T> tt[CARRY ? LZ : 1];
    LevelUV<T> e3[CT ? LZ : 1];
#pragma unroll
    for (int l = 0; l < LZ; ++l)
        if (l < nlev) {   // nlev is launch-uniform
            x[l] = load_level_uv(u, v, (long)(z0 + l) * ncell, r.c, nb);
            if constexpr (CT) e3[l] = load_level_e3(ct, (long)(z0 + l) * ncell, r.c, nb);
            if constexpr (CARRY) tt[l] = load_level_tau(ti.tau, (long)(z0 + l) * ncell, r.c, nb);
        }
#pragma unroll
    for (int l = 0; l < LZ; ++l)
        if (l < nlev) {
            SlotTh th;
            if constexpr (CT)
                th = level_th(e3[l], ct);
            else
                th = slot_th(thickness[z0 + l]);
            double *o = out + (long)l * n + k;
            const double q =
                weighted_sum(r, level_slots_tf<T, false>(th, x[l], arc, fill, fill2, two, scale, sverdrup, nb.south, FaceTf{}));
            __builtin_nontemporal_store(q, o);
            if constexpr (CARRY) {
                const double c = weighted_sum(r, level_slots_tf<T, true>(th, x[l], arc, fill, fill2, two, scale, sverdrup, nb.south,
                                                                         level_tf(tt[l], nb, ti)));
                double area, tsum;
                area_terms<T>(r, th, x[l], arc, fill, fill2, two, tt[l], nb, ti, &area, &tsum);
                __builtin_nontemporal_store(c, o + plane);
                __builtin_nontemporal_store(area, o + 2 * plane);
                __builtin_nontemporal_store(tsum, o + 3 * plane);
            } else {
                __builtin_nontemporal_store(present_area<T>(r, th, x[l], arc, fill, fill2, two, nb.south), o + plane);
            }
        }
}

// "crossing_chunk" tuning knob: the levels per chunk, one of the instantiated candidates; 0 = crossing_chunk(dtype, carried,
// cell)
static int g_crossing_chunk = 0;
int crossing_chunk_set(int levels)
{
    if (levels != 0 && levels != 2 && levels != 4 && levels != 8) return -1;
    g_crossing_chunk = levels;
    return NF_OK;
}
int crossing_chunk_now(int dtype, bool carried, bool cell)
{
    return g_crossing_chunk ? g_crossing_chunk : crossing_chunk(dtype, carried, cell);
}

template <typename T, int LZ, bool CARRY, typename... TI>
static int launch_crossing_t(const CrossingArgs &a, hipStream_t s, TI... thick)
{
    const WeightSet &ws = *a.ws;
    const StepInput &in = a.in;
    const T fill = (T)in.fill, fill2 = (T)in.fill2;
    const long plane = a.nz * ws.nrec;
    for (int zc = in.z0; zc < in.z1; zc += LZ) {
        const int nlev = in.z1 - zc < LZ ? in.z1 - zc : LZ;
        hipLaunchKernelGGL((k_crossing_terms<T, LZ, CARRY, TI...>), record_grid(ws), dim3(kBlock), 0, s, ws.cell.get(), ws.w4.get(),
                           ws.nrec, (const T *)in.u, (const T *)in.v, in.ncell, (unsigned)in.nx, zc, nlev, in.thickness, in.arcE,
                           in.arcN, fill, fill2, (int)uv_two_markers(fill, fill2), in.scale, in.sverdrup, tau_of<T>(a.t),
                           a.out + (long)zc * ws.nrec, plane, thick...);
        NF_HIP(hipGetLastError());
    }
    return NF_OK;
}

// the four forms of one dtype and chunk: volume or carried, each with the scalar or the per-cell thicknesses
template <typename T, int LZ>
static int launch_crossing_form(const CrossingArgs &a, hipStream_t s)
{
    if (a.t.tau && a.th.e3u) return launch_crossing_t<T, LZ, true>(a, s, thick_in<T>(a.th));
    if (a.t.tau) return launch_crossing_t<T, LZ, true>(a, s);
    if (a.th.e3u) return launch_crossing_t<T, LZ, false>(a, s, thick_in<T>(a.th));
    return launch_crossing_t<T, LZ, false>(a, s);
}

int launch_crossing_terms(const CrossingArgs &a, hipStream_t s)
{
    const StepInput &in = a.in;
    const int chunk = crossing_chunk_now(in.dtype, a.t.tau != nullptr, a.th.e3u != nullptr);
    NF_REQUIRE(a.ws && in.u && in.v && in.thickness && in.arcE && in.arcN, NF_ERR_ARG, "crossings: null argument");
    NF_REQUIRE(!a.th.e3u || a.th.e3v, NF_ERR_ARG, "crossings: null argument");
    NF_REQUIRE(in.ncell > 0 && in.nx > 0 && in.ncell % in.nx == 0 && in.ncell < (1l << 31), NF_ERR_ARG, "crossings: bad grid sizes");
    NF_REQUIRE(in.z0 >= 0 && in.z1 >= in.z0 && in.z1 <= a.nz, NF_ERR_ARG, "crossings: bad arguments");
    if (a.ws->nrec == 0) return NF_OK;
    NF_REQUIRE(a.out, NF_ERR_ARG, "crossings: null argument");
    NF_REQUIRE(in.dtype == NF_F64 || in.dtype == NF_F32, NF_ERR_ARG, "crossings: dtype must be NF_F64 or NF_F32");
    if (in.dtype == NF_F64 && chunk == 2) return launch_crossing_form<double, 2>(a, s);
    if (in.dtype == NF_F64 && chunk == 4) return launch_crossing_form<double, 4>(a, s);
    if (in.dtype == NF_F64 && chunk == 8) return launch_crossing_form<double, 8>(a, s);
    if (in.dtype == NF_F32 && chunk == 2) return launch_crossing_form<float, 2>(a, s);
    if (in.dtype == NF_F32 && chunk == 4) return launch_crossing_form<float, 4>(a, s);
    if (in.dtype == NF_F32 && chunk == 8) return launch_crossing_form<float, 8>(a, s);
    NF_REQUIRE(false, NF_ERR_ARG, "crossings: the crossing_chunk knob names a chunk that is not built");
}

// ---- volume transport in tracer classes: level_slots, each term sent to the row of its face's class -------------------
// One lane per record, K3's record order and 64-record waves.  Per owned level (z ascending) the four slot terms are
// level_slots' times their weights; each is added, in slot order (south, east, north, west), to the lane's accumulator of the
// row that its own face's class value selects (class_row), when that row lies in the window [r0, r0 + nwin): window_lds,
// window_add and window_scan_store, the window pieces above.  With one class per level (tau = z) a row gets exactly one
// level's four terms, added as ((0 + t0) + t1) + t2) + t3: weighted_sum's ((t0 + t1) + t2) + t3, bit for bit.
//   faces: east(c) = (tau[c], tau[c+1]; column nx-1: tau[c+1-nx] when wrap_x, else none), north(c) = (tau[c], tau[c+nx];
//   last row: none), the west slot is east(cw), the south slot north(cs).
// CARRY: the carried-tracer form, every term times tr_face of the carried tracer at its own face (level_slots_tf).  TWO: the
// class field and the carried tracer are different arrays (5 more gathers per level); otherwise the one set of values serves
// both.
constexpr int kClassLevels = 4;        // levels whose 9 gathers are issued together (volume form, one-tracer carry form)
constexpr int kClassLevelsTwo = 4;     // ... whose 14 gathers are (carry form with a class field of its own)

// row of class value x among the n edges in LDS: the number of edges <= x (binary lifting, `top` = the largest power of two
// <= n: the same number of steps in every lane); no value or NaN: row n + 1
__device__ inline int class_row(bool has, double x, const double *e, int n, int top)
{
    if (!has || x != x) return n + 1;
    int pos = 0;
    for (int step = top; step > 0; step >>= 1)
        if (pos + step <= n && e[pos + step - 1] <= x) pos += step;
    return pos;
}

// TI: empty (volume form; TWO = false) or TauIn<T>, the carried tracer; tau, tfill, tfill2 are the class field's
template <typename T, bool TWO, typename... TI>
__global__ __launch_bounds__(kBlock) void k_class_segscan(const int *__restrict__ cell, const double *__restrict__ w4,
                                                          const int *__restrict__ seg, long n, const T *__restrict__ u,
                                                          const T *__restrict__ v, const T *__restrict__ tau, long ncell,
                                                          unsigned nx, int z0, int z1, const double *__restrict__ thickness,
                                                          const double *__restrict__ arcE, const double *__restrict__ arcN,
                                                          T fill, T fill2, int two, T tfill, T tfill2, int wrap_x,
                                                          double scale, int sverdrup, const double *__restrict__ edges,
                                                          int nedges, int top, int r0, int nwin, double *__restrict__ runsum,
                                                          TI... tracer)
{
    constexpr bool CARRY = sizeof...(TI) > 0;
    constexpr int CL = TWO ? kClassLevelsTwo : kClassLevels;
    const TauIn<T> ti = tau_in<T>(tracer...);
    const WindowLds w = window_lds(edges, nedges, nwin);
    const long k = (long)blockIdx.x * kBlock + threadIdx.x;
    const int lane = threadIdx.x & (kWave - 1);
    int key = -1;
    if (k < n) {
        const Record r = load_record(cell, w4, k);
        key = load_key(seg, k);
        const ClassNeighbours nb = class_neighbours(r.c, nx, ncell, wrap_x);
        const Arcs arc = load_arcs(arcE, arcN, r.c, nb);
        // x to the row of the face value f (has: the face has one)
        auto add = [&](bool has, double f, double x) { window_add<kBlock>(w.acc, class_row(has, f, w.e, nedges, top), r0, nwin, x); };
        for (int z = z0; z < z1; z += CL) {
            const int nlev = z1 - z < CL ? z1 - z : CL;
            LevelUV<T> x[CL];
            T tc[CL], te[CL], tn[CL], tw[CL], ts[CL];   // the class field
            LevelTau<T> tt[TWO ? CL : 1];               // the carried tracer, when it is another array
#pragma unroll
            for (int l = 0; l < CL; ++l)
                if (l < nlev) {
                    const long o = (long)(z + l) * ncell;
                    x[l] = load_level_uv(u, v, o, r.c, nb);
                    tc[l] = tau[o + r.c];
                    te[l] = tau[o + nb.ce];
                    tn[l] = tau[o + nb.cn];
                    tw[l] = tau[o + nb.cw];
                    ts[l] = tau[o + nb.cs];
                    if constexpr (TWO) tt[l] = load_level_tau(ti.tau, o, r.c, nb);
                }
#pragma unroll
            for (int l = 0; l < CL; ++l)
                if (l < nlev) {
                    FaceTf tf{};
                    if constexpr (CARRY) tf = level_tf(TWO ? tt[l] : LevelTau<T>{tc[l], te[l], tn[l], tw[l], ts[l]}, nb, ti);
                    const Slots d = level_slots_tf<T, CARRY>(slot_th(thickness[z + l]), x[l], arc, fill, fill2, two, scale, sverdrup,
                                                             nb.south, tf);
                    double f;
                    bool h;
                    if (nb.south) {
                        h = tr_face_raw<T>(ts[l], tc[l], true, tfill, tfill2, &f);
                        add(h, f, r.wa.x * d.s);
                    }
                    h = tr_face_raw<T>(tc[l], te[l], nb.has_e, tfill, tfill2, &f);
                    add(h, f, r.wa.y * d.e);
                    h = tr_face_raw<T>(tc[l], tn[l], nb.has_n, tfill, tfill2, &f);
                    add(h, f, r.wb.x * d.n);
                    h = tr_face_raw<T>(tw[l], tc[l], nb.has_w, tfill, tfill2, &f);
                    add(h, f, r.wb.y * d.w);
                }
        }
    }
    window_scan_store<kBlock>(w.acc, key, lane, k, n, nwin, runsum);
}

// ---- conservative (piecewise-linear) remapping of the class transport -----------------------------------------------------
// k_class_segscan with another rule for the row: the class field is taken to vary linearly between the interfaces of a layer,
// and a term is spread uniformly in class space over the interval between its face's two interface values
//   g_up = 0.5 (f[z-1] + f[z]) where z > 0 and the face has a value at level z - 1, else f[z];  g_dn likewise with z + 1 < nz;
// row j gets the share of [lo, hi] = [min, max](g_up, g_dn) that lies in it (spread_span).  Whole to class_row(f[z]) (the
// step rule) where g_up, g_dn or their difference is not finite, whole to class_row(lo) where lo == hi, whole to row
// nedges + 1 without a class value: these fallbacks are this kernel's own, not make_span's.  Per lane the adds run
// level-ascending, then in slot order, then row-ascending.  Levels z - 1 and z + 1 are levels of the ARRAY (nz of them), not of
// the owned range: the first and the last owned level read one halo level each.
// The class field's five gathers are issued once per level: c[] is a rolling window of levels z - 1 .. z + RL whose first two
// members come from the batch before.
constexpr int kRemapLevels = 4;        // levels whose 9 gathers are issued together (volume form, one-tracer carry form)
constexpr int kRemapLevelsTwo = 2;     // ... whose 14 gathers are (carry form with a class field of its own)

// The row rule above for one term, shared by k_class_remap_segscan and k_gross_remap_segscan: the window of a lane, the class
// field's markers and the edges.  spread: the term t of the face (a, b) at a level whose class values are (a1, b1), with
// (a0, b0) above and (a2, b2) below (up, dn: the array has that level).
template <typename T>
struct RemapRows {
    WindowLds w;
    T tfill, tfill2;
    int nedges, top, r0, nwin;
    __device__ void add(int row, double x) const { window_add<kBlock>(w.acc, row, r0, nwin, x); }
    __device__ int row(double x) const { return class_row(true, x, w.e, nedges, top); }
    __device__ void spread(T a0, T b0, T a1, T b1, T a2, T b2, bool has_b, bool up, bool dn, double t) const
    {
        double f, fu = 0.0, fd = 0.0;
        const bool h = tr_face_raw<T>(a1, b1, has_b, tfill, tfill2, &f);
        if (!h || f != f) return add(nedges + 1, t);
        const bool hu = up && tr_face_raw<T>(a0, b0, has_b, tfill, tfill2, &fu);
        const bool hd = dn && tr_face_raw<T>(a2, b2, has_b, tfill, tfill2, &fd);
        const double gu = hu ? 0.5 * (fu + f) : f, gd = hd ? 0.5 * (fd + f) : f;
        if (!(__builtin_isfinite(gu) && __builtin_isfinite(gd) && __builtin_isfinite(gd - gu))) return add(row(f), t);
        const double lo = gu < gd ? gu : gd, hi = gu < gd ? gd : gu;
        const int jlo = row(lo);
        if (lo == hi) return add(jlo, t);
        spread_span<kBlock, 1>(w.acc, w.e, RowSpan{lo, hi, jlo, row(hi)}, t, r0, r0 + nwin - 1);
    }
};

template <typename T, bool TWO, typename... TI>
__global__ __launch_bounds__(kBlock) void k_class_remap_segscan(const int *__restrict__ cell, const double *__restrict__ w4,
                                                                const int *__restrict__ seg, long n, const T *__restrict__ u,
                                                                const T *__restrict__ v, const T *__restrict__ tau, long ncell,
                                                                unsigned nx, int z0, int z1,
                                                                const double *__restrict__ thickness,
                                                                const double *__restrict__ arcE,
                                                                const double *__restrict__ arcN, T fill, T fill2, int two,
                                                                T tfill, T tfill2, int wrap_x, double scale, int sverdrup,
                                                                const double *__restrict__ edges, int nedges, int top, int r0,
                                                                int nwin, double *__restrict__ runsum, int nz, TI... tracer)
{
    constexpr bool CARRY = sizeof...(TI) > 0;
    constexpr int RL = TWO ? kRemapLevelsTwo : kRemapLevels;
    const TauIn<T> ti = tau_in<T>(tracer...);
    const WindowLds w = window_lds(edges, nedges, nwin);
    const long k = (long)blockIdx.x * kBlock + threadIdx.x;
    const int lane = threadIdx.x & (kWave - 1);
    int key = -1;
    if (k < n) {   // z0 < z1 <= nz: the launcher's
        const Record r = load_record(cell, w4, k);
        key = load_key(seg, k);
        const ClassNeighbours nb = class_neighbours(r.c, nx, ncell, wrap_x);
        const Arcs arc = load_arcs(arcE, arcN, r.c, nb);
        const RemapRows<T> rows{w, tfill, tfill2, nedges, top, r0, nwin};
        auto spread = [&](auto... a) { rows.spread(a...); };
        LevelTau<T> c[RL + 2];   // the class field of levels z - 1 .. z + RL
        c[1] = load_level_tau(tau, (long)z0 * ncell, r.c, nb);
        c[0] = z0 > 0 ? load_level_tau(tau, (long)(z0 - 1) * ncell, r.c, nb) : c[1];
        for (int z = z0; z < z1; z += RL) {
            const int nlev = z1 - z < RL ? z1 - z : RL;
            LevelUV<T> x[RL];
            LevelTau<T> tt[TWO ? RL : 1];               // the carried tracer, when it is another array
#pragma unroll
            for (int l = 0; l < RL; ++l)
                if (l < nlev) {
                    const long o = (long)(z + l) * ncell;
                    x[l] = load_level_uv(u, v, o, r.c, nb);
                    c[l + 2] = z + l + 1 < nz ? load_level_tau(tau, o + ncell, r.c, nb) : c[l + 1];
                    if constexpr (TWO) tt[l] = load_level_tau(ti.tau, o, r.c, nb);
                }
#pragma unroll
            for (int l = 0; l < RL; ++l)
                if (l < nlev) {
                    const LevelTau<T> &p = c[l], &m = c[l + 1], &q = c[l + 2];
                    const bool up = z + l > 0, dn = z + l + 1 < nz;
                    FaceTf tf{};
                    if constexpr (CARRY) tf = level_tf(TWO ? tt[l] : m, nb, ti);
                    const Slots d = level_slots_tf<T, CARRY>(slot_th(thickness[z + l]), x[l], arc, fill, fill2, two, scale, sverdrup,
                                                             nb.south, tf);
                    if (nb.south) spread(p.s, p.c, m.s, m.c, q.s, q.c, true, up, dn, r.wa.x * d.s);
                    spread(p.c, p.e, m.c, m.e, q.c, q.e, nb.has_e, up, dn, r.wa.y * d.e);
                    spread(p.c, p.n, m.c, m.n, q.c, q.n, nb.has_n, up, dn, r.wb.x * d.n);
                    spread(p.w, p.c, m.w, m.c, q.w, q.c, nb.has_w, up, dn, r.wb.y * d.w);
                }
            c[0] = c[RL];
            c[1] = c[RL + 1];
        }
    }
    window_scan_store<kBlock>(w.acc, key, lane, k, n, nwin, runsum);
}

// same bits of two doubles (NaN included): the markers of two tracer slots agree
static bool same_bits(double a, double b) { return __builtin_memcmp(&a, &b, sizeof a) == 0; }

// ---- the host side of the windowed rows ----
// class_top: the largest power of two <= nedges, class_row's first step.  class_lds_bytes: window_lds' layout.
static int class_top(int nedges)
{
    int top = 1;
    while (2 * top <= nedges) top *= 2;
    return top;
}
static size_t class_lds_bytes(int nedges, int nwin) { return sizeof(double) * ((size_t)((nedges + 1) & ~1) + (size_t)nwin * kBlock); }

// a launch with `lds` bytes of dynamic LDS: above 64 KiB the kernel's limit is raised first
template <typename K, typename... A>
static int launch_lds(K kernel, dim3 grid, dim3 block, size_t lds, hipStream_t s, A... args)
{
    if (lds > 65536)
        NF_HIP(hipFuncSetAttribute(reinterpret_cast<const void *>(kernel), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
    hipLaunchKernelGGL(kernel, grid, block, lds, s, args...);
    return NF_OK;
}

// The passes over `nrows` rows, `window` rows at a time: pass(r0, nwin, win) launches the kernel that leaves the run sums of
// rows [r0, r0 + nwin), window number `win`, in `scratch` (not called without records); each pass is finalized into its rows
// of `rows` (nrows, row_length).
template <typename F>
static int for_each_window(const Transects &tr, int nrows, int window, double *scratch, double *rows, hipStream_t s, F pass)
{
    const WeightSet &ws = *tr.ws;
    const long row_length = tr.row_length();
    for (int r0 = 0, win = 0; r0 < nrows; r0 += window, ++win) {
        const int nwin = nrows - r0 < window ? nrows - r0 : window;
        if (ws.nrec > 0) NF_TRY(pass(r0, nwin, win));
        launch_finalize(tr, ws.seg_start.get(), ws.nrec, scratch, rows + (long)r0 * row_length, row_length, (unsigned)nwin, s);
        NF_HIP(hipGetLastError());
    }
    return NF_OK;
}

// k_class_segscan or (REMAP) k_class_remap_segscan over the windows.  FORM: 0 = volume, 1 = carried tracer that is the class
// field, 2 = carried tracer and a class field of its own.  The kernel of the form takes trailing arguments of its own: the
// array's levels (REMAP), then the carried tracer (FORM > 0).
template <typename T, int FORM, bool REMAP>
static int launch_class_t(const ClassArgs &a, hipStream_t s)
{
    const WeightSet &ws = *a.tr.ws;
    const StepInput &in = a.in;
    const T fill = (T)in.fill, fill2 = (T)in.fill2;
    const int top = class_top(a.nedges), wrap_x = a.cls.wrap_x ? 1 : 0;
    // the carried tracer with the class field's wrap rule; empty and not passed in the volume form (FORM == 0)
    const TauIn<T> carry{(const T *)a.carry.tau, (T)a.carry.fill, (T)a.carry.fill2, a.carry.ref, wrap_x};
    return for_each_window(a.tr, a.nedges + 2, a.window, a.scratch, a.rows, s, [&](int r0, int nwin, int) {
        // the arguments that the two kernels share, then `tail` in the kernel's own order: remap_nz first, carry last
        auto launch = [&](auto kernel, auto... tail) {
            return launch_lds(kernel, record_grid(ws), dim3(kBlock), class_lds_bytes(a.nedges, nwin), s, ws.cell.get(), ws.w4.get(),
                              ws.seg.get(), ws.nrec, (const T *)in.u, (const T *)in.v, (const T *)a.cls.tau, in.ncell, (unsigned)in.nx,
                              in.z0, in.z1, in.thickness, in.arcE, in.arcN, fill, fill2, (int)uv_two_markers(fill, fill2),
                              (T)a.cls.fill, (T)a.cls.fill2, wrap_x, in.scale, in.sverdrup, a.edges, a.nedges, top, r0, nwin,
                              a.scratch, tail...);
        };
        if constexpr (REMAP && FORM == 0) return launch(&k_class_remap_segscan<T, false>, a.remap_nz);
        if constexpr (REMAP && FORM > 0) return launch(&k_class_remap_segscan<T, FORM == 2, TauIn<T>>, a.remap_nz, carry);
        if constexpr (!REMAP && FORM == 0) return launch(&k_class_segscan<T, false>);
        if constexpr (!REMAP && FORM > 0) return launch(&k_class_segscan<T, FORM == 2, TauIn<T>>, carry);
    });
}

template <typename T, bool REMAP>
static int launch_class_form(const ClassArgs &a, hipStream_t s)
{
    if (!a.carry.tau) return launch_class_t<T, 0, REMAP>(a, s);
    const bool one = a.carry.tau == a.cls.tau && same_bits(a.carry.fill, a.cls.fill) && same_bits(a.carry.fill2, a.cls.fill2);
    return one ? launch_class_t<T, 1, REMAP>(a, s) : launch_class_t<T, 2, REMAP>(a, s);
}

int launch_class_transport(const ClassArgs &a, hipStream_t s)
{
    const StepInput &in = a.in;
    NF_REQUIRE(a.nedges >= 2 && a.nedges <= kMaxClassEdges && a.edges, NF_ERR_ARG, "class transport: bad class edges");
    NF_REQUIRE(a.window >= 1 && a.window <= kClassWindowMax, NF_ERR_ARG, "class transport: bad window");
    NF_TRY(check_raw_step("class transport", in, a.tr, a.scratch_len, (size_t)a.window));
    NF_REQUIRE(in.u && in.v && a.cls.tau && a.rows && in.thickness && in.arcE && in.arcN, NF_ERR_ARG,
               "class transport: null argument");
    if (a.tr.row_length() == 0) return NF_OK;
    if (in.dtype == NF_F64) return launch_class_form<double, false>(a, s);
    if (in.dtype == NF_F32) return launch_class_form<float, false>(a, s);
    NF_REQUIRE(false, NF_ERR_ARG, "class transport: dtype must be NF_F64 or NF_F32");
}

// a.remap_nz: the levels of the arrays; the checks are launch_class_transport's
int launch_class_remap(const ClassArgs &a, hipStream_t s)
{
    const StepInput &in = a.in;
    NF_REQUIRE(a.nedges >= 2 && a.nedges <= kMaxClassEdges && a.edges, NF_ERR_ARG, "class remap: bad class edges");
    NF_REQUIRE(a.window >= 1 && a.window <= kClassWindowMax, NF_ERR_ARG, "class remap: bad window");
    NF_TRY(check_raw_step("class remap", in, a.tr, a.scratch_len, (size_t)a.window));
    NF_REQUIRE(in.u && in.v && a.cls.tau && a.rows && in.thickness && in.arcE && in.arcN, NF_ERR_ARG, "class remap: null argument");
    NF_REQUIRE(in.z0 < in.z1 && in.z1 <= a.remap_nz, NF_ERR_ARG, "class remap: bad levels");
    if (a.tr.row_length() == 0) return NF_OK;
    if (in.dtype == NF_F64) return launch_class_form<double, true>(a, s);
    if (in.dtype == NF_F32) return launch_class_form<float, true>(a, s);
    NF_REQUIRE(false, NF_ERR_ARG, "class remap: dtype must be NF_F64 or NF_F32");
}

// ---- remapped gross (inflow / outflow) class transports: the gross class terms under the remap kernel's row rule -------------
// Where k_gross_class_terms and k_class_remap_segscan cross.  Per (record, owned level, slot) the water term q = w * d and the
// carried term c (= q in the volume form, w * d^tau with a TauIn<T> among the trailing arguments) are k_gross_class_terms'
// (weighted_slots of level_slots_tf<T, false> / <T, true>; with a ThickIn<T> among the trailing arguments the thickness at the
// slot's own face, level_th); c is spread over the class rows by RemapRows::spread from the rolling class-field window c[] of
// k_class_remap_segscan.  `part` picks the terms of a launch: 0 = P, the slots with q > 0; 1 = N, those with q < 0; a slot with
// q == 0 or NaN (row 0's south slot among them) is in neither.  The rows of a part are n + 2 window rows of their own, so no
// window straddles the parts and a lane's adds to a row run level-ascending, then in slot order, then row-ascending, from
// +0.0: skipping the other part's terms leaves the order of the kept ones alone, which is why negating uo / vo swaps and
// negates the parts bit for bit.  TWO: the carried tracer is another array than the class field (5 more gathers per level).
// Levels whose gathers are issued together: 4 (volume and one-tracer forms: 9 per level, 13 with per-cell thicknesses), 2 with
// a class field of its own (14, 18).
constexpr int kGrossRemapLevels = 4;
constexpr int kGrossRemapLevelsTwo = 2;

template <typename T, bool TWO, typename... TI>
__global__ __launch_bounds__(kBlock) void k_gross_remap_segscan(const int *__restrict__ cell, const double *__restrict__ w4,
                                                                const int *__restrict__ seg, long n, const T *__restrict__ u,
                                                                const T *__restrict__ v, const T *__restrict__ tau, long ncell,
                                                                unsigned nx, int z0, int z1,
                                                                const double *__restrict__ thickness,
                                                                const double *__restrict__ arcE,
                                                                const double *__restrict__ arcN, T fill, T fill2, int two,
                                                                T tfill, T tfill2, int wrap_x, double scale, int sverdrup,
                                                                const double *__restrict__ edges, int nedges, int top, int r0,
                                                                int nwin, double *__restrict__ runsum, int nz, int part,
                                                                TI... extra)
{
    constexpr bool CARRY = (std::is_same<TI, TauIn<T>>::value || ...);
    constexpr bool CT = (std::is_same<TI, ThickIn<T>>::value || ...);
    constexpr int RL = TWO ? kGrossRemapLevelsTwo : kGrossRemapLevels;
    static_assert(CARRY || !TWO, "a class field of its own needs a carried tracer");
    const TauIn<T> ti = tau_in<T>(extra...);
    const ThickIn<T> ct = thick_arg<T>(extra...);
    const WindowLds w = window_lds(edges, nedges, nwin);
    const long k = (long)blockIdx.x * kBlock + threadIdx.x;
    const int lane = threadIdx.x & (kWave - 1);
    int key = -1;
    if (k < n) {   // z0 < z1 <= nz: the launcher's
        const Record r = load_record(cell, w4, k);
        key = load_key(seg, k);
        const ClassNeighbours nb = class_neighbours(r.c, nx, ncell, wrap_x);
        const Arcs arc = load_arcs(arcE, arcN, r.c, nb);
        const RemapRows<T> rows{w, tfill, tfill2, nedges, top, r0, nwin};
        auto mine = [&](double q) { return part ? q < 0.0 : q > 0.0; };
        LevelTau<T> c[RL + 2];   // the class field of levels z - 1 .. z + RL
        c[1] = load_level_tau(tau, (long)z0 * ncell, r.c, nb);
        c[0] = z0 > 0 ? load_level_tau(tau, (long)(z0 - 1) * ncell, r.c, nb) : c[1];
        for (int z = z0; z < z1; z += RL) {
            const int nlev = z1 - z < RL ? z1 - z : RL;
            LevelUV<T> x[RL];
            LevelUV<T> e3[CT ? RL : 1];
            LevelTau<T> tt[TWO ? RL : 1];               // the carried tracer, when it is another array
#pragma unroll
            for (int l = 0; l < RL; ++l)
                if (l < nlev) {
                    const long o = (long)(z + l) * ncell;
                    x[l] = load_level_uv(u, v, o, r.c, nb);
                    if constexpr (CT) e3[l] = load_level_e3(ct, o, r.c, nb);
                    c[l + 2] = z + l + 1 < nz ? load_level_tau(tau, o + ncell, r.c, nb) : c[l + 1];
                    if constexpr (TWO) tt[l] = load_level_tau(ti.tau, o, r.c, nb);
                }
#pragma unroll
            for (int l = 0; l < RL; ++l)
                if (l < nlev) {
                    const LevelTau<T> &p = c[l], &m = c[l + 1], &d = c[l + 2];
                    const bool up = z + l > 0, dn = z + l + 1 < nz;
                    SlotTh th;
                    if constexpr (CT)
                        th = level_th(e3[l], ct);
                    else
                        th = slot_th(thickness[z + l]);
                    const Slots q = weighted_slots(
                        r, level_slots_tf<T, false>(th, x[l], arc, fill, fill2, two, scale, sverdrup, nb.south, FaceTf{}));
                    Slots t = q;
                    if constexpr (CARRY)
                        t = weighted_slots(r, level_slots_tf<T, true>(th, x[l], arc, fill, fill2, two, scale, sverdrup, nb.south,
                                                                      level_tf(TWO ? tt[l] : m, nb, ti)));
                    if (nb.south && mine(q.s)) rows.spread(p.s, p.c, m.s, m.c, d.s, d.c, true, up, dn, t.s);
                    if (mine(q.e)) rows.spread(p.c, p.e, m.c, m.e, d.c, d.e, nb.has_e, up, dn, t.e);
                    if (mine(q.n)) rows.spread(p.c, p.n, m.c, m.n, d.c, d.n, nb.has_n, up, dn, t.n);
                    if (mine(q.w)) rows.spread(p.w, p.c, m.w, m.c, d.w, d.c, nb.has_w, up, dn, t.w);
                }
            c[0] = c[RL];
            c[1] = c[RL + 1];
        }
    }
    window_scan_store<kBlock>(w.acc, key, lane, k, n, nwin, runsum);
}

// P then N: one for_each_window loop per part over its n + 2 rows, `rows + part * (n + 2) * row_length`.  extra: the carried
// tracer (TWO or not), then the per-cell thicknesses, each where the form has one.
template <typename T, bool TWO, typename... TI>
static int launch_gross_remap_t(const GrossRemapArgs &a, hipStream_t s, TI... extra)
{
    const WeightSet &ws = *a.tr.ws;
    const StepInput &in = a.in;
    const T fill = (T)in.fill, fill2 = (T)in.fill2;
    const int top = class_top(a.nedges), wrap_x = a.cls.wrap_x ? 1 : 0, nrows = a.nedges + 2;
    for (int part = 0; part < 2; ++part)
        NF_TRY(for_each_window(a.tr, nrows, a.window, a.scratch, a.rows + (long)part * nrows * a.tr.row_length(), s,
                               [&](int r0, int nwin, int) {
            return launch_lds(&k_gross_remap_segscan<T, TWO, TI...>, record_grid(ws), dim3(kBlock),
                              class_lds_bytes(a.nedges, nwin), s, ws.cell.get(), ws.w4.get(), ws.seg.get(), ws.nrec, (const T *)in.u,
                              (const T *)in.v, (const T *)a.cls.tau, in.ncell, (unsigned)in.nx, in.z0, in.z1, in.thickness, in.arcE,
                              in.arcN, fill, fill2, (int)uv_two_markers(fill, fill2), (T)a.cls.fill, (T)a.cls.fill2, wrap_x,
                              in.scale, in.sverdrup, a.edges, a.nedges, top, r0, nwin, a.scratch, a.nz, part, extra...);
        }));
    return NF_OK;
}

template <typename T>
static int launch_gross_remap_form(const GrossRemapArgs &a, hipStream_t s)
{
    const bool one = a.carry.tau == a.cls.tau && same_bits(a.carry.fill, a.cls.fill) && same_bits(a.carry.fill2, a.cls.fill2);
    TracerIn carry = a.carry;   // the carried tracer with the class field's wrap rule
    carry.wrap_x = a.cls.wrap_x;
    return launch_tracer_thick_form<T>(carry, a.th, [&](auto... extra) {
        if constexpr ((std::is_same<decltype(extra), TauIn<T>>::value || ...))
            if (!one) return launch_gross_remap_t<T, true>(a, s, extra...);
        return launch_gross_remap_t<T, false>(a, s, extra...);
    });
}

int launch_gross_class_remap(const GrossRemapArgs &a, hipStream_t s)
{
    const StepInput &in = a.in;
    NF_REQUIRE(a.nedges >= 2 && a.nedges <= kMaxClassEdges && a.edges, NF_ERR_ARG, "gross class remap: bad class edges");
    NF_REQUIRE(a.window >= 1 && a.window <= kClassWindowMax, NF_ERR_ARG, "gross class remap: bad window");
    NF_TRY(check_raw_step("gross class remap", in, a.tr, a.scratch_len, (size_t)a.window));
    NF_REQUIRE(in.u && in.v && a.cls.tau && a.rows && in.thickness && in.arcE && in.arcN, NF_ERR_ARG,
               "gross class remap: null argument");
    NF_REQUIRE(!a.th.e3u || a.th.e3v, NF_ERR_ARG, "gross class remap: null argument");
    NF_REQUIRE(in.z0 < in.z1 && in.z1 <= a.nz, NF_ERR_ARG, "gross class remap: bad levels");
    if (a.tr.row_length() == 0) return NF_OK;
    if (in.dtype == NF_F64) return launch_gross_remap_form<double>(a, s);
    if (in.dtype == NF_F32) return launch_gross_remap_form<float>(a, s);
    NF_REQUIRE(false, NF_ERR_ARG, "gross class remap: dtype must be NF_F64 or NF_F32");
}

// ---- transports in true-depth bins: the terms of the profile, each spread over the depth of its layer at its own face ------
// depth_walk's terms and depths, binned by the window pieces: a term of level z goes by add_span's rule (this kernel keeps a
// written-out copy of it, see `put`) to the span (make_span) of
// [D_z, D_z+1] at its own face among the depth edges, looked up with class_row; no depth: row nedges + 1.  With per-cell
// thicknesses (ThickIn<T> among the trailing arguments) there are four spans per level, else one for the four faces; TauIn<T>
// among the trailing arguments: the carried form.  Per lane the adds run level-ascending, then in slot order, then row-ascending.
template <typename T, typename... TI>
__global__ __launch_bounds__(kBlock) void k_depth_segscan(const int *__restrict__ cell, const double *__restrict__ w4,
                                                          const int *__restrict__ seg, long n, const T *__restrict__ u,
                                                          const T *__restrict__ v, long ncell, unsigned nx, int z0, int z1,
                                                          const double *__restrict__ thickness,
                                                          const double *__restrict__ arcE, const double *__restrict__ arcN,
                                                          T fill, T fill2, int two, double scale, int sverdrup,
                                                          const double *__restrict__ edges, int nedges, int top, double surface,
                                                          int r0, int nwin, double *__restrict__ runsum, TI... extra)
{
    constexpr bool TR = (std::is_same<TI, TauIn<T>>::value || ...);
    constexpr bool CT = (std::is_same<TI, ThickIn<T>>::value || ...);
    const TauIn<T> ti = tau_in<T>(extra...);
    const ThickIn<T> ct = thick_arg<T>(extra...);
    const WindowLds w = window_lds(edges, nedges, nwin);
    const long k = (long)blockIdx.x * kBlock + threadIdx.x;
    const int lane = threadIdx.x & (kWave - 1);
    int key = -1;
    if (k < n) {   // 0 <= z0 < z1: the launcher's
        const Record r = load_record(cell, w4, k);
        key = load_key(seg, k);
        const auto nb = step_neighbours<TR>(r.c, nx, ncell, ti.wrap_x);
        const Arcs arc = load_arcs(arcE, arcN, r.c, nb);
        // the span of [a, b] among the edges: class_row; lo == hi: whole to the row of lo, jhi = -1 (k_surface_segscan's span
        // lambda states the same rule for its own lookup: a change to one is a change to the other)
        auto span = [&](double a, double b) {
            return make_span(true, a, b, nedges + 1, [&](double lo, double hi) {
                const int jlo = class_row(true, lo, w.e, nedges, top);
                if (lo == hi) return RowSpan{lo, hi, jlo, -1};
                return RowSpan{lo, hi, jlo, class_row(true, hi, w.e, nedges, top)};
            });
        };
        const int rend = r0 + nwin - 1;
        const double *e = w.e;
        double *acc = w.acc;
        // add_span<kBlock, 1>, written out: through the shared function every unrolled share loop of the forms without ThickIn
        // forms the address of e[j] with a scalar add of its own (13 instructions more a kernel); written out, the kernel is
        // the one it was before the pieces were shared, up to labels and branch polarity.  The rule is spread_span's,
        // statement for statement: a change there is a change here.
        auto put = [&](const RowSpan &p, double t) {
            if (p.jhi < 0) {
                const int q = p.jlo - r0;
                if (q >= 0 && q < nwin) acc[q * kBlock] += t;
                return;
            }
            const double width = p.hi - p.lo;
            const int ja = p.jlo > r0 ? p.jlo : r0, jb = p.jhi < rend ? p.jhi : rend;
            for (int j = ja; j <= jb; ++j) {
                const double left = j == p.jlo ? p.lo : e[j - 1], right = j == p.jhi ? p.hi : e[j];
                if (right != left) acc[(j - r0) * kBlock] += t * ((right - left) / width);
            }
        };
        depth_walk<T, TR, CT>(r, nb, arc, u, v, ncell, z0, z1, thickness, fill, fill2, two, scale, sverdrup, ti, ct, surface,
                              [&](const SlotTh &D, const SlotTh &Dn, const Slots &d, bool south) {
                                  if constexpr (CT) {
                                      if (south) put(span(D.s, Dn.s), r.wa.x * d.s);
                                      put(span(D.e, Dn.e), r.wa.y * d.e);
                                      put(span(D.n, Dn.n), r.wb.x * d.n);
                                      put(span(D.w, Dn.w), r.wb.y * d.w);
                                  } else {   // one depth for the four faces: one span
                                      const RowSpan p = span(D.e, Dn.e);
                                      if (south) put(p, r.wa.x * d.s);
                                      put(p, r.wa.y * d.e);
                                      put(p, r.wb.x * d.n);
                                      put(p, r.wb.y * d.w);
                                  }
                              });
    }
    window_scan_store<kBlock>(w.acc, key, lane, k, n, nwin, runsum);
}

// the trailing arguments choose the form as in launch_gross_t
template <typename T, typename... TI>
static int launch_depth_t(const DepthArgs &a, hipStream_t s, TI... extra)
{
    const WeightSet &ws = *a.tr.ws;
    const StepInput &in = a.in;
    const T fill = (T)in.fill, fill2 = (T)in.fill2;
    const int top = class_top(a.nedges);
    return for_each_window(a.tr, a.nedges + 2, a.window, a.scratch, a.rows, s, [&](int r0, int nwin, int) {
        return launch_lds(&k_depth_segscan<T, TI...>, record_grid(ws), dim3(kBlock), class_lds_bytes(a.nedges, nwin), s, ws.cell.get(),
                          ws.w4.get(), ws.seg.get(), ws.nrec, (const T *)in.u, (const T *)in.v, in.ncell, (unsigned)in.nx, in.z0, in.z1,
                          in.thickness, in.arcE, in.arcN, fill, fill2, (int)uv_two_markers(fill, fill2), in.scale, in.sverdrup, a.edges,
                          a.nedges, top, a.top, r0, nwin, a.scratch, extra...);
    });
}

template <typename T>
static int launch_depth_form(const DepthArgs &a, hipStream_t s)
{
    return launch_tracer_thick_form<T>(a.t, a.th, [&](auto... extra) { return launch_depth_t<T>(a, s, extra...); });
}

int launch_depth_transport(const DepthArgs &a, hipStream_t s)
{
    const StepInput &in = a.in;
    NF_REQUIRE(a.nedges >= 2 && a.nedges <= kMaxClassEdges && a.edges, NF_ERR_ARG, "depth transport: bad depth edges");
    NF_REQUIRE(a.window >= 1 && a.window <= kClassWindowMax, NF_ERR_ARG, "depth transport: bad window");
    NF_TRY(check_raw_step("depth transport", in, a.tr, a.scratch_len, (size_t)a.window));
    NF_REQUIRE(in.u && in.v && a.rows && in.thickness && in.arcE && in.arcN, NF_ERR_ARG, "depth transport: null argument");
    NF_REQUIRE(!a.th.e3u || a.th.e3v, NF_ERR_ARG, "depth transport: null argument");
    NF_REQUIRE(in.z0 < in.z1, NF_ERR_ARG, "depth transport: bad levels");
    if (a.tr.row_length() == 0) return NF_OK;
    if (in.dtype == NF_F64) return launch_depth_form<double>(a, s);
    if (in.dtype == NF_F32) return launch_depth_form<float>(a, s);
    NF_REQUIRE(false, NF_ERR_ARG, "depth transport: dtype must be NF_F64 or NF_F32");
}

// ---- transports between surfaces: k_depth_segscan with an edge set per face ---------------------------------------------
// The edges of a face are the face values (tr_face_raw, the surfaces' own markers and wrap rule) of the m surfaces, each raised
// to the one before it (a running max: non-decreasing); a face where any surface has no finite value has no edge set and sends
// every term to row m + 1.  A lane gathers the five values c, e, n, w, s of every surface once, before the level loop, and
// keeps the 4 m edges of its four faces in LDS behind the accumulators, ed[(face * m + k) * kSurfaceBlock + lane]: a wave reads
// 64 consecutive doubles, no bank conflict, and no dynamic index reaches a register array (it would go to scratch).  The row
// lookup is a linear count over the m <= 8 edges; with edges that are the same on every face it is class_row of
// k_depth_segscan, and depth_walk, make_span and add_span are the ones that kernel calls: the same bits.  Both thickness forms
// carry four spans per level, the edges differ from face to face.  Nothing is shared between waves and there is no barrier, so
// a workgroup is ONE wave (kSurfaceBlock lanes: the same records in the same waves as a kBlock launch would give them, hence
// the same scan): LDS is (nwin + 4 m) x 64 doubles a workgroup, 21 KiB at m = 8 with all ten rows in one window, and seven
// waves fit a CU where one 256-lane workgroup of 84 KiB would leave one wave per SIMD.  __launch_bounds__ stays kBlock although
// the launch has kSurfaceBlock lanes: the bound is part of how the kernel is compiled, and changing it is a tuning change.
constexpr int kSurfaceBlock = kWave;
template <typename T>
struct SurfIn {
    const T *p[kMaxSurfaces];   // step t' of every surface: (ncell) of the field dtype
    int m;
    T m1, m2;
    int wrap_x;
};

template <typename T, typename... TI>
__global__ __launch_bounds__(kBlock) void k_surface_segscan(const int *__restrict__ cell, const double *__restrict__ w4,
                                                            const int *__restrict__ seg, long n, const T *__restrict__ u,
                                                            const T *__restrict__ v, long ncell, unsigned nx, int z0, int z1,
                                                            const double *__restrict__ thickness,
                                                            const double *__restrict__ arcE, const double *__restrict__ arcN,
                                                            T fill, T fill2, int two, double scale, int sverdrup,
                                                            SurfIn<T> sf, double surface, int r0, int nwin,
                                                            double *__restrict__ runsum, TI... extra)
{
    constexpr bool TR = (std::is_same<TI, TauIn<T>>::value || ...);
    constexpr bool CT = (std::is_same<TI, ThickIn<T>>::value || ...);
    const TauIn<T> ti = tau_in<T>(extra...);
    const ThickIn<T> ct = thick_arg<T>(extra...);
    const int m = sf.m;
    extern __shared__ double class_lds[];
    double *acc = class_lds + threadIdx.x;                                 // acc[r * kSurfaceBlock]: this lane's row r
    double *ed = class_lds + (size_t)nwin * kSurfaceBlock + threadIdx.x;   // ed[(face * m + k) * kSurfaceBlock]: this lane's edges
    for (int r = 0; r < nwin; ++r) acc[r * kSurfaceBlock] = 0.0;           // every lane touches only its own part of the LDS
    const long k = (long)blockIdx.x * kSurfaceBlock + threadIdx.x;
    const int lane = threadIdx.x & (kWave - 1);
    int key = -1;
    if (k < n) {   // 0 <= z0 < z1: the launcher's
        const Record r = load_record(cell, w4, k);
        key = load_key(seg, k);
        const ClassNeighbours nbs = class_neighbours(r.c, nx, ncell, sf.wrap_x);
        const auto nb = step_neighbours<TR>(r.c, nx, ncell, ti.wrap_x);
        const Arcs arc = load_arcs(arcE, arcN, r.c, nb);
        // the edge sets of the four faces (slot order: south, east, north, west); ok: every surface has a finite value there
        bool ok_s = true, ok_e = true, ok_n = true, ok_w = true;
        {
            double ps = 0.0, pe = 0.0, pn = 0.0, pw = 0.0;
            auto edge = [&](int f, int q, bool h, double x, bool &ok, double &prev) {
                ok = ok && h && __builtin_isfinite(x);
                prev = (q == 0 || x > prev) ? x : prev;
                ed[(f * m + q) * kSurfaceBlock] = prev;
            };
            for (int q = 0; q < m; ++q) {
                const LevelTau<T> x = load_level_tau(sf.p[q], 0, r.c, nbs);
                double f;
                bool h = tr_face_raw<T>(x.s, x.c, true, sf.m1, sf.m2, &f);
                edge(0, q, h, f, ok_s, ps);
                h = tr_face_raw<T>(x.c, x.e, nbs.has_e, sf.m1, sf.m2, &f);
                edge(1, q, h, f, ok_e, pe);
                h = tr_face_raw<T>(x.c, x.n, nbs.has_n, sf.m1, sf.m2, &f);
                edge(2, q, h, f, ok_n, pn);
                h = tr_face_raw<T>(x.w, x.c, nbs.has_w, sf.m1, sf.m2, &f);
                edge(3, q, h, f, ok_w, pw);
            }
        }
        // the span of [a, b] among the m edges e of a face: row(x), the number of edges <= x, lo and hi in one pass; lo == hi:
        // whole to the row of lo, jhi = -1 (k_depth_segscan's span lambda states the same rule for class_row: a change to
        // one is a change to the other)
        auto span = [&](const double *e, bool ok, double a, double b) {
            return make_span(ok, a, b, m + 1, [&](double lo, double hi) {
                int jlo = 0, jhi = 0;
                for (int q = 0; q < m; ++q) {
                    const double x = e[q * kSurfaceBlock];
                    jlo += x <= lo ? 1 : 0;
                    jhi += x <= hi ? 1 : 0;
                }
                return RowSpan{lo, hi, jlo, lo == hi ? -1 : jhi};
            });
        };
        auto put = [&](const double *e, const RowSpan &p, double t) { add_span<kSurfaceBlock, kSurfaceBlock>(acc, e, p, t, r0, nwin); };
        const double *es = ed, *ee = ed + (size_t)m * kSurfaceBlock, *en = ed + (size_t)2 * m * kSurfaceBlock, *ew = ed + (size_t)3 * m * kSurfaceBlock;
        depth_walk<T, TR, CT>(r, nb, arc, u, v, ncell, z0, z1, thickness, fill, fill2, two, scale, sverdrup, ti, ct, surface,
                              [&](const SlotTh &D, const SlotTh &Dn, const Slots &d, bool south) {
                                  if (south) put(es, span(es, ok_s, D.s, Dn.s), r.wa.x * d.s);
                                  put(ee, span(ee, ok_e, D.e, Dn.e), r.wa.y * d.e);
                                  put(en, span(en, ok_n, D.n, Dn.n), r.wb.x * d.n);
                                  put(ew, span(ew, ok_w, D.w, Dn.w), r.wb.y * d.w);
                              });
    }
    window_scan_store<kSurfaceBlock>(acc, key, lane, k, n, nwin, runsum);
}

// m + 2 <= 10 rows fit one window of the default size, a smaller one repeats the pass
template <typename T, typename... TI>
static int launch_surface_t(const SurfaceArgs &a, hipStream_t s, TI... extra)
{
    const WeightSet &ws = *a.tr.ws;
    const StepInput &in = a.in;
    const T fill = (T)in.fill, fill2 = (T)in.fill2;
    SurfIn<T> sf{};
    for (int q = 0; q < a.sf.m; ++q) sf.p[q] = (const T *)a.sf.p[q];
    sf.m = a.sf.m;
    sf.m1 = (T)a.sf.fill;
    sf.m2 = (T)a.sf.fill2;
    sf.wrap_x = a.sf.wrap_x ? 1 : 0;
    const dim3 grid((unsigned)((ws.nrec + kSurfaceBlock - 1) / kSurfaceBlock));
    return for_each_window(a.tr, a.sf.m + 2, a.window, a.scratch, a.rows, s, [&](int r0, int nwin, int) {
        const size_t lds = sizeof(double) * ((size_t)nwin + 4 * (size_t)a.sf.m) * kSurfaceBlock;   // <= 21 KiB
        hipLaunchKernelGGL((k_surface_segscan<T, TI...>), grid, dim3(kSurfaceBlock), lds, s, ws.cell.get(), ws.w4.get(), ws.seg.get(),
                           ws.nrec, (const T *)in.u, (const T *)in.v, in.ncell, (unsigned)in.nx, in.z0, in.z1, in.thickness, in.arcE,
                           in.arcN, fill, fill2, (int)uv_two_markers(fill, fill2), in.scale, in.sverdrup, sf, a.top, r0, nwin,
                           a.scratch, extra...);
        return (int)NF_OK;
    });
}

template <typename T>
static int launch_surface_form(const SurfaceArgs &a, hipStream_t s)
{
    return launch_tracer_thick_form<T>(a.t, a.th, [&](auto... extra) { return launch_surface_t<T>(a, s, extra...); });
}

int launch_surface_transport(const SurfaceArgs &a, hipStream_t s)
{
    const StepInput &in = a.in;
    NF_REQUIRE(a.sf.m >= 1 && a.sf.m <= kMaxSurfaces, NF_ERR_ARG, "surface transport: bad number of surfaces");
    for (int q = 0; q < a.sf.m; ++q) NF_REQUIRE(a.sf.p[q], NF_ERR_ARG, "surface transport: null argument");
    NF_REQUIRE(a.window >= 1 && a.window <= kClassWindowMax, NF_ERR_ARG, "surface transport: bad window");
    NF_TRY(check_raw_step("surface transport", in, a.tr, a.scratch_len, (size_t)a.window));
    NF_REQUIRE(in.u && in.v && a.rows && in.thickness && in.arcE && in.arcN, NF_ERR_ARG, "surface transport: null argument");
    NF_REQUIRE(!a.th.e3u || a.th.e3v, NF_ERR_ARG, "surface transport: null argument");
    NF_REQUIRE(in.z0 < in.z1, NF_ERR_ARG, "surface transport: bad levels");
    NF_REQUIRE(__builtin_isfinite(a.top), NF_ERR_ARG, "surface transport: top must be a finite number");
    if (a.tr.row_length() == 0) return NF_OK;
    if (in.dtype == NF_F64) return launch_surface_form<double>(a, s);
    if (in.dtype == NF_F32) return launch_surface_form<float>(a, s);
    NF_REQUIRE(false, NF_ERR_ARG, "surface transport: dtype must be NF_F64 or NF_F32");
}

// ---- transport in joint classes of two tracers: gather once (k_joint_terms), bin many times (k_joint_bin) -------------
// The terms and the accumulation are k_class_segscan's: per owned level (z ascending) the four slot terms of level_slots_tf
// times their weights, each added in slot order (south, east, north, west) to the lane's accumulator of its row, then
// seg_scan_step per row with the one set of flags.  What differs is the row -- ra * (nb + 2) + rb from the faces' raw values
// of A and of B -- and that there may be thousands of rows: a window-by-window pass over the FIELDS would repeat the 14
// gathers per level for every window, so stage 1 issues them once and leaves the products and their rows in a table (layout:
// JointArgs), which stage 2 streams once per window with contiguous, full-sector loads.  -ffp-contract=off: a stored product
// added later has the bits of the product added at once, hence the 1-D class rows bit for bit where one axis has one class.
constexpr int kJointLevels = 4;        // levels whose 14 gathers (stage 1) or table loads (stage 2) are issued together
typedef unsigned short usvec4 __attribute__((ext_vector_type(4)));

// Stage 1.  LDS: ea (na doubles), eb (nbe doubles), then the block's window bitmap (nwords words), filled with LDS OR -- the
// outcome does not depend on the order -- and stored with one vector store per word.
// joint_mark_window: a term with row `row` was written, so the block's bit of that row's window is set.
__device__ inline void joint_mark_window(unsigned *bits, int row, int window)
{
    const int w = row / window;
    const unsigned m = 1u << (w & 31);
    if (!(bits[w >> 5] & m)) atomicOr(&bits[w >> 5], m);   // the read only spares the OR: a stale 0 sets the bit again
}
template <typename T, bool CARRY>
__global__ __launch_bounds__(kBlock) void k_joint_terms(const int *__restrict__ cell, const double *__restrict__ w4, long n,
                                                        const T *__restrict__ u, const T *__restrict__ v,
                                                        const T *__restrict__ sig, long ncell, unsigned nx, int z0, int z1,
                                                        const double *__restrict__ thickness,
                                                        const double *__restrict__ arcE, const double *__restrict__ arcN,
                                                        T fill, T fill2, int two, TauIn<T> ta, T sfill, T sfill2, double scale,
                                                        int sverdrup, const double *__restrict__ edges, int na, int nbe,
                                                        int topa, int topb, int window, int nwords,
                                                        dvec2 *__restrict__ terms, usvec4 *__restrict__ rows,
                                                        unsigned *__restrict__ flags)
{
    extern __shared__ double joint_lds[];
    const double *ea = joint_lds, *eb = joint_lds + na;
    unsigned *bits = reinterpret_cast<unsigned *>(joint_lds + na + nbe);
    for (int q = threadIdx.x; q < na + nbe; q += kBlock) joint_lds[q] = edges[q];
    for (int q = threadIdx.x; q < nwords; q += kBlock) bits[q] = 0u;
    __syncthreads();
    const long k = (long)blockIdx.x * kBlock + threadIdx.x;
    if (k < n) {
        const Record r = load_record(cell, w4, k);
        const ClassNeighbours nb = class_neighbours(r.c, nx, ncell, ta.wrap_x);
        const Arcs arc = load_arcs(arcE, arcN, r.c, nb);
        // the joint row of the face (a0, a1) of A and (b0, b1) of B; its window is marked in the bitmap
        auto joint_row = [&](T a0, T a1, T b0, T b1, bool has) {
            double f;
            bool h = tr_face_raw<T>(a0, a1, has, ta.m1, ta.m2, &f);
            const int ra = class_row(h, f, ea, na, topa);
            h = tr_face_raw<T>(b0, b1, has, sfill, sfill2, &f);
            const int row = ra * (nbe + 2) + class_row(h, f, eb, nbe, topb);
            joint_mark_window(bits, row, window);
            return (unsigned short)row;
        };
        for (int z = z0; z < z1; z += kJointLevels) {
            const int nlev = z1 - z < kJointLevels ? z1 - z : kJointLevels;
            LevelUV<T> x[kJointLevels];
            LevelTau<T> A[kJointLevels], B[kJointLevels];
#pragma unroll
            for (int l = 0; l < kJointLevels; ++l)
                if (l < nlev) {
                    const long o = (long)(z + l) * ncell;
                    x[l] = load_level_uv(u, v, o, r.c, nb);
                    A[l] = load_level_tau(ta.tau, o, r.c, nb);
                    B[l] = load_level_tau(sig, o, r.c, nb);
                }
#pragma unroll
            for (int l = 0; l < kJointLevels; ++l)
                if (l < nlev) {
                    FaceTf tf{};
                    if constexpr (CARRY) tf = level_tf(A[l], nb, ta);
                    const Slots d = level_slots_tf<T, CARRY>(slot_th(thickness[z + l]), x[l], arc, fill, fill2, two, scale, sverdrup,
                                                             nb.south, tf);
                    usvec4 jr;
                    jr.x = nb.south ? joint_row(A[l].s, A[l].c, B[l].s, B[l].c, true) : (unsigned short)kJointNoRow;
                    jr.y = joint_row(A[l].c, A[l].e, B[l].c, B[l].e, nb.has_e);
                    jr.z = joint_row(A[l].c, A[l].n, B[l].c, B[l].n, nb.has_n);
                    jr.w = joint_row(A[l].w, A[l].c, B[l].w, B[l].c, nb.has_w);
                    const long zi = z + l - z0;
                    __builtin_nontemporal_store(dvec2{r.wa.x * d.s, r.wa.y * d.e}, terms + (2 * zi) * n + k);
                    __builtin_nontemporal_store(dvec2{r.wb.x * d.n, r.wb.y * d.w}, terms + (2 * zi + 1) * n + k);
                    __builtin_nontemporal_store(jr, rows + zi * n + k);
                }
        }
    }
    __syncthreads();
    for (int q = threadIdx.x; q < nwords; q += kBlock) flags[(long)blockIdx.x * nwords + q] = bits[q];
}

// Stage 2 for the window [r0, r0 + nwin) of joint rows, window number `win`.  A lane reads its own table entries, z ascending:
// the rows of kJointLevels levels first, then the terms of the levels that have a row in the window, all in flight before
// the first add.  LDS: nwin x kBlock accumulators, no edges; the add keeps an unsigned window test of its own (the rows are
// unsigned short), the scan and the stores are window_scan_store.  skip: a block whose flag is clear adds nothing,
// so it does not read the table; its run sums are the +0.0 that the scan of untouched accumulators gives either way.
__global__ __launch_bounds__(kBlock) void k_joint_bin(const int *__restrict__ seg, long n, int nlev,
                                                      const dvec2 *__restrict__ terms, const usvec4 *__restrict__ rows,
                                                      const unsigned *__restrict__ flags, int nwords, int win, int skip, int r0,
                                                      int nwin, double *__restrict__ runsum)
{
    extern __shared__ double joint_acc[];
    double *acc = joint_acc + threadIdx.x;   // acc[q * kBlock]: this lane's row r0 + q; no lane touches another's
    for (int q = 0; q < nwin; ++q) acc[q * kBlock] = 0.0;
    const long k = (long)blockIdx.x * kBlock + threadIdx.x;
    const int lane = threadIdx.x & (kWave - 1);
    const bool live = !skip || ((flags[(long)blockIdx.x * nwords + (win >> 5)] >> (win & 31)) & 1u);
    int key = -1;
    if (k < n) {
        key = load_key(seg, k);
        if (live) {
            auto in_window = [&](unsigned short row) { return (unsigned)row - (unsigned)r0 < (unsigned)nwin; };
            auto add = [&](unsigned short row, double x) {
                if (in_window(row)) acc[((unsigned)row - (unsigned)r0) * kBlock] += x;
            };
            for (int z = 0; z < nlev; z += kJointLevels) {
                usvec4 jr[kJointLevels];
                dvec2 se[kJointLevels], nw[kJointLevels];
                bool hit[kJointLevels];
#pragma unroll
                for (int l = 0; l < kJointLevels; ++l)
                    if (z + l < nlev) jr[l] = __builtin_nontemporal_load(rows + (long)(z + l) * n + k);
#pragma unroll
                for (int l = 0; l < kJointLevels; ++l) {
                    hit[l] = z + l < nlev && (in_window(jr[l].x) || in_window(jr[l].y) || in_window(jr[l].z) || in_window(jr[l].w));
                    if (hit[l]) {
                        se[l] = __builtin_nontemporal_load(terms + (2l * (z + l)) * n + k);
                        nw[l] = __builtin_nontemporal_load(terms + (2l * (z + l) + 1) * n + k);
                    }
                }
#pragma unroll
                for (int l = 0; l < kJointLevels; ++l)
                    if (hit[l]) {
                        add(jr[l].x, se[l].x);
                        add(jr[l].y, se[l].y);
                        add(jr[l].z, nw[l].x);
                        add(jr[l].w, nw[l].y);
                    }
            }
        }
    }
    window_scan_store<kBlock>(acc, key, lane, k, n, nwin, runsum);
}

// stage 2 over all `nrows` rows of a term table of `nlev` levels, `window` rows per pass, each pass finalized into its rows of
// `out` (nrows, row_length): shared by the joint classes and the gross class transport
static int launch_joint_bins(const Transects &tr, int nrows, int nlev, int window, int skip, const dvec2 *terms,
                             const usvec4 *rows, const unsigned *flags, int nwords, double *scratch, double *out, hipStream_t s)
{
    const WeightSet &ws = *tr.ws;
    return for_each_window(tr, nrows, window, scratch, out, s, [&](int r0, int nwin, int win) {
        hipLaunchKernelGGL(k_joint_bin, record_grid(ws), dim3(kBlock), sizeof(double) * (size_t)nwin * kBlock, s, ws.seg.get(), ws.nrec,
                           nlev, terms, rows, flags, nwords, win, skip ? 1 : 0, r0, nwin, scratch);
        return (int)NF_OK;
    });
}

template <typename T, bool CARRY>
static int launch_joint_t(const JointArgs &a, hipStream_t s)
{
    const WeightSet &ws = *a.tr.ws;
    const StepInput &in = a.in;
    const int nrows = (a.na + 2) * (a.nb + 2), nlev = in.z1 - in.z0;
    const int nwords = joint_flag_words(nrows, a.window);
    const T fill = (T)in.fill, fill2 = (T)in.fill2;
    const int topa = class_top(a.na), topb = class_top(a.nb);
    dvec2 *terms = reinterpret_cast<dvec2 *>(a.table);
    usvec4 *rows = reinterpret_cast<usvec4 *>(a.table + sizeof(dvec2) * 2 * (size_t)ws.nrec * nlev);
    if (ws.nrec > 0) {
        const size_t lds = sizeof(double) * (size_t)(a.na + a.nb) + sizeof(unsigned) * (size_t)nwords;
        hipLaunchKernelGGL((k_joint_terms<T, CARRY>), record_grid(ws), dim3(kBlock), lds, s, ws.cell.get(), ws.w4.get(), ws.nrec,
                           (const T *)in.u, (const T *)in.v, (const T *)a.tb.tau, in.ncell, (unsigned)in.nx, in.z0, in.z1,
                           in.thickness, in.arcE, in.arcN, fill, fill2, (int)uv_two_markers(fill, fill2), tau_of<T>(a.ta),
                           (T)a.tb.fill, (T)a.tb.fill2, in.scale, in.sverdrup, a.edges, a.na, a.nb, topa, topb, a.window, nwords,
                           terms, rows, a.flags);
        NF_HIP(hipGetLastError());
    }
    return launch_joint_bins(a.tr, nrows, nlev, a.window, a.skip, terms, rows, a.flags, nwords, a.scratch, a.rows, s);
}

int launch_joint_class_transport(const JointArgs &a, hipStream_t s)
{
    const StepInput &in = a.in;
    const auto edges_ok = [](int n) { return n >= 2 && n <= kMaxClassEdges; };
    NF_REQUIRE(edges_ok(a.na) && edges_ok(a.nb) && a.edges && (a.na + 2) * (a.nb + 2) <= kMaxJointRows, NF_ERR_ARG,
               "joint class transport: bad class edges");
    NF_REQUIRE(a.window >= 1 && a.window <= kClassWindowMax, NF_ERR_ARG, "joint class transport: bad window");
    NF_TRY(check_raw_step("joint class transport", in, a.tr, a.scratch_len, (size_t)a.window));
    NF_REQUIRE(in.u && in.v && a.ta.tau && a.tb.tau && a.rows && in.thickness && in.arcE && in.arcN, NF_ERR_ARG,
               "joint class transport: null argument");
    if (a.tr.row_length() == 0) return NF_OK;
    const size_t nrec = (size_t)a.tr.ws->nrec, blocks = (nrec + kBlock - 1) / kBlock;
    NF_REQUIRE(nrec == 0 || (a.table && a.table_len >= kJointEntryBytes * nrec * (size_t)(in.z1 - in.z0)), NF_ERR_ARG,
               "joint class transport: the term table is too small");
    NF_REQUIRE(nrec == 0 || (a.flags && a.flags_len >= blocks * (size_t)joint_flag_words((a.na + 2) * (a.nb + 2), a.window)),
               NF_ERR_ARG, "joint class transport: the flag array is too small");
    if (in.dtype == NF_F64) return a.carry ? launch_joint_t<double, true>(a, s) : launch_joint_t<double, false>(a, s);
    if (in.dtype == NF_F32) return a.carry ? launch_joint_t<float, true>(a, s) : launch_joint_t<float, false>(a, s);
    NF_REQUIRE(false, NF_ERR_ARG, "joint class transport: dtype must be NF_F64 or NF_F32");
}

// ---- gross (inflow / outflow) transports in tracer classes: k_gross_class_terms, then k_joint_bin ---------------------
// Where the gross profile and the class transport cross: per (record, owned level, slot) the water term q = w * d of
// k_gross_segscan, the carried term c (= q in the volume form, w * d^tau in the carried form) and the class row r of the slot's
// face, k_class_segscan's; c goes to row r of P where q > 0 and to row r of N where q < 0 -- row part * (nedges + 2) + r of the
// term table, part 0 = P, 1 = N -- and a slot with q == 0 (row 0's south slot among them) to kJointNoRow.  The table and the
// window bitmap are JointArgs', so stage 2 is k_joint_bin as it stands: a lane's accumulator of a row starts at +0.0 and takes
// its terms z ascending, slots in order.  The widest form gathers 4 + 4 + 5 + 5 values per level, once.
// FORM: 0 = volume, 1 = carried tracer that is the class field (one set of 5 gathers), 2 = carried tracer and a class field of
// its own.  TI: empty or ThickIn<T>, the per-cell thicknesses.  LZ: the levels whose gathers are issued together.
// LDS: the edges (nedges doubles), then the block's window bitmap (nwords words).
template <typename T, int FORM, int LZ, typename... TI>
__global__ __launch_bounds__(kBlock) void k_gross_class_terms(const int *__restrict__ cell, const double *__restrict__ w4, long n,
                                                              const T *__restrict__ u, const T *__restrict__ v, long ncell,
                                                              unsigned nx, int z0, int z1, const double *__restrict__ thickness,
                                                              const double *__restrict__ arcE, const double *__restrict__ arcN,
                                                              T fill, T fill2, int two, TauIn<T> cls, TauIn<T> carry, double scale,
                                                              int sverdrup, const double *__restrict__ edges, int nedges, int top,
                                                              int window, int nwords, dvec2 *__restrict__ terms,
                                                              usvec4 *__restrict__ rows, unsigned *__restrict__ flags, TI... extra)
{
    constexpr bool CT = sizeof...(TI) > 0;
    const ThickIn<T> ct = thick_arg<T>(extra...);
    extern __shared__ double gross_class_lds[];
    const double *e = gross_class_lds;
    unsigned *bits = reinterpret_cast<unsigned *>(gross_class_lds + nedges);
    for (int q = threadIdx.x; q < nedges; q += kBlock) gross_class_lds[q] = edges[q];
    for (int q = threadIdx.x; q < nwords; q += kBlock) bits[q] = 0u;
    __syncthreads();
    const long k = (long)blockIdx.x * kBlock + threadIdx.x;
    if (k < n) {
        const Record r = load_record(cell, w4, k);
        const ClassNeighbours nb = class_neighbours(r.c, nx, ncell, cls.wrap_x);
        const Arcs arc = load_arcs(arcE, arcN, r.c, nb);
        // the row of a slot with water term q whose face has the class values (a0, a1); its window is marked in the bitmap
        auto gross_row = [&](double q, T a0, T a1, bool has) {
            if (!(q > 0.0) && !(q < 0.0)) return (unsigned short)kJointNoRow;
            double f;
            const bool h = tr_face_raw<T>(a0, a1, has, cls.m1, cls.m2, &f);
            const int row = (q < 0.0 ? nedges + 2 : 0) + class_row(h, f, e, nedges, top);
            joint_mark_window(bits, row, window);
            return (unsigned short)row;
        };
        for (int z = z0; z < z1; z += LZ) {
            const int nlev = z1 - z < LZ ? z1 - z : LZ;
            LevelUV<T> x[LZ];
            LevelUV<T> e3[CT ? LZ : 1];
            LevelTau<T> S[LZ];                    // the class field
            LevelTau<T> A[FORM == 2 ? LZ : 1];    // the carried tracer, when it is another array
#pragma unroll
            for (int l = 0; l < LZ; ++l)
                if (l < nlev) {
                    const long o = (long)(z + l) * ncell;
                    x[l] = load_level_uv(u, v, o, r.c, nb);
                    if constexpr (CT) e3[l] = load_level_e3(ct, o, r.c, nb);
                    S[l] = load_level_tau(cls.tau, o, r.c, nb);
                    if constexpr (FORM == 2) A[l] = load_level_tau(carry.tau, o, r.c, nb);
                }
#pragma unroll
            for (int l = 0; l < LZ; ++l)
                if (l < nlev) {
                    SlotTh th;
                    if constexpr (CT)
                        th = level_th(e3[l], ct);
                    else
                        th = slot_th(thickness[z + l]);
                    const Slots q = weighted_slots(
                        r, level_slots_tf<T, false>(th, x[l], arc, fill, fill2, two, scale, sverdrup, nb.south, FaceTf{}));
                    Slots c = q;
                    if constexpr (FORM != 0)
                        c = weighted_slots(r, level_slots_tf<T, true>(th, x[l], arc, fill, fill2, two, scale, sverdrup, nb.south,
                                                                      level_tf(FORM == 2 ? A[l] : S[l], nb, carry)));
                    usvec4 jr;
                    jr.x = nb.south ? gross_row(q.s, S[l].s, S[l].c, true) : (unsigned short)kJointNoRow;
                    jr.y = gross_row(q.e, S[l].c, S[l].e, nb.has_e);
                    jr.z = gross_row(q.n, S[l].c, S[l].n, nb.has_n);
                    jr.w = gross_row(q.w, S[l].w, S[l].c, nb.has_w);
                    const long zi = z + l - z0;
                    __builtin_nontemporal_store(dvec2{c.s, c.e}, terms + (2 * zi) * n + k);
                    __builtin_nontemporal_store(dvec2{c.n, c.w}, terms + (2 * zi + 1) * n + k);
                    __builtin_nontemporal_store(jr, rows + zi * n + k);
                }
        }
    }
    __syncthreads();
    for (int q = threadIdx.x; q < nwords; q += kBlock) flags[(long)blockIdx.x * nwords + q] = bits[q];
}

template <typename T, int FORM, typename... TI>
static int launch_gross_class_t(const GrossClassArgs &a, hipStream_t s, TI... extra)
{
    const WeightSet &ws = *a.tr.ws;
    const StepInput &in = a.in;
    const int nrows = 2 * (a.nedges + 2), nlev = in.z1 - in.z0;
    const int nwords = joint_flag_words(nrows, a.window);
    const T fill = (T)in.fill, fill2 = (T)in.fill2;
    const int top = class_top(a.nedges);
    dvec2 *terms = reinterpret_cast<dvec2 *>(a.table);
    usvec4 *rows = reinterpret_cast<usvec4 *>(a.table + sizeof(dvec2) * 2 * (size_t)ws.nrec * nlev);
    if (ws.nrec > 0) {
        const size_t lds = sizeof(double) * (size_t)a.nedges + sizeof(unsigned) * (size_t)nwords;
        TauIn<T> carry = tau_of<T>(a.carry);
        carry.wrap_x = a.cls.wrap_x ? 1 : 0;
        hipLaunchKernelGGL((k_gross_class_terms<T, FORM, kGrossClassLevels, TI...>), record_grid(ws), dim3(kBlock), lds, s,
                           ws.cell.get(), ws.w4.get(), ws.nrec, (const T *)in.u, (const T *)in.v, in.ncell, (unsigned)in.nx, in.z0,
                           in.z1, in.thickness, in.arcE, in.arcN, fill, fill2, (int)uv_two_markers(fill, fill2), tau_of<T>(a.cls),
                           carry, in.scale, in.sverdrup, a.edges, a.nedges, top, a.window, nwords, terms, rows, a.flags, extra...);
        NF_HIP(hipGetLastError());
    }
    return launch_joint_bins(a.tr, nrows, nlev, a.window, a.skip, terms, rows, a.flags, nwords, a.scratch, a.rows, s);
}

// the three forms of one dtype, each with the scalar or the per-cell thicknesses
template <typename T, int FORM>
static int launch_gross_class_th(const GrossClassArgs &a, hipStream_t s)
{
    if (a.th.e3u) return launch_gross_class_t<T, FORM>(a, s, thick_in<T>(a.th));
    return launch_gross_class_t<T, FORM>(a, s);
}
template <typename T>
static int launch_gross_class_form(const GrossClassArgs &a, hipStream_t s)
{
    if (!a.carry.tau) return launch_gross_class_th<T, 0>(a, s);
    const bool one = a.carry.tau == a.cls.tau && same_bits(a.carry.fill, a.cls.fill) && same_bits(a.carry.fill2, a.cls.fill2);
    return one ? launch_gross_class_th<T, 1>(a, s) : launch_gross_class_th<T, 2>(a, s);
}

int launch_gross_class_transport(const GrossClassArgs &a, hipStream_t s)
{
    const StepInput &in = a.in;
    NF_REQUIRE(a.nedges >= 2 && a.nedges <= kMaxClassEdges && a.edges, NF_ERR_ARG, "gross class transport: bad class edges");
    static_assert(2 * (kMaxClassEdges + 2) <= kMaxJointRows && 2 * (kMaxClassEdges + 2) < (int)kJointNoRow, "rows fit the table");
    NF_REQUIRE(a.window >= 1 && a.window <= kClassWindowMax, NF_ERR_ARG, "gross class transport: bad window");
    NF_TRY(check_raw_step("gross class transport", in, a.tr, a.scratch_len, (size_t)a.window));
    NF_REQUIRE(in.u && in.v && a.cls.tau && a.rows && in.thickness && in.arcE && in.arcN, NF_ERR_ARG,
               "gross class transport: null argument");
    NF_REQUIRE(!a.th.e3u || a.th.e3v, NF_ERR_ARG, "gross class transport: null argument");
    if (a.tr.row_length() == 0) return NF_OK;
    const size_t nrec = (size_t)a.tr.ws->nrec, blocks = (nrec + kBlock - 1) / kBlock;
    NF_REQUIRE(nrec == 0 || (a.table && a.table_len >= kJointEntryBytes * nrec * (size_t)(in.z1 - in.z0)), NF_ERR_ARG,
               "gross class transport: the term table is too small");
    NF_REQUIRE(nrec == 0 || (a.flags && a.flags_len >= blocks * (size_t)joint_flag_words(2 * (a.nedges + 2), a.window)),
               NF_ERR_ARG, "gross class transport: the flag array is too small");
    if (in.dtype == NF_F64) return launch_gross_class_form<double>(a, s);
    if (in.dtype == NF_F32) return launch_gross_class_form<float>(a, s);
    NF_REQUIRE(false, NF_ERR_ARG, "gross class transport: dtype must be NF_F64 or NF_F32");
}

// ---- section area in tracer classes: k_class_area_terms, then k_joint_bin ---------------------------------------------
// Where the area profile and the class transport cross: per (record, owned level, slot) the alpha and beta of area_terms
// (area_slot) and the class row r of the slot's face, k_class_segscan's, from the class field -- the carried tracer itself
// (TWO = false: one set of 5 gathers, the face value that makes the face count is its class value) or a class field of its own
// (TWO = true: a counted face without a class value goes to row nedges + 1).  alpha goes to row r of part 0 (A), beta to row
// (nedges + 2) + r of part 1 (B); a slot that does not count (row 0's south slot among them) to kJointNoRow in both.  A table
// entry of JointArgs' layout holds ONE term per slot, so a (record, level) takes two: entry zi of the nlev owned levels holds
// the alphas, entry nlev + zi the betas, and stage 2 is k_joint_bin as it stands over 2 * nlev "levels" -- a lane's accumulator
// of a row starts at +0.0 and takes its terms z ascending, slots in order, because a row of A meets only the first nlev entries
// and a row of B only the last.  The velocities are gathered for their presence alone; the widest form gathers 4 + 4 + 5 + 5
// values per level, once.  TI: empty or ThickIn<T>, the per-cell thicknesses.  LZ: the levels whose gathers are issued together.
// LDS: the edges (nedges doubles), then the block's window bitmap (nwords words).
template <typename T, bool TWO, int LZ, typename... TI>
__global__ __launch_bounds__(kBlock) void k_class_area_terms(const int *__restrict__ cell, const double *__restrict__ w4, long n,
                                                             const T *__restrict__ u, const T *__restrict__ v, long ncell,
                                                             unsigned nx, int z0, int z1, const double *__restrict__ thickness,
                                                             const double *__restrict__ arcE, const double *__restrict__ arcN,
                                                             T fill, T fill2, int two, TauIn<T> cls, TauIn<T> carry,
                                                             const double *__restrict__ edges, int nedges, int top, int window,
                                                             int nwords, dvec2 *__restrict__ terms, usvec4 *__restrict__ rows,
                                                             unsigned *__restrict__ flags, TI... extra)
{
    constexpr bool CT = sizeof...(TI) > 0;
    const ThickIn<T> ct = thick_arg<T>(extra...);
    extern __shared__ double class_area_lds[];
    const double *e = class_area_lds;
    unsigned *bits = reinterpret_cast<unsigned *>(class_area_lds + nedges);
    for (int q = threadIdx.x; q < nedges; q += kBlock) class_area_lds[q] = edges[q];
    for (int q = threadIdx.x; q < nwords; q += kBlock) bits[q] = 0u;
    __syncthreads();
    const long k = (long)blockIdx.x * kBlock + threadIdx.x;
    if (k < n) {
        const Record r = load_record(cell, w4, k);
        const ClassNeighbours nb = class_neighbours(r.c, nx, ncell, carry.wrap_x);
        const Arcs arc = load_arcs(arcE, arcN, r.c, nb);
        const long ztot = z1 - z0;
        // one slot: its alpha and beta and its row in A, kJointNoRow where the face does not count (its row in B: part_b);
        // both windows are marked in the bitmap.  (s0, s1): the face's values of the class field, (t0, t1) of the carried tracer
        auto slot = [&](bool on, double w, double th, T vel, double a, T s0, T s1, T t0, T t1, bool has_b, double *al,
                        double *be) {
            double f;
            if (!area_slot<T>(on, w, th, vel, a, t0, t1, has_b, fill, fill2, two, carry, al, be, &f))
                return (unsigned short)kJointNoRow;
            bool h = true;
            if constexpr (TWO) h = tr_face_raw<T>(s0, s1, has_b, cls.m1, cls.m2, &f);
            const int row = class_row(h, f, e, nedges, top);
            joint_mark_window(bits, row, window);
            joint_mark_window(bits, nedges + 2 + row, window);
            return (unsigned short)row;
        };
        auto part_b = [&](unsigned short row) {
            return row == (unsigned short)kJointNoRow ? row : (unsigned short)(nedges + 2 + row);
        };
        for (int z = z0; z < z1; z += LZ) {
            const int nlev = z1 - z < LZ ? z1 - z : LZ;
            LevelUV<T> x[LZ];
            LevelUV<T> e3[CT ? LZ : 1];
            LevelTau<T> A[LZ];                // the carried tracer
            LevelTau<T> S[TWO ? LZ : 1];      // the class field, when it is another array
#pragma unroll
            for (int l = 0; l < LZ; ++l)
                if (l < nlev) {
                    const long o = (long)(z + l) * ncell;
                    x[l] = load_level_uv(u, v, o, r.c, nb);
                    if constexpr (CT) e3[l] = load_level_e3(ct, o, r.c, nb);
                    A[l] = load_level_tau(carry.tau, o, r.c, nb);
                    if constexpr (TWO) S[l] = load_level_tau(cls.tau, o, r.c, nb);
                }
#pragma unroll
            for (int l = 0; l < LZ; ++l)
                if (l < nlev) {
                    SlotTh th;
                    if constexpr (CT)
                        th = level_th(e3[l], ct);
                    else
                        th = slot_th(thickness[z + l]);
                    const LevelTau<T> &C = TWO ? S[l] : A[l];
                    Slots al, be;
                    usvec4 ja, jb;
                    ja.x = slot(nb.south, r.wa.x, th.s, x[l].vs, arc.Ns, C.s, C.c, A[l].s, A[l].c, true, &al.s, &be.s);
                    ja.y = slot(true, r.wa.y, th.e, x[l].uc, arc.Ec, C.c, C.e, A[l].c, A[l].e, nb.has_e, &al.e, &be.e);
                    ja.z = slot(true, r.wb.x, th.n, x[l].vc, arc.Nc, C.c, C.n, A[l].c, A[l].n, nb.has_n, &al.n, &be.n);
                    ja.w = slot(true, r.wb.y, th.w, x[l].uw, arc.Ew, C.w, C.c, A[l].w, A[l].c, nb.has_w, &al.w, &be.w);
                    jb.x = part_b(ja.x), jb.y = part_b(ja.y), jb.z = part_b(ja.z), jb.w = part_b(ja.w);
                    const long za = z + l - z0, zb = ztot + za;
                    __builtin_nontemporal_store(dvec2{al.s, al.e}, terms + (2 * za) * n + k);
                    __builtin_nontemporal_store(dvec2{al.n, al.w}, terms + (2 * za + 1) * n + k);
                    __builtin_nontemporal_store(ja, rows + za * n + k);
                    __builtin_nontemporal_store(dvec2{be.s, be.e}, terms + (2 * zb) * n + k);
                    __builtin_nontemporal_store(dvec2{be.n, be.w}, terms + (2 * zb + 1) * n + k);
                    __builtin_nontemporal_store(jb, rows + zb * n + k);
                }
        }
    }
    __syncthreads();
    for (int q = threadIdx.x; q < nwords; q += kBlock) flags[(long)blockIdx.x * nwords + q] = bits[q];
}

template <typename T, bool TWO, typename... TI>
static int launch_class_area_t(const ClassAreaArgs &a, hipStream_t s, TI... extra)
{
    const WeightSet &ws = *a.tr.ws;
    const StepInput &in = a.in;
    const int nrows = 2 * (a.nedges + 2), nent = 2 * (in.z1 - in.z0);   // two table entries per owned level
    const int nwords = joint_flag_words(nrows, a.window);
    const T fill = (T)in.fill, fill2 = (T)in.fill2;
    const int top = class_top(a.nedges);
    dvec2 *terms = reinterpret_cast<dvec2 *>(a.table);
    usvec4 *rows = reinterpret_cast<usvec4 *>(a.table + sizeof(dvec2) * 2 * (size_t)ws.nrec * nent);
    if (ws.nrec > 0) {
        const size_t lds = sizeof(double) * (size_t)a.nedges + sizeof(unsigned) * (size_t)nwords;
        TauIn<T> carry = tau_of<T>(a.carry);
        carry.wrap_x = a.cls.wrap_x ? 1 : 0;
        hipLaunchKernelGGL((k_class_area_terms<T, TWO, kClassAreaLevels, TI...>), record_grid(ws), dim3(kBlock), lds, s,
                           ws.cell.get(), ws.w4.get(), ws.nrec, (const T *)in.u, (const T *)in.v, in.ncell, (unsigned)in.nx, in.z0,
                           in.z1, in.thickness, in.arcE, in.arcN, fill, fill2, (int)uv_two_markers(fill, fill2), tau_of<T>(a.cls),
                           carry, a.edges, a.nedges, top, a.window, nwords, terms, rows, a.flags, extra...);
        NF_HIP(hipGetLastError());
    }
    return launch_joint_bins(a.tr, nrows, nent, a.window, a.skip, terms, rows, a.flags, nwords, a.scratch, a.rows, s);
}

// the two forms of one dtype, each with the scalar or the per-cell thicknesses
template <typename T, bool TWO>
static int launch_class_area_th(const ClassAreaArgs &a, hipStream_t s)
{
    if (a.th.e3u) return launch_class_area_t<T, TWO>(a, s, thick_in<T>(a.th));
    return launch_class_area_t<T, TWO>(a, s);
}
template <typename T>
static int launch_class_area_form(const ClassAreaArgs &a, hipStream_t s)
{
    const bool one = a.carry.tau == a.cls.tau && same_bits(a.carry.fill, a.cls.fill) && same_bits(a.carry.fill2, a.cls.fill2);
    return one ? launch_class_area_th<T, false>(a, s) : launch_class_area_th<T, true>(a, s);
}

int launch_class_area(const ClassAreaArgs &a, hipStream_t s)
{
    const StepInput &in = a.in;
    NF_REQUIRE(a.nedges >= 2 && a.nedges <= kMaxClassEdges && a.edges, NF_ERR_ARG, "class area: bad class edges");
    NF_REQUIRE(a.window >= 1 && a.window <= kClassWindowMax, NF_ERR_ARG, "class area: bad window");
    NF_TRY(check_raw_step("class area", in, a.tr, a.scratch_len, (size_t)a.window));
    NF_REQUIRE(in.u && in.v && a.cls.tau && a.carry.tau && a.rows && in.thickness && in.arcE && in.arcN, NF_ERR_ARG,
               "class area: null argument");
    NF_REQUIRE(!a.th.e3u || a.th.e3v, NF_ERR_ARG, "class area: null argument");
    if (a.tr.row_length() == 0) return NF_OK;
    const size_t nrec = (size_t)a.tr.ws->nrec, blocks = (nrec + kBlock - 1) / kBlock;
    NF_REQUIRE(nrec == 0 || (a.table && a.table_len >= kClassAreaEntryBytes * nrec * (size_t)(in.z1 - in.z0)), NF_ERR_ARG,
               "class area: the term table is too small");
    NF_REQUIRE(nrec == 0 || (a.flags && a.flags_len >= blocks * (size_t)joint_flag_words(2 * (a.nedges + 2), a.window)),
               NF_ERR_ARG, "class area: the flag array is too small");
    if (in.dtype == NF_F64) return launch_class_area_form<double>(a, s);
    if (in.dtype == NF_F32) return launch_class_area_form<float>(a, s);
    NF_REQUIRE(false, NF_ERR_ARG, "class area: dtype must be NF_F64 or NF_F32");
}

}  // namespace nf
