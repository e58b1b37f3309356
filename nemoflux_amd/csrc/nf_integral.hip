// nf_integral.hip -- K3: gather of the weighted edge fluxes and their reduction onto target segments.
//
// Replaces  mint.PolylineIntegral.getIntegral(data, mint.CELL_BY_CELL_DATA) as driven by
//           nemoflux/field.py:102 and nemoflux/fluxplot.py:56, for ALL transects of a Field at once.
//
// Two forms of stage A.  For the engine's own resident planes the weights come folded onto the unique edges
// (k_gather_edges, below: one gather per entry); for caller-supplied (ncell,4) data -- mint's getIntegral -- the records
// are used as they are:
// Records (cell, 4 edge weights, global segment id) are sorted by segment (K2).  Stage A: one lane per
// record gathers the cell's 4 edge values (either the reference's (ncell,4) AoS: one 32-B read, or the engine's
// resident [4][ncell] planes), forms the weighted sum and runs a WAVEFRONT SEGMENTED SCAN keyed by the
// segment id (6 shuffle steps); the last lane of every run inside the wave stores the run's sum.  Stage B: one
// wavefront per target segment stitches the run sums of the waves the segment spans.  Stage C: one wavefront
// per transect adds its segments.  No atomics: the summation tree is fixed, so results are bitwise
// reproducible.
//
// Output row: [ per-segment sums (nseg) | per-transect sums (ntransect) ].
#include "nf_common.h"

namespace nf {

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
    const int lane = threadIdx.x & (kWave - 1);
    double val = 0.0;
    int key = -1;
    if (k < n) {
        // the record stream is read once per launch: non-temporal, so that it does not push the plane sectors its
        // neighbours gather -- nor the arc lengths the next flux kernel re-reads -- out of the caches (-0.7 % per pass)
        typedef double dvec2 __attribute__((ext_vector_type(2)));
        const long c = __builtin_nontemporal_load(cell + k);
        const dvec2 *pw = reinterpret_cast<const dvec2 *>(w4 + 4 * k);
        const dvec2 wa = __builtin_nontemporal_load(pw), wb = __builtin_nontemporal_load(pw + 1);
        double d0, d1, d2, d3;
        if (planes == 2) {
            // the engine's own planes: the south and west slots are copies of the neighbours' north and east values
            // (field.py:219-223), so only the two signed planes are touched: eU[c-1], eU[c] share a sector and
            // eV[c-nx] is the eV[c] of the record one row below -- about half the sectors of four separate planes
            const unsigned j = (unsigned)(c / nx), i = (unsigned)(c - (long)j * nx);
            const double *eU = data + ncell, *eV = data + 2 * ncell;
            d1 = eU[c];
            d2 = eV[c];
            d0 = j > 0 ? eV[c - nx] : 0.0;               // row 0's south slot is never written (field.py:219)
            d3 = eU[i > 0 ? c - 1 : c - 1 + nx];         // column 0: periodic copy of column nx-1 (field.py:223)
        } else if (planes) {
            d0 = data[c];
            d1 = data[ncell + c];
            d2 = data[2 * ncell + c];
            d3 = data[3 * ncell + c];
        } else {
            const double2 *pd = reinterpret_cast<const double2 *>(data + 4 * c);
            const double2 da = pd[0], db = pd[1];
            d0 = da.x; d1 = da.y; d2 = db.x; d3 = db.y;
        }
        val = ((wa.x * d0 + wa.y * d1) + wb.x * d2) + wb.y * d3;
        key = __builtin_nontemporal_load(seg + k);
    }
#pragma unroll
    for (int o = 1; o < kWave; o <<= 1) {
        const double pv = __shfl_up(val, o, kWave);
        const int pk = __shfl_up(key, o, kWave);
        if (lane >= o && pk == key) val += pv;
    }
    const int nk = __shfl_down(key, 1, kWave);
    if (k < n && (lane == kWave - 1 || k == n - 1 || nk != key)) runsum[k] = val;
}

// Stage A for TWO time steps of the engine's own planes at once (the per-step pass takes its whole steps in pairs): the
// 40-byte record is read once, the same four elements are gathered from both steps' signed planes, and the two weighted
// sums go through the segmented scan side by side.  Each step's sum is formed and scanned exactly as in k_gather_segscan
// (planes = 2): bit-identical rows.  uvA / uvB: a step's eU plane, its eV plane right behind it; runsum: 2 * n doubles.
__global__ __launch_bounds__(kBlock) void k_gather_segscan_pair(const int *__restrict__ cell, const double *__restrict__ w4,
                                                                const int *__restrict__ seg, long n,
                                                                const double *__restrict__ uvA,
                                                                const double *__restrict__ uvB, long ncell, unsigned nx,
                                                                double *__restrict__ runsum)
{
    const long k = (long)blockIdx.x * kBlock + threadIdx.x;
    const int lane = threadIdx.x & (kWave - 1);
    double va = 0.0, vb = 0.0;
    int key = -1;
    if (k < n) {
        typedef double dvec2 __attribute__((ext_vector_type(2)));
        const long c = __builtin_nontemporal_load(cell + k);
        const dvec2 *pw = reinterpret_cast<const dvec2 *>(w4 + 4 * k);
        const dvec2 wa = __builtin_nontemporal_load(pw), wb = __builtin_nontemporal_load(pw + 1);
        const unsigned j = (unsigned)(c / nx), i = (unsigned)(c - (long)j * nx);
        const long cw = i > 0 ? c - 1 : c - 1 + nx;
        {
            const double *eU = uvA, *eV = uvA + ncell;
            const double d1 = eU[c], d2 = eV[c], d0 = j > 0 ? eV[c - nx] : 0.0, d3 = eU[cw];
            va = ((wa.x * d0 + wa.y * d1) + wb.x * d2) + wb.y * d3;
        }
        {
            const double *eU = uvB, *eV = uvB + ncell;
            const double d1 = eU[c], d2 = eV[c], d0 = j > 0 ? eV[c - nx] : 0.0, d3 = eU[cw];
            vb = ((wa.x * d0 + wa.y * d1) + wb.x * d2) + wb.y * d3;
        }
        key = __builtin_nontemporal_load(seg + k);
    }
#pragma unroll
    for (int o = 1; o < kWave; o <<= 1) {
        const double pa = __shfl_up(va, o, kWave), pb = __shfl_up(vb, o, kWave);
        const int pk = __shfl_up(key, o, kWave);
        if (lane >= o && pk == key) {
            va += pa;
            vb += pb;
        }
    }
    const int nk = __shfl_down(key, 1, kWave);
    if (k < n && (lane == kWave - 1 || k == n - 1 || nk != key)) {
        runsum[k] = va;
        runsum[n + k] = vb;
    }
}

// Unique-edge form of stage A for the engine's own planes (WeightSet::EdgeEntry): one lane per (segment, plane element)
// entry -- ONE 16-byte record load and ONE 8-byte gather from [eU | eV] -- then the same wavefront segmented scan.
// Entries are sorted by (segment, element), so the gathers of neighbouring lanes walk the planes in ascending order.
__global__ __launch_bounds__(kBlock) void k_gather_edges(const WeightSet::EdgeEntry *__restrict__ ent, long n,
                                                         const double *__restrict__ data, long ncell,
                                                         double *__restrict__ runsum, long data_stride)
{
    data += (long)blockIdx.y * data_stride + ncell;   // planes 1 (eU) and 2 (eV) are contiguous: one array of 2*ncell
    runsum += (long)blockIdx.y * n;
    const long k = (long)blockIdx.x * kBlock + threadIdx.x;
    const int lane = threadIdx.x & (kWave - 1);
    double val = 0.0;
    int key = -1;
    if (k < n) {
        typedef int ivec4 __attribute__((ext_vector_type(4)));
        const ivec4 r = __builtin_nontemporal_load(reinterpret_cast<const ivec4 *>(ent + k));   // read-once stream
        double w;
        const int wbits[2] = {r.z, r.w};
        __builtin_memcpy(&w, wbits, 8);
        val = w * data[(unsigned)r.x];
        key = r.y;
    }
#pragma unroll
    for (int o = 1; o < kWave; o <<= 1) {
        const double pv = __shfl_up(val, o, kWave);
        const int pk = __shfl_up(key, o, kWave);
        if (lane >= o && pk == key) val += pv;
    }
    const int nk = __shfl_down(key, 1, kWave);
    if (k < n && (lane == kWave - 1 || k == n - 1 || nk != key)) runsum[k] = val;
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
// ws.nseg segments (seg_start for the records, ent_start for the unique-edge entries) and goes to row + r * row_stride
static void launch_finalize(const WeightSet &ws, const int *run_start, long nrun, const double *runsum,
                            const int *tr_offsets_dev, int ntransect, double *row, long row_stride, unsigned nrows,
                            hipStream_t s)
{
    if (ws.nseg > 0) {
        const unsigned nb = (unsigned)(((long)ws.nseg * kWave + kBlock - 1) / kBlock);
        hipLaunchKernelGGL(k_finalize_seg, dim3(nb, nrows), dim3(kBlock), 0, s, runsum, run_start, ws.nseg, row, nrun,
                           row_stride);
    }
    if (ntransect > 0) {
        const unsigned nb = (unsigned)(((long)ntransect * kWave + kBlock - 1) / kBlock);
        hipLaunchKernelGGL(k_finalize_tr, dim3(nb, nrows), dim3(kBlock), 0, s, tr_offsets_dev, ntransect, ws.nseg, row,
                           row_stride);
    }
}

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
    const unsigned ny = (unsigned)(nsteps > 1 ? nsteps : 1);
    if (planes == 2 && ws.ent_start.get() && g_use_edges) {   // the engine's own planes through the unique-edge entries
        if (ws.nent > 0)
            hipLaunchKernelGGL(k_gather_edges, dim3((unsigned)((ws.nent + kBlock - 1) / kBlock), ny), dim3(kBlock), 0, s,
                               ws.ent.get(), ws.nent, data, ncell, scratch, data_stride);
        launch_finalize(ws, ws.ent_start.get(), ws.nent, scratch, tr_offsets_dev, ntransect, row, row_stride, ny, s);
        NF_HIP(hipGetLastError());
        return NF_OK;
    }
    if (ws.nrec > 0) {
        hipLaunchKernelGGL(k_gather_segscan, dim3((unsigned)((ws.nrec + kBlock - 1) / kBlock), ny), dim3(kBlock), 0, s,
                           rec_cells ? rec_cells : ws.cell.get(), ws.w4.get(), ws.seg.get(), ws.nrec, data, ncell, planes,
                           (unsigned)(nx > 0 ? nx : 1), scratch, data_stride);
    }
    launch_finalize(ws, ws.seg_start.get(), ws.nrec, scratch, tr_offsets_dev, ntransect, row, row_stride, ny, s);
    NF_HIP(hipGetLastError());
    return NF_OK;
}

int launch_integral_pair(const WeightSet &ws, const double *uvA, const double *uvB, long ncell, long nx,
                         const int *tr_offsets_dev, int ntransect, double *scratch, double *row, long row_stride,
                         hipStream_t s)
{
    if (ws.nrec > 0)
        hipLaunchKernelGGL(k_gather_segscan_pair, dim3((unsigned)((ws.nrec + kBlock - 1) / kBlock)), dim3(kBlock), 0, s,
                           ws.cell.get(), ws.w4.get(), ws.seg.get(), ws.nrec, uvA, uvB, ncell, (unsigned)(nx > 0 ? nx : 1),
                           scratch);
    launch_finalize(ws, ws.seg_start.get(), ws.nrec, scratch, tr_offsets_dev, ntransect, row, row_stride, 2, s);
    NF_HIP(hipGetLastError());
    return NF_OK;
}

// ---- depth-resolved rows: stage A of the record form, one level at a time, straight from the raw fields ------------------
// Level z's edge values are formed on the fly exactly as K1 forms them for a field whose only non-zero layer is z:
// eU(c) = +fma(th[z], fixed(u[z,c]), 0) * arcE[c], eV(c) = -fma(th[z], fixed(v[z,c]), 0) * arcN[c], times the Sverdrup
// scale; south = eV(c - nx) (0 on row 0), west = eU(c - 1) (periodic on column 0), the weighted sum with K3's association
// and K3's wavefront segmented scan (the flags of the scan depend on the keys only: computed once for all levels).  A lane
// owns one record and up to kProfileChunk levels: the 40-byte record and the four arc lengths are read once per chunk, the
// 4 x LZ gathers of a lane are all in flight together.  runsum: (levels of the launch) x n doubles, level-major.
template <typename T>
__device__ inline double profile_fixed(T x, T fill, T fill2, bool two)
{
    return (x != x || x == fill || (two && x == fill2)) ? 0.0 : (double)x;
}

template <typename T, int LZ>
__global__ __launch_bounds__(kBlock) void k_profile_segscan(const int *__restrict__ cell, const double *__restrict__ w4,
                                                            const int *__restrict__ seg, long n, const T *__restrict__ u,
                                                            const T *__restrict__ v, long ncell, unsigned nx, int z0,
                                                            int nlev, const double *__restrict__ thickness,
                                                            const double *__restrict__ arcE,
                                                            const double *__restrict__ arcN, T fill, T fill2, int two,
                                                            double scale, int sverdrup, double *__restrict__ runsum)
{
    const long k = (long)blockIdx.x * kBlock + threadIdx.x;
    const int lane = threadIdx.x & (kWave - 1);
    double val[LZ];
#pragma unroll
    for (int l = 0; l < LZ; ++l) val[l] = 0.0;
    int key = -1;
    if (k < n) {
        typedef double dvec2 __attribute__((ext_vector_type(2)));
        const long c = __builtin_nontemporal_load(cell + k);
        const dvec2 *pw = reinterpret_cast<const dvec2 *>(w4 + 4 * k);
        const dvec2 wa = __builtin_nontemporal_load(pw), wb = __builtin_nontemporal_load(pw + 1);
        key = __builtin_nontemporal_load(seg + k);
        const unsigned j = (unsigned)(c / nx), i = (unsigned)(c - (long)j * nx);
        const bool south = j > 0;
        const long cs = south ? c - nx : c;             // row 0: no south value (read, then discarded)
        const long cw = i > 0 ? c - 1 : c - 1 + nx;
        const double aEc = arcE[c], aNc = arcN[c], aNs = arcN[cs], aEw = arcE[cw];
        T uc[LZ], uw[LZ], vc[LZ], vs[LZ];
#pragma unroll
        for (int l = 0; l < LZ; ++l)
            if (l < nlev) {   // launch-uniform
                const long o = (long)(z0 + l) * ncell;
                uc[l] = u[o + c];
                uw[l] = u[o + cw];
                vc[l] = v[o + c];
                vs[l] = v[o + cs];
            }
#pragma unroll
        for (int l = 0; l < LZ; ++l)
            if (l < nlev) {
                const double th = thickness[z0 + l];
                double d1 = +fma(th, profile_fixed<T>(uc[l], fill, fill2, two), 0.0) * aEc;
                double d3 = +fma(th, profile_fixed<T>(uw[l], fill, fill2, two), 0.0) * aEw;
                double d2 = -fma(th, profile_fixed<T>(vc[l], fill, fill2, two), 0.0) * aNc;
                double d0 = -fma(th, profile_fixed<T>(vs[l], fill, fill2, two), 0.0) * aNs;
                if (sverdrup) {
                    d0 *= scale;
                    d1 *= scale;
                    d2 *= scale;
                    d3 *= scale;
                }
                if (!south) d0 = 0.0;
                // the library is built with -ffp-contract=off: the same rounded products and sums as k_gather_segscan
                val[l] = ((wa.x * d0 + wa.y * d1) + wb.x * d2) + wb.y * d3;
            }
    }
#pragma unroll
    for (int o = 1; o < kWave; o <<= 1) {
        const int pk = __shfl_up(key, o, kWave);
        const bool take = lane >= o && pk == key;
#pragma unroll
        for (int l = 0; l < LZ; ++l) {
            const double pv = __shfl_up(val[l], o, kWave);
            if (take) val[l] += pv;
        }
    }
    const int nk = __shfl_down(key, 1, kWave);
    if (k < n && (lane == kWave - 1 || k == n - 1 || nk != key)) {
#pragma unroll
        for (int l = 0; l < LZ; ++l)
            if (l < nlev) runsum[(long)l * n + k] = val[l];
    }
}

template <typename T>
static int launch_profile_t(const ProfileArgs &a, hipStream_t s)
{
    const WeightSet &ws = *a.ws;
    const StepInput &in = a.in;
    const T fill = (T)in.fill, fill2 = (T)in.fill2;
    const int two = fill2 == fill2 && !(fill2 == fill);   // K1's rule: a second marker that differs from the first
    for (int zc = in.z0; zc < in.z1; zc += kProfileChunk) {
        const int nlev = in.z1 - zc < kProfileChunk ? in.z1 - zc : kProfileChunk;
        double *rows = a.prof + (long)zc * a.row_length;
        if (ws.nrec > 0)
            hipLaunchKernelGGL((k_profile_segscan<T, kProfileChunk>), dim3((unsigned)((ws.nrec + kBlock - 1) / kBlock)),
                               dim3(kBlock), 0, s, ws.cell.get(), ws.w4.get(), ws.seg.get(), ws.nrec, (const T *)in.u,
                               (const T *)in.v, in.ncell, (unsigned)in.nx, zc, nlev, in.thickness, in.arcE, in.arcN, fill,
                               fill2, two, in.scale, in.sverdrup, a.scratch);
        launch_finalize(ws, ws.seg_start.get(), ws.nrec, a.scratch, a.tr_offsets_dev, a.ntransect, rows, a.row_length,
                        (unsigned)nlev, s);
        NF_HIP(hipGetLastError());
    }
    return NF_OK;
}

int launch_profile(const ProfileArgs &a, hipStream_t s)
{
    const StepInput &in = a.in;
    NF_REQUIRE(a.ws && in.ncell > 0 && in.nx > 0 && in.ncell % in.nx == 0 && in.ncell < (1l << 31), NF_ERR_ARG,
               "profile: bad grid sizes");
    NF_REQUIRE(in.z0 >= 0 && in.z1 >= in.z0 && a.row_length == a.ws->nseg + a.ntransect, NF_ERR_ARG, "profile: bad arguments");
    NF_REQUIRE(a.scratch_len >= (size_t)a.ws->nrec * kProfileChunk, NF_ERR_ARG, "profile: scratch too small");
    if (a.row_length == 0) return NF_OK;
    if (in.dtype == NF_F64) return launch_profile_t<double>(a, s);
    if (in.dtype == NF_F32) return launch_profile_t<float>(a, s);
    NF_REQUIRE(false, NF_ERR_ARG, "profile: dtype must be NF_F64 or NF_F32");
}

// ---- volume transport in tracer classes: the profile kernel's terms, each sent to the row of its face's class ----------------
// One lane per record, K3's record order and 64-record waves.  Per owned level (z ascending) the four slot terms are the
// ones of k_profile_segscan; each is added, in slot order (south, east, north, west), to the lane's accumulator of the row
// that its own face's class value selects, when that row lies in the window [r0, r0 + nwin).  The accumulators are a column
// of LDS per lane (a dynamic row index in registers would go to scratch).  Then K3's segmented scan runs once per row of the
// window.  With one class per level (tau = z) a row gets exactly one level's four terms, added as ((0 + t0) + t1) + t2) + t3:
// the profile's ((t0 + t1) + t2) + t3, bit for bit.
//   faces: east(c) = (tau[c], tau[c+1]; column nx-1: tau[c+1-nx] when wrap_x, else none), north(c) = (tau[c], tau[c+nx];
//   last row: none), the west slot is east(cw), the south slot north(cs).
// LDS: the edges (nedges doubles, padded to even), then nwin x kBlock accumulators.
constexpr int kClassLevels = 4;   // levels whose 9 gathers are issued together

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

template <typename T>
__global__ __launch_bounds__(kBlock) void k_class_segscan(const int *__restrict__ cell, const double *__restrict__ w4,
                                                          const int *__restrict__ seg, long n, const T *__restrict__ u,
                                                          const T *__restrict__ v, const T *__restrict__ tau, long ncell,
                                                          unsigned nx, int z0, int z1, const double *__restrict__ thickness,
                                                          const double *__restrict__ arcE, const double *__restrict__ arcN,
                                                          T fill, T fill2, int two, T tfill, T tfill2, int wrap_x,
                                                          double scale, int sverdrup, const double *__restrict__ edges,
                                                          int nedges, int top, int r0, int nwin, double *__restrict__ runsum)
{
    extern __shared__ double class_lds[];
    double *e = class_lds;
    double *acc = class_lds + ((nedges + 1) & ~1) + threadIdx.x;   // acc[r * kBlock]: this lane's row r
    for (int q = threadIdx.x; q < nedges; q += kBlock) e[q] = edges[q];
    for (int r = 0; r < nwin; ++r) acc[r * kBlock] = 0.0;
    __syncthreads();   // the edges; every lane touches only its own accumulators
    const long k = (long)blockIdx.x * kBlock + threadIdx.x;
    const int lane = threadIdx.x & (kWave - 1);
    int key = -1;
    if (k < n) {
        typedef double dvec2 __attribute__((ext_vector_type(2)));
        const long c = __builtin_nontemporal_load(cell + k);
        const dvec2 *pw = reinterpret_cast<const dvec2 *>(w4 + 4 * k);
        const dvec2 wa = __builtin_nontemporal_load(pw), wb = __builtin_nontemporal_load(pw + 1);
        key = __builtin_nontemporal_load(seg + k);
        const unsigned j = (unsigned)(c / nx), i = (unsigned)(c - (long)j * nx);
        const bool south = j > 0;
        const bool has_e = i + 1 < nx || wrap_x, has_n = c + (long)nx < ncell, has_w = i > 0 || wrap_x;
        const long cs = south ? c - nx : c;             // row 0: no south value (read, then discarded)
        const long cw = i > 0 ? c - 1 : c - 1 + nx;
        const long ce = i + 1 < nx ? c + 1 : (wrap_x ? c + 1 - (long)nx : c);
        const long cn = has_n ? c + nx : c;
        const double aEc = arcE[c], aNc = arcN[c], aNs = arcN[cs], aEw = arcE[cw];
        auto add = [&](int row, double x) {
            const int r = row - r0;
            if (r >= 0 && r < nwin) acc[r * kBlock] += x;
        };
        for (int z = z0; z < z1; z += kClassLevels) {
            const int nlev = z1 - z < kClassLevels ? z1 - z : kClassLevels;
            T uc[kClassLevels], uw[kClassLevels], vc[kClassLevels], vs[kClassLevels];
            T tc[kClassLevels], te[kClassLevels], tn[kClassLevels], tw[kClassLevels], ts[kClassLevels];
#pragma unroll
            for (int l = 0; l < kClassLevels; ++l)
                if (l < nlev) {
                    const long o = (long)(z + l) * ncell;
                    uc[l] = u[o + c];
                    uw[l] = u[o + cw];
                    vc[l] = v[o + c];
                    vs[l] = v[o + cs];
                    tc[l] = tau[o + c];
                    te[l] = tau[o + ce];
                    tn[l] = tau[o + cn];
                    tw[l] = tau[o + cw];
                    ts[l] = tau[o + cs];
                }
#pragma unroll
            for (int l = 0; l < kClassLevels; ++l)
                if (l < nlev) {
                    const double th = thickness[z + l];
                    double d1 = +fma(th, profile_fixed<T>(uc[l], fill, fill2, two), 0.0) * aEc;
                    double d3 = +fma(th, profile_fixed<T>(uw[l], fill, fill2, two), 0.0) * aEw;
                    double d2 = -fma(th, profile_fixed<T>(vc[l], fill, fill2, two), 0.0) * aNc;
                    double d0 = -fma(th, profile_fixed<T>(vs[l], fill, fill2, two), 0.0) * aNs;
                    if (sverdrup) {
                        d0 *= scale;
                        d1 *= scale;
                        d2 *= scale;
                        d3 *= scale;
                    }
                    double x;
                    bool h;
                    if (south) {
                        h = tr_face_raw<T>(ts[l], tc[l], true, tfill, tfill2, &x);
                        add(class_row(h, x, e, nedges, top), wa.x * d0);
                    }
                    h = tr_face_raw<T>(tc[l], te[l], has_e, tfill, tfill2, &x);
                    add(class_row(h, x, e, nedges, top), wa.y * d1);
                    h = tr_face_raw<T>(tc[l], tn[l], has_n, tfill, tfill2, &x);
                    add(class_row(h, x, e, nedges, top), wb.x * d2);
                    h = tr_face_raw<T>(tw[l], tc[l], has_w, tfill, tfill2, &x);
                    add(class_row(h, x, e, nedges, top), wb.y * d3);
                }
        }
    }
    // K3's segmented scan, once per row of the window; its flags depend on the keys only
    unsigned take = 0;
#pragma unroll
    for (int o = 1, b = 0; o < kWave; o <<= 1, ++b) {
        const int pk = __shfl_up(key, o, kWave);
        if (lane >= o && pk == key) take |= 1u << b;
    }
    const int nk = __shfl_down(key, 1, kWave);
    const bool store = k < n && (lane == kWave - 1 || k == n - 1 || nk != key);
    for (int r = 0; r < nwin; ++r) {
        double val = k < n ? acc[r * kBlock] : 0.0;
#pragma unroll
        for (int o = 1, b = 0; o < kWave; o <<= 1, ++b) {
            const double pv = __shfl_up(val, o, kWave);
            if (take & (1u << b)) val += pv;
        }
        if (store) runsum[(long)r * n + k] = val;
    }
}

template <typename T>
static int launch_class_t(const ClassArgs &a, hipStream_t s)
{
    const WeightSet &ws = *a.ws;
    const StepInput &in = a.in;
    const T fill = (T)in.fill, fill2 = (T)in.fill2;
    const int two = fill2 == fill2 && !(fill2 == fill);   // K1's rule: a second marker that differs from the first
    int top = 1;
    while (2 * top <= a.nedges) top *= 2;
    const int nrows = a.nedges + 2;
    for (int r0 = 0; r0 < nrows; r0 += a.window) {
        const int nwin = nrows - r0 < a.window ? nrows - r0 : a.window;
        const size_t lds = sizeof(double) * ((size_t)((a.nedges + 1) & ~1) + (size_t)nwin * kBlock);
        if (ws.nrec > 0) {
            if (lds > 65536)
                NF_HIP(hipFuncSetAttribute(reinterpret_cast<const void *>(&k_class_segscan<T>),
                                           hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
            hipLaunchKernelGGL(k_class_segscan<T>, dim3((unsigned)((ws.nrec + kBlock - 1) / kBlock)), dim3(kBlock), lds, s,
                               ws.cell.get(), ws.w4.get(), ws.seg.get(), ws.nrec, (const T *)in.u, (const T *)in.v,
                               (const T *)a.tau, in.ncell, (unsigned)in.nx, in.z0, in.z1, in.thickness, in.arcE, in.arcN,
                               fill, fill2, two, (T)a.tfill, (T)a.tfill2, a.wrap_x ? 1 : 0, in.scale, in.sverdrup, a.edges,
                               a.nedges, top, r0, nwin, a.scratch);
        }
        launch_finalize(ws, ws.seg_start.get(), ws.nrec, a.scratch, a.tr_offsets_dev, a.ntransect,
                        a.rows + (long)r0 * a.row_length, a.row_length, (unsigned)nwin, s);
        NF_HIP(hipGetLastError());
    }
    return NF_OK;
}

int launch_class_transport(const ClassArgs &a, hipStream_t s)
{
    const StepInput &in = a.in;
    NF_REQUIRE(a.ws && in.ncell > 0 && in.nx > 0 && in.ncell % in.nx == 0 && in.ncell < (1l << 31), NF_ERR_ARG,
               "class transport: bad grid sizes");
    NF_REQUIRE(in.z0 >= 0 && in.z1 >= in.z0 && a.row_length == a.ws->nseg + a.ntransect, NF_ERR_ARG,
               "class transport: bad arguments");
    NF_REQUIRE(a.nedges >= 2 && a.nedges <= kMaxClassEdges && a.edges, NF_ERR_ARG, "class transport: bad class edges");
    NF_REQUIRE(a.window >= 1 && a.window <= kClassWindowMax, NF_ERR_ARG, "class transport: bad window");
    NF_REQUIRE(a.scratch_len >= (size_t)a.ws->nrec * a.window, NF_ERR_ARG, "class transport: scratch too small");
    NF_REQUIRE(in.u && in.v && a.tau && a.rows && in.thickness && in.arcE && in.arcN, NF_ERR_ARG,
               "class transport: null argument");
    if (a.row_length == 0) return NF_OK;
    if (in.dtype == NF_F64) return launch_class_t<double>(a, s);
    if (in.dtype == NF_F32) return launch_class_t<float>(a, s);
    NF_REQUIRE(false, NF_ERR_ARG, "class transport: dtype must be NF_F64 or NF_F32");
}

}  // namespace nf
