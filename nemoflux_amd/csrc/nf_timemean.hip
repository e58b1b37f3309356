// nf_timemean.hip -- the time mean of a series of arrays (nf_time_mean, Field.timeMean): one streaming, bandwidth-bound pass
// over nsteps arrays of n values each.
//
// Definition, per value i, the steps visited strictly in ascending order:
//   s = +0.0, c = 0                      (or the s, c a previous call left in acc / cnt)
//   x = src[t * stride + i];             x present:  s = s + (double)x,  c += 1
// "Present" is the engine's rule (uv_fixed / tr_present of nf_common.h): not NaN and equal to neither marker, each marker cast
// to the array's dtype and compared in that dtype; +-inf is present.  There is no other arithmetic and no reassociation: s is
// the left-to-right float64 sum whatever the launch shape or the grouping of the steps into calls, so a series split over
// several calls gives the bits of one call and a numpy loop reproduces them.  The last call finishes in place:
//   NF_MEAN_OVER_STEPS    s / total_steps   (velocities: a missing one counts as 0, as in every flux kernel)
//   NF_MEAN_OVER_PRESENT  s / c             (tracers)
// and fill_out where c == 0 under both rules.
//
// Access pattern.  A lane owns 16 consecutive bytes of the value axis (2 doubles or 4 floats) and walks the steps with stride
// `stride`; the loads of a batch of steps -- one aligned, read-once (non-temporal) 16-byte load per step -- are issued before
// the first add, the adds of the batch then run in step order.  acc leaves in 16-byte stores.  When some step is not 16-byte
// aligned (an odd n with stride = n, an odd base pointer) the same code runs with one value per lane: the same bits.  All
// offsets are 64-bit (step 5 of a 3600 x 1800 x 75 series starts beyond 2^31 elements).
//
// Algorithmic bytes of a first && last call: nsteps * n * sizeof(T) read + 8 n written; a carried call adds 12 n each way.
//
// The thickness-weighted mean (nf_time_mean_weighted, Field.timeMean(thicknessWeighted=True)) reads two series at once, a
// velocity and the cell thickness at its points.  Per value i, the steps visited strictly in ascending order:
//   sF = +0.0, sH = +0.0, c = 0          (or what the previous call left in accf / acch / cnt)
//   h = fixth(thk[t * thk_stride + i])   thick_fixed of nf_common.h: NaN or one of the thickness's two markers -> 0
//   sH = sH + h                          at every step
//   x = src[t * src_stride + i];         x present (the rule above, src's own markers):  sF = sF + (h * (double)x),  c += 1
// The product is rounded, then added (-ffp-contract=off: no fma).  The last call finishes in place:
//   accf = c == 0 ? fill_out : (sH == 0 ? +0.0 : sF / sH)      the weighted mean velocity
//   acch = sH / total_steps                                    the mean thickness
// so that acch * accf is the mean volume flux per unit width, face by face.  Same access pattern with two loads per step and
// lane; 2 * nsteps * n * sizeof(T) read + 16 n written by a first && last call, a carried call adds 20 n each way.
//
// Selected, weighted steps (nf_time_mean_steps, nf_time_mean_weighted_steps; Field.timeMean(select=, weights=)).  The steps
// are a table of element offsets from src (any order, repeats allowed) with one float64 weight each, walked strictly in
// table order j = 0 .. nsteps - 1.  Per value i:
//   x = src[off_j + i];   x present:  s = s + (w_j * (double)x),  wp = wp + w_j,  c += 1        the product rounded, then added
// and the last call finishes with s / total_weight (NF_MEAN_OVER_STEPS) or s / wp (NF_MEAN_OVER_PRESENT), fill_out where
// c == 0.  The thickness-weighted form takes g = w_j * fixth(h), rounded:  sH = sH + g at every step,  sF = sF + (g *
// (double)x) where x is present, and finishes as nf_time_mean_weighted does with total_weight for total_steps.  With unit
// weights 1 * x is exact, wp == c and total_weight == total_steps: the bits of the two calls above.
// How the table reaches the kernel: as a kernel argument, kTmTable = 16 steps a launch -- 16 offsets and 16 weights, 256
// bytes (384 with the second series' offsets) of the kernarg segment, read by scalar loads at constant indices, so they are
// wave-uniform and cost no HBM traffic and no allocation.  A longer table goes in launches of 16 steps chained through first /
// last on the stream: each further launch carries acc, cnt and (NF_MEAN_OVER_PRESENT) wsum, 12 n or 20 n bytes each way (28
// n for the weighted form, which has no wsum).  A carried array the caller did not give (allowed when first && last) is
// allocated and freed on the stream for such a chain.  Nothing synchronises: the calls are asynchronous on hip_stream.
// The access pattern is the one above; when any listed step, acc, wsum or cnt is not 16-byte aligned the whole call, every
// launch of it, takes one value per lane.
#include "nf_capi.h"
#include "nf_lanes.h"

namespace nf {

namespace {

struct TmFinish {
    int first, last, rule;
    double total_steps, fill_out;
};

// VEC float64 sums at p, 16 bytes at a time
template <int VEC>
__device__ inline void tm_load_sums(double (&s)[VEC], const double *p)
{
#pragma unroll
    for (int k = 0; k < VEC; k += 2) {
        constexpr int W = VEC > 1 ? 2 : 1;
        const Lanes<double, W> a = lane_load<double, W, false>(p + k);
#pragma unroll
        for (int q = 0; q < W; ++q) s[k + q] = a.x[q];
    }
}
template <int VEC>
__device__ inline void tm_store_sums(double *p, const double (&s)[VEC])
{
#pragma unroll
    for (int k = 0; k < VEC; k += 2) {
        constexpr int W = VEC > 1 ? 2 : 1;
        Lanes<double, W> a;
#pragma unroll
        for (int q = 0; q < W; ++q) a.x[q] = s[k + q];
        lane_store<double, W>(p + k, a);
    }
}

// the VEC values that begin at i0: US steps' loads in flight, the adds in step order.  acc is read and written here as
// tm_load_sums / tm_store_sums do it, written out: through the two helpers the compiler allocates and schedules
// k_time_mean<float, 4, 8> differently (612 of its 951 instructions, one more of them), and the kernels stay as measured.
template <typename T, int VEC, int US>
__device__ inline void tm_lane(double *acc, unsigned *cnt, const T *src, long nsteps, long long stride, size_t i0, T m1, T m2,
                               const TmFinish &f)
{
    double s[VEC];
    unsigned c[VEC];
    if (f.first) {
#pragma unroll
        for (int k = 0; k < VEC; ++k) s[k] = 0.0, c[k] = 0u;
    } else {
#pragma unroll
        for (int k = 0; k < VEC; k += 2) {   // 16 bytes of acc at a time
            constexpr int W = VEC > 1 ? 2 : 1;
            const Lanes<double, W> a = lane_load<double, W, false>(acc + i0 + k);
#pragma unroll
            for (int q = 0; q < W; ++q) s[k + q] = a.x[q];
        }
        const Lanes<unsigned, VEC> n0 = lane_load<unsigned, VEC, false>(cnt + i0);
#pragma unroll
        for (int k = 0; k < VEC; ++k) c[k] = n0.x[k];
    }
    const T *p = src + i0;
    for (long t = 0; t < nsteps; t += US) {
        const int nb = nsteps - t < US ? (int)(nsteps - t) : US;   // wave-uniform
        Lanes<T, VEC> x[US];
#pragma unroll
        for (int r = 0; r < US; ++r)
            if (r < nb) x[r] = lane_load<T, VEC, true>(p + (long long)r * stride);
#pragma unroll
        for (int r = 0; r < US; ++r)
            if (r < nb) {
#pragma unroll
                for (int k = 0; k < VEC; ++k) {
                    const bool here = tr_present<T>(x[r].x[k], m1, m2);
                    s[k] = here ? s[k] + (double)x[r].x[k] : s[k];
                    c[k] += here ? 1u : 0u;
                }
            }
        p += (long long)US * stride;
    }
    if (f.last) {
#pragma unroll
        for (int k = 0; k < VEC; ++k)
            s[k] = c[k] == 0u ? f.fill_out : (f.rule == NF_MEAN_OVER_STEPS ? s[k] / f.total_steps : s[k] / (double)c[k]);
    } else {
        Lanes<unsigned, VEC> n1;
#pragma unroll
        for (int k = 0; k < VEC; ++k) n1.x[k] = c[k];
        lane_store<unsigned, VEC>(cnt + i0, n1);
    }
#pragma unroll
    for (int k = 0; k < VEC; k += 2) {
        constexpr int W = VEC > 1 ? 2 : 1;
        Lanes<double, W> a;
#pragma unroll
        for (int q = 0; q < W; ++q) a.x[q] = s[k + q];
        lane_store<double, W>(acc + i0 + k, a);
    }
}

template <typename T> struct TmwSeries {
    const T *src, *thk;
    long long src_stride, thk_stride;
    T m1, m2, h1, h2;     // the markers of src, of thk
};

// the weighted form of tm_lane: the VEC values that begin at i0, two loads per step, US steps' loads in flight, the adds in
// step order.  f.rule is not read.
template <typename T, int VEC, int US>
__device__ inline void tmw_lane(double *accf, double *acch, unsigned *cnt, const TmwSeries<T> &in, long nsteps, size_t i0,
                                const TmFinish &f)
{
    double sF[VEC], sH[VEC];
    unsigned c[VEC];
    if (f.first) {
#pragma unroll
        for (int k = 0; k < VEC; ++k) sF[k] = 0.0, sH[k] = 0.0, c[k] = 0u;
    } else {
        tm_load_sums<VEC>(sF, accf + i0);
        tm_load_sums<VEC>(sH, acch + i0);
        const Lanes<unsigned, VEC> n0 = lane_load<unsigned, VEC, false>(cnt + i0);
#pragma unroll
        for (int k = 0; k < VEC; ++k) c[k] = n0.x[k];
    }
    const T *p = in.src + i0, *q = in.thk + i0;
    for (long t = 0; t < nsteps; t += US) {
        const int nb = nsteps - t < US ? (int)(nsteps - t) : US;   // wave-uniform
        Lanes<T, VEC> x[US], h[US];
#pragma unroll
        for (int r = 0; r < US; ++r)
            if (r < nb) {
                x[r] = lane_load<T, VEC, true>(p + (long long)r * in.src_stride);
                h[r] = lane_load<T, VEC, true>(q + (long long)r * in.thk_stride);
            }
#pragma unroll
        for (int r = 0; r < US; ++r)
            if (r < nb) {
#pragma unroll
                for (int k = 0; k < VEC; ++k) {
                    const double hh = thick_fixed<T>(h[r].x[k], in.h1, in.h2);
                    sH[k] = sH[k] + hh;
                    const bool here = tr_present<T>(x[r].x[k], in.m1, in.m2);
                    const double prod = hh * (double)x[r].x[k];     // rounded, then added: no fma (-ffp-contract=off)
                    sF[k] = here ? sF[k] + prod : sF[k];
                    c[k] += here ? 1u : 0u;
                }
            }
        p += (long long)US * in.src_stride;
        q += (long long)US * in.thk_stride;
    }
    if (f.last) {
#pragma unroll
        for (int k = 0; k < VEC; ++k) {
            sF[k] = c[k] == 0u ? f.fill_out : (sH[k] == 0.0 ? 0.0 : sF[k] / sH[k]);
            sH[k] = sH[k] / f.total_steps;
        }
    } else {
        Lanes<unsigned, VEC> n1;
#pragma unroll
        for (int k = 0; k < VEC; ++k) n1.x[k] = c[k];
        lane_store<unsigned, VEC>(cnt + i0, n1);
    }
    tm_store_sums<VEC>(accf + i0, sF);
    tm_store_sums<VEC>(acch + i0, sH);
}

// ---- selected, weighted steps: the table of one launch is a kernel argument (file header)
constexpr int kTmTable = 16;

struct TmsTable {
    long long off[kTmTable];    // elements from src
    double w[kTmTable];
};
struct TmwsTable {
    long long off[kTmTable], thk_off[kTmTable];
    double w[kTmTable];
};

// tm_lane over the first nsteps (1 .. kTmTable) entries of a table; f.total_steps is the total weight.  Both loops are
// unrolled over the whole table, so every index into it is a constant and the entries are scalar loads from the kernarg
// segment; the entries beyond nsteps are skipped by wave-uniform branches.  wsum is read and written under
// NF_MEAN_OVER_PRESENT only.
template <typename T, int VEC, int US>
__device__ inline void tms_lane(double *acc, double *wsum, unsigned *cnt, const T *src, const TmsTable &tab, int nsteps,
                                size_t i0, T m1, T m2, const TmFinish &f)
{
    const bool over_present = f.rule == NF_MEAN_OVER_PRESENT;
    double s[VEC], wp[VEC];
    unsigned c[VEC];
#pragma unroll
    for (int k = 0; k < VEC; ++k) s[k] = 0.0, wp[k] = 0.0, c[k] = 0u;
    if (!f.first) {
        tm_load_sums<VEC>(s, acc + i0);
        if (over_present) tm_load_sums<VEC>(wp, wsum + i0);
        const Lanes<unsigned, VEC> n0 = lane_load<unsigned, VEC, false>(cnt + i0);
#pragma unroll
        for (int k = 0; k < VEC; ++k) c[k] = n0.x[k];
    }
    const T *p = src + i0;
#pragma unroll
    for (int t = 0; t < kTmTable; t += US) {
        if (t >= nsteps) break;
        Lanes<T, VEC> x[US];
#pragma unroll
        for (int r = 0; r < US; ++r)
            if (t + r < nsteps) x[r] = lane_load<T, VEC, true>(p + tab.off[t + r]);
#pragma unroll
        for (int r = 0; r < US; ++r)
            if (t + r < nsteps) {
                const double w = tab.w[t + r];
#pragma unroll
                for (int k = 0; k < VEC; ++k) {
                    const bool here = tr_present<T>(x[r].x[k], m1, m2);
                    const double prod = w * (double)x[r].x[k];      // rounded, then added: no fma (-ffp-contract=off)
                    s[k] = here ? s[k] + prod : s[k];
                    wp[k] = here ? wp[k] + w : wp[k];
                    c[k] += here ? 1u : 0u;
                }
            }
    }
    if (f.last) {
#pragma unroll
        for (int k = 0; k < VEC; ++k)
            s[k] = c[k] == 0u ? f.fill_out : (over_present ? s[k] / wp[k] : s[k] / f.total_steps);
    } else {
        Lanes<unsigned, VEC> n1;
#pragma unroll
        for (int k = 0; k < VEC; ++k) n1.x[k] = c[k];
        lane_store<unsigned, VEC>(cnt + i0, n1);
        if (over_present) tm_store_sums<VEC>(wsum + i0, wp);
    }
    tm_store_sums<VEC>(acc + i0, s);
}

// tmw_lane over the first nsteps (1 .. kTmTable) entries of a table, built as tms_lane; f.rule is not read
template <typename T, int VEC, int US>
__device__ inline void tmws_lane(double *accf, double *acch, unsigned *cnt, const T *src, const T *thk, const TmwsTable &tab,
                                 int nsteps, size_t i0, T m1, T m2, T h1, T h2, const TmFinish &f)
{
    double sF[VEC], sH[VEC];
    unsigned c[VEC];
    if (f.first) {
#pragma unroll
        for (int k = 0; k < VEC; ++k) sF[k] = 0.0, sH[k] = 0.0, c[k] = 0u;
    } else {
        tm_load_sums<VEC>(sF, accf + i0);
        tm_load_sums<VEC>(sH, acch + i0);
        const Lanes<unsigned, VEC> n0 = lane_load<unsigned, VEC, false>(cnt + i0);
#pragma unroll
        for (int k = 0; k < VEC; ++k) c[k] = n0.x[k];
    }
    const T *p = src + i0, *q = thk + i0;
#pragma unroll
    for (int t = 0; t < kTmTable; t += US) {
        if (t >= nsteps) break;
        Lanes<T, VEC> x[US], h[US];
#pragma unroll
        for (int r = 0; r < US; ++r)
            if (t + r < nsteps) {
                x[r] = lane_load<T, VEC, true>(p + tab.off[t + r]);
                h[r] = lane_load<T, VEC, true>(q + tab.thk_off[t + r]);
            }
#pragma unroll
        for (int r = 0; r < US; ++r)
            if (t + r < nsteps) {
                const double w = tab.w[t + r];
#pragma unroll
                for (int k = 0; k < VEC; ++k) {
                    const double g = w * thick_fixed<T>(h[r].x[k], h1, h2);     // rounded
                    sH[k] = sH[k] + g;
                    const bool here = tr_present<T>(x[r].x[k], m1, m2);
                    const double prod = g * (double)x[r].x[k];                  // rounded, then added
                    sF[k] = here ? sF[k] + prod : sF[k];
                    c[k] += here ? 1u : 0u;
                }
            }
    }
    if (f.last) {
#pragma unroll
        for (int k = 0; k < VEC; ++k) {
            sF[k] = c[k] == 0u ? f.fill_out : (sH[k] == 0.0 ? 0.0 : sF[k] / sH[k]);
            sH[k] = sH[k] / f.total_steps;
        }
    } else {
        Lanes<unsigned, VEC> n1;
#pragma unroll
        for (int k = 0; k < VEC; ++k) n1.x[k] = c[k];
        lane_store<unsigned, VEC>(cnt + i0, n1);
    }
    tm_store_sums<VEC>(accf + i0, sF);
    tm_store_sums<VEC>(acch + i0, sH);
}

}  // namespace

// 256 threads, VEC values per lane, one tile of 256 * VEC values per block: i0 = (tile * 256 + tid) * VEC.  The tiles are dealt
// in K1's XCD bands (xcd_tile: every XCD streams one contiguous band of every step); the grid is xcd_grid(ntiles), tiles
// >= ntiles exit.  The one lane that holds fewer than VEC values (n is no multiple of VEC) takes them one at a time.
template <typename T, int VEC, int US>
__global__ __launch_bounds__(256) void k_time_mean(double *acc, unsigned *cnt, const T *__restrict__ src, long nsteps,
                                                   long long stride, size_t n, unsigned ntiles, T m1, T m2, TmFinish f)
{
    const unsigned tile = xcd_tile(blockIdx.x, gridDim.x);
    const size_t i0 = ((size_t)tile * 256 + threadIdx.x) * VEC;
    if (tile >= ntiles || i0 >= n) return;
    if (VEC == 1 || n - i0 >= (size_t)VEC) {
        tm_lane<T, VEC, US>(acc, cnt, src, nsteps, stride, i0, m1, m2, f);
        return;
    }
    for (size_t i = i0; i < n; ++i) tm_lane<T, 1, US>(acc, cnt, src, nsteps, stride, i, m1, m2, f);
}

// the same launch shape for the thickness-weighted mean: two series in, accf and acch out
template <typename T, int VEC, int US>
__global__ __launch_bounds__(256) void k_time_mean_weighted(double *accf, double *acch, unsigned *cnt, TmwSeries<T> in,
                                                            long nsteps, size_t n, unsigned ntiles, TmFinish f)
{
    const unsigned tile = xcd_tile(blockIdx.x, gridDim.x);
    const size_t i0 = ((size_t)tile * 256 + threadIdx.x) * VEC;
    if (tile >= ntiles || i0 >= n) return;
    if (VEC == 1 || n - i0 >= (size_t)VEC) {
        tmw_lane<T, VEC, US>(accf, acch, cnt, in, nsteps, i0, f);
        return;
    }
    for (size_t i = i0; i < n; ++i) tmw_lane<T, 1, US>(accf, acch, cnt, in, nsteps, i, f);
}

// the same launch shape for one launch's table of selected, weighted steps
template <typename T, int VEC, int US>
__global__ __launch_bounds__(256) void k_time_mean_steps(double *acc, double *wsum, unsigned *cnt, const T *__restrict__ src,
                                                         TmsTable tab, int nsteps, size_t n, unsigned ntiles, T m1, T m2,
                                                         TmFinish f)
{
    const unsigned tile = xcd_tile(blockIdx.x, gridDim.x);
    const size_t i0 = ((size_t)tile * 256 + threadIdx.x) * VEC;
    if (tile >= ntiles || i0 >= n) return;
    if (VEC == 1 || n - i0 >= (size_t)VEC) {
        tms_lane<T, VEC, US>(acc, wsum, cnt, src, tab, nsteps, i0, m1, m2, f);
        return;
    }
    for (size_t i = i0; i < n; ++i) tms_lane<T, 1, US>(acc, wsum, cnt, src, tab, nsteps, i, m1, m2, f);
}

template <typename T, int VEC, int US>
__global__ __launch_bounds__(256) void k_time_mean_weighted_steps(double *accf, double *acch, unsigned *cnt,
                                                                  const T *__restrict__ src, const T *__restrict__ thk,
                                                                  TmwsTable tab, int nsteps, size_t n, unsigned ntiles, T m1,
                                                                  T m2, T h1, T h2, TmFinish f)
{
    const unsigned tile = xcd_tile(blockIdx.x, gridDim.x);
    const size_t i0 = ((size_t)tile * 256 + threadIdx.x) * VEC;
    if (tile >= ntiles || i0 >= n) return;
    if (VEC == 1 || n - i0 >= (size_t)VEC) {
        tmws_lane<T, VEC, US>(accf, acch, cnt, src, thk, tab, nsteps, i0, m1, m2, h1, h2, f);
        return;
    }
    for (size_t i = i0; i < n; ++i) tmws_lane<T, 1, US>(accf, acch, cnt, src, thk, tab, nsteps, i, m1, m2, h1, h2, f);
}

namespace {

// Steps in flight per lane, one 16-byte load each (4 VGPRs): 44 VGPRs at float64, 52 at float32, 8 waves per SIMD, no
// scratch (-Rpass-analysis=kernel-resource-usage).  Measured at the bench shape while this was written and not kept
// (profiles/timemean_timing.txt): 4 or 12 steps in flight (within 1 %), two tiles per lane with all
// their loads in flight (within 1 % at float64, -4 to +6 % at float32), a capped grid whose blocks walk the tiles (5 to 10 %
// slower), plain instead of non-temporal loads or stores (no difference); the XCD bands are worth 6 % at float32, nothing
// at float64.
constexpr int kTimeMeanSteps = 8;

// one tile of 256 * VEC values per block: the number of tiles of n values, refused when one launch cannot hold them
template <int VEC>
int tm_tiles(size_t n, const char *what, unsigned *ntiles)
{
    const size_t per_block = 256u * (size_t)VEC, tiles = (n + per_block - 1) / per_block;
    NF_REQUIRE(tiles <= 0x7ffffff0u, NF_ERR_ARG, std::string(what) + ": n is too large for one launch");
    *ntiles = (unsigned)tiles;
    return NF_OK;
}

struct TimeMeanArgs {
    double *acc;
    unsigned *cnt;
    const void *src;
    long nsteps;
    long long stride;
    size_t n;
    double fill, missing;
    TmFinish f;
};

template <typename T, int VEC>
int launch_time_mean_v(const TimeMeanArgs &a, hipStream_t s)
{
    unsigned ntiles;
    NF_TRY(tm_tiles<VEC>(a.n, "nf_time_mean", &ntiles));
    hipLaunchKernelGGL((k_time_mean<T, VEC, kTimeMeanSteps>), dim3(xcd_grid(ntiles)), dim3(256), 0, s, a.acc, a.cnt,
                       (const T *)a.src, a.nsteps, a.stride, a.n, ntiles, (T)a.fill, (T)a.missing, a.f);
    NF_HIP(hipGetLastError());
    return NF_OK;
}

template <typename T, int VEC>
int launch_time_mean_t(const TimeMeanArgs &a, hipStream_t s)
{
    // every step, acc and cnt 16-byte aligned at every lane's first value: else one value per lane
    const bool al16 = lanes_aligned16({a.src, a.acc, a.cnt}, a.nsteps, {a.stride * (long long)sizeof(T)});
    return al16 ? launch_time_mean_v<T, VEC>(a, s) : launch_time_mean_v<T, 1>(a, s);
}

// Steps in flight per lane of the weighted form, two 16-byte loads each (8 VGPRs), so 4 steps keep the 128 bytes per lane in
// flight that k_time_mean has with 8.  VGPRs at float64 / float32 and waves per SIMD, none with scratch
// (-Rpass-analysis=kernel-resource-usage): 2 steps 35 / 50, 8 / 8 waves; 4 steps 54 / 64, 7 (102 SGPRs) / 8 waves; 8 steps
// 81 / 95, 5 / 5 waves.  Measured at the bench shape, two series of 3600 x 1800 x 75 x 12, each build in a process of its own
// beside nf_time_mean on one of the series (profiles/weighted_mean_timing.txt): 4 steps 16.44 ms at
// float64 and 9.44 ms at float32, 0.97 and 0.98 of nf_time_mean's fraction of the HBM peak in that process; 2 steps 17.24
// and 9.75 ms (1.02, 0.93); 8 steps 16.92 and 10.00 ms (0.93, 0.91).
constexpr int kTimeMeanWeightedSteps = 4;

struct TimeMeanWeightedArgs {
    double *accf, *acch;
    unsigned *cnt;
    const void *src, *thk;
    long long src_stride, thk_stride;
    long nsteps;
    size_t n;
    double fill, missing, thk_fill, thk_missing;
    TmFinish f;
};

template <typename T, int VEC>
int launch_time_mean_weighted_v(const TimeMeanWeightedArgs &a, hipStream_t s)
{
    unsigned ntiles;
    NF_TRY(tm_tiles<VEC>(a.n, "nf_time_mean_weighted", &ntiles));
    const TmwSeries<T> in{(const T *)a.src, (const T *)a.thk, a.src_stride, a.thk_stride,
                          (T)a.fill, (T)a.missing, (T)a.thk_fill, (T)a.thk_missing};
    hipLaunchKernelGGL((k_time_mean_weighted<T, VEC, kTimeMeanWeightedSteps>), dim3(xcd_grid(ntiles)), dim3(256), 0, s, a.accf,
                       a.acch, a.cnt, in, a.nsteps, a.n, ntiles, a.f);
    NF_HIP(hipGetLastError());
    return NF_OK;
}

template <typename T, int VEC>
int launch_time_mean_weighted_t(const TimeMeanWeightedArgs &a, hipStream_t s)
{
    // every step of both series, accf, acch and cnt 16-byte aligned at every lane's first value: else one value per lane
    const bool al16 = lanes_aligned16({a.src, a.thk, a.accf, a.acch, a.cnt}, a.nsteps,
                                      {a.src_stride * (long long)sizeof(T), a.thk_stride * (long long)sizeof(T)});
    return al16 ? launch_time_mean_weighted_v<T, VEC>(a, s) : launch_time_mean_weighted_v<T, 1>(a, s);
}

// ---- selected, weighted steps.  Steps in flight per lane as in the two kernels above (8, and 4 with two loads each); the
// table is held in scalar registers.  VGPRs / SGPRs / waves per SIMD of each instantiation
// (-Rpass-analysis=kernel-resource-usage), none with scratch:
//   k_time_mean_steps           <double, 2> 50 / 106 / 7   <float, 4> 62 / 106 / 7   <double, 1> 30 / 99 / 8   <float, 1> 22 / 100 / 8
//   k_time_mean_weighted_steps  <double, 2> 53 / 106 / 7   <float, 4> 67 / 106 / 7   <double, 1> 34 / 78 / 8   <float, 1> 26 / 74 / 8
// The 16-byte forms run 7 waves per SIMD where k_time_mean runs 8: the scalar registers of the table set that, not the VGPRs.

struct TimeMeanStepsArgs {
    double *acc, *wsum;
    unsigned *cnt;
    const void *src, *thk;                              // thk, thk_off: the weighted form (acc = accf, wsum = acch)
    const long long *off, *thk_off;
    const double *weights;                              // null: all 1
    long nsteps;
    size_t n;
    double fill, missing, thk_fill, thk_missing;
    TmFinish f;
};

// a carried array the caller did not give: allocated on the stream for a chain of launches, freed on it afterwards
struct StreamScratch {
    void *p = nullptr;
    hipStream_t s;
    explicit StreamScratch(hipStream_t stream) : s(stream) {}
    hipError_t get(size_t bytes) { return hipMallocAsync(&p, bytes, s); }
    ~StreamScratch()
    {
        if (p) (void)hipFreeAsync(p, s);
    }
    StreamScratch(const StreamScratch &) = delete;
    StreamScratch &operator=(const StreamScratch &) = delete;
};

template <typename T, int VEC, bool WEIGHTED>
int launch_time_mean_steps_v(const TimeMeanStepsArgs &a, hipStream_t s)
{
    const char *what = WEIGHTED ? "nf_time_mean_weighted_steps" : "nf_time_mean_steps";
    unsigned ntiles;
    NF_TRY(tm_tiles<VEC>(a.n, what, &ntiles));
    double *wsum = a.wsum;
    unsigned *cnt = a.cnt;
    StreamScratch tmp_cnt(s), tmp_wsum(s);
    if (a.nsteps > kTmTable) {      // a chain: something is carried between its launches
        if (!cnt) {
            NF_HIP(tmp_cnt.get(a.n * sizeof(unsigned)));
            cnt = (unsigned *)tmp_cnt.p;
        }
        if (!WEIGHTED && !wsum && a.f.rule == NF_MEAN_OVER_PRESENT) {
            NF_HIP(tmp_wsum.get(a.n * sizeof(double)));
            wsum = (double *)tmp_wsum.p;
        }
    }
    for (long t = 0; t < a.nsteps; t += kTmTable) {
        const int nb = a.nsteps - t < kTmTable ? (int)(a.nsteps - t) : kTmTable;
        TmFinish f = a.f;
        f.first = a.f.first && t == 0;
        f.last = a.f.last && t + nb == a.nsteps;
        if constexpr (WEIGHTED) {
            TmwsTable tab{};
            for (int j = 0; j < nb; ++j) {
                tab.off[j] = a.off[t + j];
                tab.thk_off[j] = a.thk_off[t + j];
                tab.w[j] = a.weights ? a.weights[t + j] : 1.0;
            }
            hipLaunchKernelGGL((k_time_mean_weighted_steps<T, VEC, kTimeMeanWeightedSteps>), dim3(xcd_grid(ntiles)), dim3(256),
                               0, s, a.acc, a.wsum, cnt, (const T *)a.src, (const T *)a.thk, tab, nb, a.n, ntiles, (T)a.fill,
                               (T)a.missing, (T)a.thk_fill, (T)a.thk_missing, f);
        } else {
            TmsTable tab{};
            for (int j = 0; j < nb; ++j) {
                tab.off[j] = a.off[t + j];
                tab.w[j] = a.weights ? a.weights[t + j] : 1.0;
            }
            hipLaunchKernelGGL((k_time_mean_steps<T, VEC, kTimeMeanSteps>), dim3(xcd_grid(ntiles)), dim3(256), 0, s, a.acc, wsum,
                               cnt, (const T *)a.src, tab, nb, a.n, ntiles, (T)a.fill, (T)a.missing, f);
        }
        NF_HIP(hipGetLastError());
    }
    return NF_OK;
}

template <typename T, int VEC, bool WEIGHTED>
int launch_time_mean_steps_t(const TimeMeanStepsArgs &a, hipStream_t s)
{
    // every listed step (of both series), acc, wsum and cnt 16-byte aligned at every lane's first value: else the whole
    // call, every launch of it, takes one value per lane
    bool al16 = lanes_aligned16({a.src, a.thk, a.acc, a.wsum, a.cnt});
    for (long j = 0; j < a.nsteps && al16; ++j) {
        al16 = a.off[j] * (long long)sizeof(T) % 16 == 0;
        if (WEIGHTED) al16 = al16 && a.thk_off[j] * (long long)sizeof(T) % 16 == 0;
    }
    return al16 ? launch_time_mean_steps_v<T, VEC, WEIGHTED>(a, s) : launch_time_mean_steps_v<T, 1, WEIGHTED>(a, s);
}

// the table as every call takes it: offsets >= 0, weights finite and > 0
int tm_check_table(const char *what, const long long *off, const double *weights, long nsteps)
{
    for (long j = 0; j < nsteps; ++j) {
        NF_REQUIRE(off[j] >= 0, NF_ERR_ARG, std::string(what) + ": a step offset is negative");
        NF_REQUIRE(!weights || (weights[j] > 0.0 && std::isfinite(weights[j])), NF_ERR_ARG,
                   std::string(what) + ": every weight must be finite and > 0");
    }
    return NF_OK;
}

}  // namespace

}  // namespace nf

using namespace nf;

extern "C" int nf_time_mean(double *acc_dev, unsigned *cnt_dev, const void *src_dev, long nsteps, long long stride_elems,
                            size_t n, int dtype, double fill, double missing, int first, int last, int rule, long total_steps,
                            double fill_out, void *hip_stream)
try {
    NF_REQUIRE(acc_dev && src_dev, NF_ERR_ARG, "nf_time_mean: null acc_dev or src_dev");
    NF_REQUIRE(nsteps >= 1, NF_ERR_ARG, "nf_time_mean: nsteps must be at least 1");
    NF_REQUIRE(n > 0, NF_ERR_ARG, "nf_time_mean: n must not be 0");
    NF_REQUIRE(nsteps == 1 || (stride_elems >= 0 && (unsigned long long)stride_elems >= n), NF_ERR_ARG,
               "nf_time_mean: stride_elems must be at least n when there is more than one step");
    NF_REQUIRE(dtype == NF_F64 || dtype == NF_F32, NF_ERR_ARG, "nf_time_mean: dtype must be NF_F64 or NF_F32");
    NF_REQUIRE(rule == NF_MEAN_OVER_STEPS || rule == NF_MEAN_OVER_PRESENT, NF_ERR_ARG,
               "nf_time_mean: rule must be NF_MEAN_OVER_STEPS or NF_MEAN_OVER_PRESENT");
    NF_REQUIRE(!(last && rule == NF_MEAN_OVER_STEPS) || total_steps >= 1, NF_ERR_ARG,
               "nf_time_mean: total_steps must be at least 1 for the last call of NF_MEAN_OVER_STEPS");
    NF_REQUIRE(cnt_dev || (first && last), NF_ERR_ARG,
               "nf_time_mean: cnt_dev may be null only when first && last (nothing is carried)");
    NF_NEED_DEVICE();
    const TimeMeanArgs a{acc_dev, cnt_dev, src_dev, nsteps, stride_elems, n, fill, missing,
                         TmFinish{first ? 1 : 0, last ? 1 : 0, rule, (double)total_steps, fill_out}};
    hipStream_t s = (hipStream_t)hip_stream;
    return dtype == NF_F64 ? launch_time_mean_t<double, 2>(a, s) : launch_time_mean_t<float, 4>(a, s);
}
NF_API_CATCH

extern "C" int nf_time_mean_weighted(double *accf_dev, double *acch_dev, unsigned *cnt_dev, const void *src_dev,
                                     long long src_stride_elems, const void *thk_dev, long long thk_stride_elems, long nsteps,
                                     size_t n, int dtype, double fill, double missing, double thk_fill, double thk_missing,
                                     int first, int last, long total_steps, double fill_out, void *hip_stream)
try {
    NF_REQUIRE(accf_dev && acch_dev && src_dev && thk_dev, NF_ERR_ARG,
               "nf_time_mean_weighted: null accf_dev, acch_dev, src_dev or thk_dev");
    NF_REQUIRE(nsteps >= 1, NF_ERR_ARG, "nf_time_mean_weighted: nsteps must be at least 1");
    NF_REQUIRE(n > 0, NF_ERR_ARG, "nf_time_mean_weighted: n must not be 0");
    NF_REQUIRE(nsteps == 1 || (src_stride_elems >= 0 && (unsigned long long)src_stride_elems >= n), NF_ERR_ARG,
               "nf_time_mean_weighted: src_stride_elems must be at least n when there is more than one step");
    NF_REQUIRE(nsteps == 1 || (thk_stride_elems >= 0 && (unsigned long long)thk_stride_elems >= n), NF_ERR_ARG,
               "nf_time_mean_weighted: thk_stride_elems must be at least n when there is more than one step");
    NF_REQUIRE(dtype == NF_F64 || dtype == NF_F32, NF_ERR_ARG, "nf_time_mean_weighted: dtype must be NF_F64 or NF_F32");
    NF_REQUIRE(!last || total_steps >= 1, NF_ERR_ARG, "nf_time_mean_weighted: total_steps must be at least 1 for the last call");
    NF_REQUIRE(cnt_dev || (first && last), NF_ERR_ARG,
               "nf_time_mean_weighted: cnt_dev may be null only when first && last (nothing is carried)");
    NF_NEED_DEVICE();
    const TimeMeanWeightedArgs a{accf_dev, acch_dev, cnt_dev, src_dev, thk_dev, src_stride_elems, thk_stride_elems, nsteps, n,
                                 fill, missing, thk_fill, thk_missing,
                                 TmFinish{first ? 1 : 0, last ? 1 : 0, NF_MEAN_OVER_STEPS, (double)total_steps, fill_out}};
    hipStream_t s = (hipStream_t)hip_stream;
    return dtype == NF_F64 ? launch_time_mean_weighted_t<double, 2>(a, s) : launch_time_mean_weighted_t<float, 4>(a, s);
}
NF_API_CATCH

extern "C" int nf_time_mean_steps(double *acc_dev, double *wsum_dev, unsigned *cnt_dev, const void *src_dev,
                                  const long long *step_offsets, const double *weights, long nsteps, size_t n, int dtype,
                                  double fill, double missing, int first, int last, int rule, double total_weight,
                                  double fill_out, void *hip_stream)
try {
    NF_REQUIRE(acc_dev && src_dev && step_offsets, NF_ERR_ARG, "nf_time_mean_steps: null acc_dev, src_dev or step_offsets");
    NF_REQUIRE(nsteps >= 1, NF_ERR_ARG, "nf_time_mean_steps: nsteps must be at least 1");
    NF_REQUIRE(n > 0, NF_ERR_ARG, "nf_time_mean_steps: n must not be 0");
    NF_REQUIRE(dtype == NF_F64 || dtype == NF_F32, NF_ERR_ARG, "nf_time_mean_steps: dtype must be NF_F64 or NF_F32");
    NF_REQUIRE(rule == NF_MEAN_OVER_STEPS || rule == NF_MEAN_OVER_PRESENT, NF_ERR_ARG,
               "nf_time_mean_steps: rule must be NF_MEAN_OVER_STEPS or NF_MEAN_OVER_PRESENT");
    NF_TRY(tm_check_table("nf_time_mean_steps", step_offsets, weights, nsteps));
    NF_REQUIRE(!(last && rule == NF_MEAN_OVER_STEPS) || (total_weight > 0.0 && std::isfinite(total_weight)), NF_ERR_ARG,
               "nf_time_mean_steps: total_weight must be finite and > 0 for the last call of NF_MEAN_OVER_STEPS");
    NF_REQUIRE(cnt_dev || (first && last), NF_ERR_ARG,
               "nf_time_mean_steps: cnt_dev may be null only when first && last (nothing is carried)");
    NF_REQUIRE(wsum_dev || (first && last) || rule == NF_MEAN_OVER_STEPS, NF_ERR_ARG,
               "nf_time_mean_steps: wsum_dev may be null only when first && last or under NF_MEAN_OVER_STEPS");
    NF_NEED_DEVICE();
    TimeMeanStepsArgs a{};
    a.acc = acc_dev, a.wsum = wsum_dev, a.cnt = cnt_dev, a.src = src_dev, a.off = step_offsets, a.weights = weights;
    a.nsteps = nsteps, a.n = n, a.fill = fill, a.missing = missing;
    a.f = TmFinish{first ? 1 : 0, last ? 1 : 0, rule, total_weight, fill_out};
    hipStream_t s = (hipStream_t)hip_stream;
    return dtype == NF_F64 ? launch_time_mean_steps_t<double, 2, false>(a, s) : launch_time_mean_steps_t<float, 4, false>(a, s);
}
NF_API_CATCH

extern "C" int nf_time_mean_weighted_steps(double *accf_dev, double *acch_dev, unsigned *cnt_dev, const void *src_dev,
                                           const long long *src_offsets, const void *thk_dev, const long long *thk_offsets,
                                           const double *weights, long nsteps, size_t n, int dtype, double fill, double missing,
                                           double thk_fill, double thk_missing, int first, int last, double total_weight,
                                           double fill_out, void *hip_stream)
try {
    NF_REQUIRE(accf_dev && acch_dev && src_dev && thk_dev && src_offsets && thk_offsets, NF_ERR_ARG,
               "nf_time_mean_weighted_steps: null accf_dev, acch_dev, src_dev, thk_dev, src_offsets or thk_offsets");
    NF_REQUIRE(nsteps >= 1, NF_ERR_ARG, "nf_time_mean_weighted_steps: nsteps must be at least 1");
    NF_REQUIRE(n > 0, NF_ERR_ARG, "nf_time_mean_weighted_steps: n must not be 0");
    NF_REQUIRE(dtype == NF_F64 || dtype == NF_F32, NF_ERR_ARG, "nf_time_mean_weighted_steps: dtype must be NF_F64 or NF_F32");
    NF_TRY(tm_check_table("nf_time_mean_weighted_steps", src_offsets, weights, nsteps));
    NF_TRY(tm_check_table("nf_time_mean_weighted_steps", thk_offsets, nullptr, nsteps));
    NF_REQUIRE(!last || (total_weight > 0.0 && std::isfinite(total_weight)), NF_ERR_ARG,
               "nf_time_mean_weighted_steps: total_weight must be finite and > 0 for the last call");
    NF_REQUIRE(cnt_dev || (first && last), NF_ERR_ARG,
               "nf_time_mean_weighted_steps: cnt_dev may be null only when first && last (nothing is carried)");
    NF_NEED_DEVICE();
    TimeMeanStepsArgs a{};
    a.acc = accf_dev, a.wsum = acch_dev, a.cnt = cnt_dev, a.src = src_dev, a.thk = thk_dev;
    a.off = src_offsets, a.thk_off = thk_offsets, a.weights = weights;
    a.nsteps = nsteps, a.n = n, a.fill = fill, a.missing = missing, a.thk_fill = thk_fill, a.thk_missing = thk_missing;
    a.f = TmFinish{first ? 1 : 0, last ? 1 : 0, NF_MEAN_OVER_STEPS, total_weight, fill_out};
    hipStream_t s = (hipStream_t)hip_stream;
    return dtype == NF_F64 ? launch_time_mean_steps_t<double, 2, true>(a, s) : launch_time_mean_steps_t<float, 4, true>(a, s);
}
NF_API_CATCH
