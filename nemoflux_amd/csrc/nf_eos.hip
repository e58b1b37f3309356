// nf_eos.hip -- potential density from potential temperature and practical salinity (nf_sigma_eos80, nemoflux_amd.eos): one
// streaming pass, two arrays in, one array out, the arithmetic in float64.
//
// Definition, per value i (UNESCO EOS-80; theta in degC referenced to the surface, S practical salinity, pref in dbar):
//   sigma = pref == 0 ? rho0(S, theta) - 1000                                    the one-atmosphere equation: sigma0, exact
//                     : rho(S, ptmp(S, theta, 0, pref), pref) - 1000             sigma2, sigma4, ...
// rho0 is the Millero-Poisson one-atmosphere density, rho = rho0 / (1 - P / K) with the secant bulk modulus K (P in bar), ptmp
// the Fofonoff-Millard Runge-Kutta step over Bryden's adiabatic lapse rate atg.  Every polynomial is the Horner form written
// below, evaluated left to right in float64: no fused multiply-add (-ffp-contract=off), no reassociation, IEEE sqrt and
// division.  float32 inputs are widened first and the result is rounded once, at the store.  A numpy float64 loop that states
// the same expressions (tests/eos_reference.py) reproduces the bits.
// "Present" is the engine's rule (tr_present of nf_common.h): not NaN and equal to neither of the array's own two markers, each
// cast to the array's dtype and compared in that dtype.  Where theta or S is missing the output is fill_out.  A negative S gives
// NaN through sqrt, which every consumer reads as "no value".
// EOS-80 only: TEOS-10 (conservative temperature, absolute salinity) is not covered.
//
// Access pattern (k_time_mean's).  A lane owns 16 consecutive bytes of the value axis (2 doubles or 4 floats) of each of G
// groups; group g of a block's tile is the 256 * VEC values that begin at (tile * G + g) * 256 * VEC, so a wave's load is 1 KiB
// of consecutive bytes.  The 2 G non-temporal 16-byte loads of a lane are issued before the first operation; the results leave
// in G non-temporal 16-byte stores.  When theta, S or out is not 16-byte aligned the same code runs with one value per lane:
// the same bits.  All offsets are 64-bit.  out may be theta or S itself (a lane has read all its groups before it writes).
// Algorithmic bytes: 3 * n * sizeof(T).
//
// Launch shape, decided with -Rpass-analysis=kernel-resource-usage (no instantiation uses scratch memory) and measured at one
// step of the bench shape, 3600 x 1800 x 75 (profiles/eos_timing.txt):
//   block 256 (4 waves, as every streaming kernel here); one tile per block, the tiles dealt in K1's XCD bands.
//   Groups per lane, VGPRs at float64 / float32 and waves per SIMD: pref == 0  G = 1: 35 / 37, 8;  G = 2: 37 / 39, 8;
//   G = 4: 56 / 59, 8.  pref > 0  G = 1: 49 / 47, 7 (106 SGPRs: the coefficients);  G = 2: 49 / 51, 7;  G = 4: 69 / 71, 7.
//   pref == 0 is about 40 float64 vector instructions per value against 24 (12) bytes: bandwidth-bound, 1.84 ms at float64 =
//   0.79 of the 8 TB/s peak beside nf_time_mean's 0.77 on one of the arrays in the same process (float32 1.11 ms, 0.66 beside
//   0.59).  G = 1 and G = 4, each in a process of its own, gave 1.77 and 1.93 ms (float32 1.14 and 1.11), 1.02 and 0.96 (0.97
//   and 1.06) of nf_time_mean's fraction there, which itself moved between 0.77 and 0.81 (0.59 and 0.66): no difference beyond
//   the spread between processes, and G = 2 is kept (NF_EOS_GROUPS0).
//   pref > 0 is about 330 float64 vector instructions per value, division and sqrt expanded: compute-bound, 4.66 ms at float64
//   and 4.12 ms at float32, 2.5 x and 3.7 x the sigma0 form; the float64 time is 0.88 of the data sheet's float64 vector rate
//   (39.3e12 unfused operations per second: 4.1 ms for these instructions).  The compiler keeps the chains of a lane's values apart (the registers do
//   not grow from G = 1 to 2), so the dependent chain is hidden by the 7 waves of a SIMD; G = 1 and G = 4 gave 4.68 and 4.61 ms
//   (float32 4.20 and 4.17): no difference, and G = 2 is kept (NF_EOS_GROUPSP).
#include "nf_capi.h"
#include "nf_lanes.h"

#ifndef NF_EOS_GROUPS0
#define NF_EOS_GROUPS0 2
#endif
#ifndef NF_EOS_GROUPSP
#define NF_EOS_GROUPSP 2
#endif

namespace nf {

namespace {

// one-atmosphere density, r = sqrt(S)
__device__ inline double eos_rho0(double S, double T, double r)
{
    const double rw = 999.842594 + (6.793952e-2 + (-9.095290e-3 + (1.001685e-4 + (-1.120083e-6 + 6.536332e-9 * T) * T) * T) * T) * T;
    const double b = 8.24493e-1 + (-4.0899e-3 + (7.6438e-5 + (-8.2467e-7 + 5.3875e-9 * T) * T) * T) * T;
    const double c = -5.72466e-3 + (1.0227e-4 - 1.6546e-6 * T) * T;
    return rw + (b + c * r + 4.8314e-4 * S) * S;
}

// secant bulk modulus, P in bar
__device__ inline double eos_bulk(double S, double T, double P, double r)
{
    const double kw = 19652.21 + (148.4206 + (-2.327105 + (1.360477e-2 - 5.155288e-5 * T) * T) * T) * T;
    const double k0 = kw + (54.6746 + (-0.603459 + (1.09987e-2 - 6.1670e-5 * T) * T) * T) * S +
                      (7.944e-2 + (1.6483e-2 - 5.3009e-4 * T) * T) * S * r;
    const double aw = 3.239908 + (1.43713e-3 + (1.16092e-4 - 5.77905e-7 * T) * T) * T;
    const double a = aw + (2.2838e-3 + (-1.0981e-5 - 1.6078e-6 * T) * T) * S + 1.91075e-4 * S * r;
    const double bw = 8.50935e-5 + (-6.12293e-6 + 5.2787e-8 * T) * T;
    const double bb = bw + (-9.9348e-7 + (2.0816e-8 + 9.1697e-10 * T) * T) * S;
    return k0 + (a + bb * P) * P;
}

// adiabatic lapse rate in degC / dbar, p in dbar
__device__ inline double eos_atg(double S, double T, double p)
{
    const double ds = S - 35.0;
    return 3.5803e-5 + (8.5258e-6 + (-6.836e-8 + 6.6228e-10 * T) * T) * T + (1.8932e-6 - 4.2393e-8 * T) * ds +
           ((1.8741e-8 + (-6.7795e-10 + (8.733e-12 - 5.4481e-14 * T) * T) * T) + (-1.1351e-10 + 2.7759e-12 * T) * ds) * p +
           (-4.6206e-13 + (1.8676e-14 - 2.1687e-16 * T) * T) * p * p;
}

// T moved adiabatically from p to pr
__device__ inline double eos_ptmp(double S, double T, double p, double pr)
{
    const double h = pr - p;
    double xk = h * eos_atg(S, T, p);
    T += 0.5 * xk;
    double q = xk;
    p += 0.5 * h;
    xk = h * eos_atg(S, T, p);
    T += 0.29289322 * (xk - q);
    q = 0.58578644 * xk + 0.121320344 * q;
    xk = h * eos_atg(S, T, p);
    T += 1.707106781 * (xk - q);
    q = 3.414213562 * xk - 4.121320344 * q;
    p += 0.5 * h;
    xk = h * eos_atg(S, T, p);
    return T + (xk - 2.0 * q) / 6.0;
}

template <bool PRESS>
__device__ inline double eos_sigma(double theta, double S, double pref)
{
    const double r = sqrt(S);
    if (!PRESS) return eos_rho0(S, theta, r) - 1000.0;
    const double T = eos_ptmp(S, theta, 0.0, pref);
    const double P = pref / 10.0;
    return eos_rho0(S, T, r) / (1.0 - P / eos_bulk(S, T, P, r)) - 1000.0;
}

template <typename T> struct EosIn {
    const T *theta, *salt;
    T t1, t2, s1, s2;     // the markers of theta, of S
    T fill_out;
    double pref;
};

template <typename T, bool PRESS>
__device__ inline T eos_value(T th, T sa, const EosIn<T> &in)
{
    const bool here = tr_present<T>(th, in.t1, in.t2) && tr_present<T>(sa, in.s1, in.s2);
    const double sg = eos_sigma<PRESS>((double)th, (double)sa, in.pref);
    return here ? (T)sg : in.fill_out;
}

}  // namespace

// 256 threads, G groups of VEC values per lane, one tile of G * 256 * VEC values per block.  The tiles are dealt in K1's XCD
// bands; the grid is xcd_grid(ntiles), tiles >= ntiles exit.  The one lane that holds fewer than VEC values of a group (n is no
// multiple of VEC) takes them one at a time, after its whole groups.
template <typename T, int VEC, int G, bool PRESS>
__global__ __launch_bounds__(256) void k_sigma_eos80(T *out, EosIn<T> in, size_t n, unsigned ntiles)
{
    const unsigned tile = xcd_tile(blockIdx.x, gridDim.x);
    if (tile >= ntiles) return;
    const size_t base = (size_t)tile * G * 256 * VEC + (size_t)threadIdx.x * VEC;
    Lanes<T, VEC> th[G], sa[G];
    bool whole[G];
#pragma unroll
    for (int g = 0; g < G; ++g) {
        const size_t i0 = base + (size_t)g * 256 * VEC;
        whole[g] = i0 < n && n - i0 >= (size_t)VEC;
        if (whole[g]) {
            th[g] = lane_load<T, VEC, true>(in.theta + i0);
            sa[g] = lane_load<T, VEC, true>(in.salt + i0);
        }
    }
#pragma unroll
    for (int g = 0; g < G; ++g) {
        if (!whole[g]) continue;
        Lanes<T, VEC> r;
#pragma unroll
        for (int k = 0; k < VEC; ++k) r.x[k] = eos_value<T, PRESS>(th[g].x[k], sa[g].x[k], in);
        lane_store<T, VEC>(out + base + (size_t)g * 256 * VEC, r);
    }
    if (VEC > 1) {
#pragma unroll
        for (int g = 0; g < G; ++g) {
            const size_t i0 = base + (size_t)g * 256 * VEC;
            if (whole[g] || i0 >= n) continue;
            for (size_t i = i0; i < n; ++i) out[i] = eos_value<T, PRESS>(in.theta[i], in.salt[i], in);
        }
    }
}

namespace {

struct SigmaArgs {
    void *out;
    const void *theta, *salt;
    size_t n;
    double pref, theta_fill, theta_missing, salt_fill, salt_missing, fill_out;
};

template <typename T, int VEC, int G, bool PRESS>
int launch_sigma_v(const SigmaArgs &a, hipStream_t s)
{
    const size_t per_block = (size_t)G * 256u * VEC, tiles = (a.n + per_block - 1) / per_block;
    NF_REQUIRE(tiles <= 0x7ffffff0u, NF_ERR_ARG, "nf_sigma_eos80: n is too large for one launch");
    const EosIn<T> in{(const T *)a.theta, (const T *)a.salt, (T)a.theta_fill, (T)a.theta_missing, (T)a.salt_fill,
                      (T)a.salt_missing, (T)a.fill_out, a.pref};
    hipLaunchKernelGGL((k_sigma_eos80<T, VEC, G, PRESS>), dim3(xcd_grid((unsigned)tiles)), dim3(256), 0, s, (T *)a.out, in, a.n,
                       (unsigned)tiles);
    NF_HIP(hipGetLastError());
    return NF_OK;
}

template <typename T, int VEC>
int launch_sigma_t(const SigmaArgs &a, hipStream_t s)
{
    // theta, S and out 16-byte aligned at every lane's first value: else one value per lane
    const bool al16 = lanes_aligned16({a.theta, a.salt, a.out});
    if (a.pref == 0.0)
        return al16 ? launch_sigma_v<T, VEC, NF_EOS_GROUPS0, false>(a, s) : launch_sigma_v<T, 1, NF_EOS_GROUPS0, false>(a, s);
    return al16 ? launch_sigma_v<T, VEC, NF_EOS_GROUPSP, true>(a, s) : launch_sigma_v<T, 1, NF_EOS_GROUPSP, true>(a, s);
}

// [p, p + bytes) and [q, q + bytes) share a byte, and are not one and the same range
inline bool partly_overlap(const void *p, const void *q, size_t bytes)
{
    const uintptr_t a = (uintptr_t)p, b = (uintptr_t)q;
    return a != b && (a < b ? b - a : a - b) < bytes;
}

}  // namespace

}  // namespace nf

using namespace nf;

extern "C" int nf_sigma_eos80(void *out_dev, const void *theta_dev, const void *salt_dev, size_t n, int dtype, double pref_dbar,
                              double theta_fill, double theta_missing, double salt_fill, double salt_missing, double fill_out,
                              void *hip_stream)
try {
    NF_REQUIRE(dtype == NF_F64 || dtype == NF_F32, NF_ERR_ARG, "nf_sigma_eos80: dtype must be NF_F64 or NF_F32");
    NF_REQUIRE(pref_dbar >= 0.0 && pref_dbar <= std::numeric_limits<double>::max(), NF_ERR_ARG,
               "nf_sigma_eos80: pref_dbar must be finite and not negative");
    if (n == 0) return NF_OK;
    NF_REQUIRE(out_dev && theta_dev && salt_dev, NF_ERR_ARG, "nf_sigma_eos80: null out_dev, theta_dev or salt_dev");
    const size_t size = dtype == NF_F64 ? sizeof(double) : sizeof(float);
    NF_REQUIRE(n <= std::numeric_limits<size_t>::max() / size, NF_ERR_ARG, "nf_sigma_eos80: n is too large");
    NF_REQUIRE(!partly_overlap(out_dev, theta_dev, n * size) && !partly_overlap(out_dev, salt_dev, n * size), NF_ERR_ARG,
               "nf_sigma_eos80: out_dev overlaps theta_dev or salt_dev without being equal to it");
    NF_NEED_DEVICE();
    const SigmaArgs a{out_dev, theta_dev, salt_dev, n, pref_dbar, theta_fill, theta_missing, salt_fill, salt_missing, fill_out};
    hipStream_t s = (hipStream_t)hip_stream;
    return dtype == NF_F64 ? launch_sigma_t<double, 2>(a, s) : launch_sigma_t<float, 4>(a, s);
}
NF_API_CATCH
