// nf_facethick.hip -- layer thicknesses at the U and V faces from the thickness at T-points (nf_face_thickness,
// nemoflux_amd.thickness): one streaming pass, e3t (and with the anomaly rule the three static thicknesses) in, e3u and e3v
// out, the arithmetic in float64.  The definition is in include/nemoflux_amd.h; tests/face_thickness_reference.py states it
// in numpy and reproduces the bits.
//
// Access pattern.  A tile is G consecutive rows j0 .. j0 + G - 1 of one level times one chunk of 256 * VEC values along x; a
// lane owns 16 consecutive bytes (2 doubles or 4 floats) of each of the rows.  It loads its 16 bytes of the G rows and of row
// j0 + G -- the north neighbour of the tile's last row, so the second read of a row happens once per G rows and not once per
// row -- and, per row, the one value east of its last one (the first value of the next lane's 16 bytes, or column 0 at the
// seam): a 4- or 8-byte load that falls into the line the next lane has just asked for.  All loads of a lane are issued
// before the first operation; the results leave in 2 G non-temporal 16-byte stores.  e3t and e3t0 are read with plain loads
// (the row j0 + G is the first row of the next tile), e3u0 and e3v0, read once, with non-temporal ones.  The tiles are dealt
// in K1's XCD bands with the chunk fastest and the row group next, so the tile that reads row j0 + G again runs on the same
// XCD shortly after: the second read is likely to hit in L2.  When a base or a row start is not 16-byte aligned (nx = 73, a
// pointer moved by one element) the same code runs with one value per lane: the same bits.  All offsets are 64-bit.
// Algorithmic bytes: 3 * n * sizeof(T) for MIN and MEAN, 6 * n * sizeof(T) for ANOMALY.
// One template over dtype and rule: MIN and MEAN hold no pointer to a static array and pay for none of their loads.
//
// Launch shape, decided with -Rpass-analysis=kernel-resource-usage (no instantiation uses scratch memory): block 256 (4 waves,
// as every streaming kernel here); G = 4 rows for MIN / MEAN (NF_FACETHICK_ROWS), G = 2 for ANOMALY (NF_FACETHICK_ROWS_ANOM),
// which holds four arrays' values per row.  VGPRs at float64 / float32: MIN 42 / 38, MEAN 38 / 40, ANOMALY 62 / 62 (one value
// per lane: 26 / 18, 26 / 18, 38 / 28); 8 waves per SIMD everywhere.  Measured at one step of the bench shape, 3600 x 1800 x
// 75, beside nf_sigma_eos80 at pref = 0 on arrays of the same size in the same process (profiles/face_thickness_timing.txt):
//   MIN 1.94 ms at float64 = 0.75 of the 8 TB/s peak beside 0.85, ratio 0.89 (MEAN 1.94 ms, 0.89): the aim of 0.9 is missed by
//   0.01 -- the kernel moves 3.25 n values, not 3 n, when the second read of row j0 + G misses, and issues one more load per
//   row for the east value; float32 1.03 ms = 0.71 beside 0.64, ratio 1.10.  ANOMALY 3.79 ms, 0.77, ratio 0.91 (float32
//   2.10 ms, 0.70, 1.09).  G = 2 and G = 8 for MIN / MEAN, each in a process of its own, gave 2.07 and 2.06 ms at float64
//   (float32 0.97 and 1.10) while nf_sigma_eos80 itself moved between 0.77 and 0.85 (0.63 and 0.64) of the peak from process
//   to process: no difference beyond that spread at float64, a hint that fewer rows serve float32; G = 4 is kept.
#include "nf_capi.h"
#include "nf_lanes.h"

#ifndef NF_FACETHICK_ROWS
#define NF_FACETHICK_ROWS 4
#endif
#ifndef NF_FACETHICK_ROWS_ANOM
#define NF_FACETHICK_ROWS_ANOM 2
#endif

namespace nf {

namespace {

template <typename T> struct FaceIn {
    const T *e3t, *e3t0, *e3u0, *e3v0;
    T m1, m2;       // the markers of e3t
    T s1, s2;       // the markers of the statics
    int wrap;
};

// one face: a, b the thicknesses of the two cells (b = a, b0 = a0 where there is no neighbour by geometry), f0 the static
// thickness of the face itself
template <typename T, int RULE>
__device__ inline T face_value(T a, T b, T a0, T b0, T f0, const FaceIn<T> &in)
{
    const bool both = tr_present<T>(a, in.m1, in.m2) && tr_present<T>(b, in.m1, in.m2);
    const double A = (double)a, B = (double)b;
    if (RULE == NF_E3_MIN) return both ? (T)(B < A ? B : A) : (T)0.0;
    if (RULE == NF_E3_MEAN) return both ? (T)(0.5 * (A + B)) : (T)0.0;
    if (!tr_present<T>(f0, in.s1, in.s2)) return (T)0.0;
    const bool all = both && tr_present<T>(a0, in.s1, in.s2) && tr_present<T>(b0, in.s1, in.s2);
    const double d = 0.5 * ((A - (double)a0) + (B - (double)b0));
    return all ? (T)((double)f0 + d) : f0;
}

}  // namespace

// 256 threads; a tile is G rows x 256 * VEC columns of one level.  tile -> (chunk fastest, then the row group, then the level).
// In the VEC > 1 form nx is a multiple of VEC, so a lane holds VEC values of a row or none.
template <typename T, int VEC, int G, int RULE>
__global__ __launch_bounds__(256) void k_face_thickness(T *e3u, T *e3v, FaceIn<T> in, long ny, long nx, unsigned nchunks,
                                                        unsigned ngroups, unsigned ntiles)
{
    constexpr bool ANOM = RULE == NF_E3_ANOMALY;
    const unsigned tile = xcd_tile(blockIdx.x, gridDim.x);
    if (tile >= ntiles) return;
    const unsigned c = tile % nchunks, rg = tile / nchunks;
    const long z = rg / ngroups, j0 = (long)(rg % ngroups) * G;
    const long x0 = (long)c * 256 * VEC + (long)threadIdx.x * VEC;
    if (x0 >= nx) return;
    const bool east_in = x0 + VEC < nx;
    const long xe = east_in ? x0 + VEC : 0;
    const bool has_e = east_in || in.wrap != 0;
    const size_t lev = (size_t)z * (size_t)ny * (size_t)nx;

    Lanes<T, VEC> a[G + 1], a0[G + 1], fu[G], fv[G];
    T ae[G], ae0[G];
#pragma unroll
    for (int g = 0; g <= G; ++g) {
        const long j = j0 + g;
#pragma unroll
        for (int k = 0; k < VEC; ++k) a[g].x[k] = a0[g].x[k] = (T)0;
        if (j >= ny) continue;
        const size_t row = lev + (size_t)j * (size_t)nx;
        a[g] = lane_load<T, VEC, false>(in.e3t + row + x0);
        if (ANOM) a0[g] = lane_load<T, VEC, false>(in.e3t0 + row + x0);
        if (g < G) {
            ae[g] = in.e3t[row + xe];
            if (ANOM) {
                ae0[g] = in.e3t0[row + xe];
                fu[g] = lane_load<T, VEC, true>(in.e3u0 + row + x0);
                fv[g] = lane_load<T, VEC, true>(in.e3v0 + row + x0);
            }
        }
    }
#pragma unroll
    for (int g = 0; g < G; ++g) {
        const long j = j0 + g;
        if (j >= ny) continue;
        const bool has_n = j + 1 < ny;
        Lanes<T, VEC> ru, rv;
#pragma unroll
        for (int k = 0; k < VEC; ++k) {
            const T A = a[g].x[k], A0 = ANOM ? a0[g].x[k] : (T)0;
            const bool he = k + 1 < VEC || has_e;
            const T Be = k + 1 < VEC ? a[g].x[k + 1 < VEC ? k + 1 : k] : ae[g];
            const T Be0 = ANOM ? (k + 1 < VEC ? a0[g].x[k + 1 < VEC ? k + 1 : k] : ae0[g]) : (T)0;
            ru.x[k] = face_value<T, RULE>(A, he ? Be : A, A0, he ? Be0 : A0, ANOM ? fu[g].x[k] : (T)0, in);
            rv.x[k] = face_value<T, RULE>(A, has_n ? a[g + 1].x[k] : A, A0, has_n ? a0[g + 1].x[k] : A0,
                                          ANOM ? fv[g].x[k] : (T)0, in);
        }
        const size_t at = lev + (size_t)j * (size_t)nx + (size_t)x0;
        lane_store<T, VEC>(e3u + at, ru);
        lane_store<T, VEC>(e3v + at, rv);
    }
}

namespace {

struct FaceArgs {
    void *e3u, *e3v;
    const void *e3t, *e3t0, *e3u0, *e3v0;
    long nz, ny, nx;
    int wrap;
    double fill, missing, fill0, missing0;
};

template <typename T, int VEC, int G, int RULE>
int launch_face_v(const FaceArgs &a, hipStream_t s)
{
    const size_t per_chunk = 256u * VEC;
    const size_t nchunks = ((size_t)a.nx + per_chunk - 1) / per_chunk, ngroups = ((size_t)a.ny + G - 1) / G;
    NF_REQUIRE(nchunks <= 0x7ffffff0u && ngroups <= 0x7ffffff0u && nchunks * ngroups <= 0x7ffffff0u / (size_t)a.nz, NF_ERR_ARG,
               "nf_face_thickness: the grid is too large for one launch");
    const size_t tiles = nchunks * ngroups * (size_t)a.nz;
    const FaceIn<T> in{(const T *)a.e3t, (const T *)a.e3t0, (const T *)a.e3u0, (const T *)a.e3v0, (T)a.fill, (T)a.missing,
                       (T)a.fill0, (T)a.missing0, a.wrap};
    hipLaunchKernelGGL((k_face_thickness<T, VEC, G, RULE>), dim3(xcd_grid((unsigned)tiles)), dim3(256), 0, s, (T *)a.e3u,
                       (T *)a.e3v, in, a.ny, a.nx, (unsigned)nchunks, (unsigned)ngroups, (unsigned)tiles);
    NF_HIP(hipGetLastError());
    return NF_OK;
}

template <typename T, int VEC, int RULE>
int launch_face_r(const FaceArgs &a, hipStream_t s)
{
    constexpr int G = RULE == NF_E3_ANOMALY ? NF_FACETHICK_ROWS_ANOM : NF_FACETHICK_ROWS;
    // every base and every row start 16-byte aligned: else one value per lane
    const bool al16 = lanes_aligned16({a.e3u, a.e3v, a.e3t, a.e3t0, a.e3u0, a.e3v0}) && a.nx % VEC == 0;
    return al16 ? launch_face_v<T, VEC, G, RULE>(a, s) : launch_face_v<T, 1, G, RULE>(a, s);
}

template <typename T, int VEC>
int launch_face_t(const FaceArgs &a, int rule, hipStream_t s)
{
    if (rule == NF_E3_MIN) return launch_face_r<T, VEC, NF_E3_MIN>(a, s);
    if (rule == NF_E3_MEAN) return launch_face_r<T, VEC, NF_E3_MEAN>(a, s);
    return launch_face_r<T, VEC, NF_E3_ANOMALY>(a, s);
}

// [p, p + bytes) and [q, q + bytes) share a byte; a null q is an array that is not there
inline bool ranges_meet(const void *p, const void *q, size_t bytes)
{
    if (!q) return false;
    const uintptr_t a = (uintptr_t)p, b = (uintptr_t)q;
    return (a < b ? b - a : a - b) < bytes;
}

}  // namespace

}  // namespace nf

using namespace nf;

extern "C" int nf_face_thickness(void *e3u_out_dev, void *e3v_out_dev, const void *e3t_dev, const void *e3t0_dev,
                                 const void *e3u0_dev, const void *e3v0_dev, long nz, long ny, long nx, int dtype, int rule,
                                 int wrap_x, double fill, double missing, double fill0, double missing0, void *hip_stream)
try {
    NF_REQUIRE(e3u_out_dev && e3v_out_dev && e3t_dev, NF_ERR_ARG, "nf_face_thickness: null e3u_out_dev, e3v_out_dev or e3t_dev");
    NF_REQUIRE(dtype == NF_F64 || dtype == NF_F32, NF_ERR_ARG, "nf_face_thickness: dtype must be NF_F64 or NF_F32");
    NF_REQUIRE(rule == NF_E3_MIN || rule == NF_E3_MEAN || rule == NF_E3_ANOMALY, NF_ERR_ARG,
               "nf_face_thickness: rule must be NF_E3_MIN, NF_E3_MEAN or NF_E3_ANOMALY");
    NF_REQUIRE(nz >= 1 && ny >= 1 && nx >= 1, NF_ERR_ARG, "nf_face_thickness: nz, ny and nx must be >= 1");
    if (rule == NF_E3_ANOMALY)
        NF_REQUIRE(e3t0_dev && e3u0_dev && e3v0_dev, NF_ERR_ARG,
                   "nf_face_thickness: the anomaly rule needs e3t0_dev, e3u0_dev and e3v0_dev");
    else
        NF_REQUIRE(!e3t0_dev && !e3u0_dev && !e3v0_dev, NF_ERR_ARG,
                   "nf_face_thickness: e3t0_dev, e3u0_dev and e3v0_dev go with the anomaly rule only");
    const size_t size = dtype == NF_F64 ? sizeof(double) : sizeof(float);
    const size_t lim = std::numeric_limits<size_t>::max() / size;
    NF_REQUIRE((size_t)ny <= lim / (size_t)nz && (size_t)nx <= lim / ((size_t)nz * (size_t)ny), NF_ERR_ARG,
               "nf_face_thickness: nz * ny * nx is too large");
    const size_t bytes = (size_t)nz * (size_t)ny * (size_t)nx * size;
    bool meet = ranges_meet(e3u_out_dev, e3v_out_dev, bytes);
    for (const void *out : {(const void *)e3u_out_dev, (const void *)e3v_out_dev})
        for (const void *q : {e3t_dev, e3t0_dev, e3u0_dev, e3v0_dev}) meet = meet || ranges_meet(out, q, bytes);
    NF_REQUIRE(!meet, NF_ERR_ARG, "nf_face_thickness: an output overlaps an input or the other output");
    NF_NEED_DEVICE();
    const FaceArgs a{e3u_out_dev, e3v_out_dev, e3t_dev, e3t0_dev, e3u0_dev, e3v0_dev, nz,    ny,
                     nx,          wrap_x != 0, fill,    missing,  fill0,    missing0};
    hipStream_t s = (hipStream_t)hip_stream;
    return dtype == NF_F64 ? launch_face_t<double, 2>(a, rule, s) : launch_face_t<float, 4>(a, rule, s);
}
NF_API_CATCH
