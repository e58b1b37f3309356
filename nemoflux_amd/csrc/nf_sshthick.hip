// nf_sshthick.hip -- z* layer thicknesses at the U and V faces from the sea surface height (nf_ssh_thickness, nf_column_depth,
// nemoflux_amd.thickness): e3u(t) = e3u_0 * (1 + ssh_u(t) / hu_0), one streaming pass, the two static face thicknesses in, e3u
// and e3v out, one (ny, nx) plane of ssh per step instead of a volume, the arithmetic in float64.  The definition is in
// include/nemoflux_amd.h; tests/ssh_thickness_reference.py states it in numpy and reproduces the bits.
//
// Access pattern (that of nf_facethick.hip).  A tile is one row j times one chunk of 256 * VEC values along x times a group of
// L consecutive levels; a lane owns 16 consecutive bytes (2 doubles or 4 floats) of the row in each level.  The lane forms its
// factors f_u and f_v once per tile: it loads its 16 bytes of ssh in row j and in row j + 1, the one value east of its last one
// (the first value of the next lane's 16 bytes, or column 0 at the seam), its values of the two column depths and, in the form
// with areas, of the three areas with the east and north neighbours of area_t -- plain loads, the planes are read again by the
// other level groups of the column and stay in L2 -- and divides twice per value.  Then it streams the group: the 2 L
// non-temporal 16-byte loads of e3u0 and e3v0 (read once) are all issued before the first multiply, the results leave in 2 L
// non-temporal 16-byte stores.  No row of a volume is read twice.  The tiles are dealt in K1's XCD bands with the chunk fastest,
// the level group next and the row last, so the level groups that read one row of the planes run on one XCD close together.
// The last group of a column may be short (nz = 75 with L = 8: 3 levels; nz = 1).  When a base or a row start is not 16-byte
// aligned (nx = 73, a pointer moved by one element) the same code runs with one value per lane: the same bits.  All offsets
// are 64-bit.  Algorithmic bytes: 4 * n * sizeof(T), plus the planes.
// One template over dtype, VEC and areas yes / no: the form without areas holds no area pointer and pays for none of their loads.
//
// Launch shape, decided with -Rpass-analysis=kernel-resource-usage (no instantiation uses scratch memory): block 256 (4 waves,
// as every streaming kernel here); L = 8 levels per group (NF_SSHTHICK_LEVELS).  VGPRs: 76 at float64 and 86 at float32, the
// same with areas as without, which is 6 and 5 waves per SIMD; the one-value-per-lane forms take 52 (float64) and 26 (float32)
// without areas, 42 and 30 with, 8 waves per SIMD.
// Measured at one step of the bench shape, 3600 x 1800 x 75, beside nf_sigma_eos80 at pref = 0 on arrays of the same size in
// the same process (profiles/ssh_thickness_timing.txt), the fraction of the 8 TB/s peak taken over 4 n values:
//   float64 2.68 ms = 0.73 beside 0.84, ratio 0.87 (with areas 2.78 ms, 0.70, 0.84): the aim of 0.9 is missed by 0.03 (0.06);
//   the same build in a process of its own just before gave 2.54 ms = 0.76 beside 0.80, ratio 0.95 (with areas 2.64 ms, 0.92)
//   -- the yardstick moved between 0.79 and 0.84 from process to process, this kernel between 0.70 and 0.76.  float32 1.33 ms =
//   0.73 beside 0.63, ratio 1.16 (with areas 1.45 ms, 0.67, 1.06).  0 of 972 million values differ from the restatement.
//   L = 2, 4 and 8, and the group's loads asked for before or after the factors are formed, each in a process of its own one
//   after the other (in which every kernel with two outputs, nf_face_thickness too, ran a tenth slower than above while
//   nf_sigma_eos80 stayed at 0.79 / 0.64: the builds compare with each other only), float64 / float32 ms without areas, then
//   with: L = 2 3.19 / 1.49, 3.45 / 2.05; L = 4 3.12 / 1.42, 3.25 / 1.64 (loads first: 3.13 / 1.42, 3.22 / 1.56); L = 8
//   3.10 / 1.39, 3.18 / 1.45 (loads first: 3.10 / 1.39, 3.17 / 1.42).  Longer groups spread the planes' loads and the two
//   divisions over more levels, which shows with areas and at float32; the place of the loads makes no difference beyond 2 %
//   at L = 8 and costs 20 to 54 VGPRs (96 to 140, 3 to 5 waves), so the loads follow the factors; L = 8 is kept.
//
// k_column_depth: the sum of a static thickness down each column, once per setting, one lane per 16 bytes of a row, the levels
// in ascending order in a register.  Not a hot path.
#include "nf_capi.h"
#include "nf_lanes.h"

#ifndef NF_SSHTHICK_LEVELS
#define NF_SSHTHICK_LEVELS 8
#endif

namespace nf {

namespace {

template <typename T, bool AREAS> struct SshIn;
template <typename T> struct SshIn<T, false> {
    const T *ssh, *e3u0, *e3v0;
    const double *hu0, *hv0;
    T m1, m2;       // the markers of ssh
    T s1, s2;       // the markers of the statics
    int wrap;
};
template <typename T> struct SshIn<T, true> : SshIn<T, false> {
    const double *at, *au, *av;
};

// VEC consecutive doubles of a plane at p: 16-byte loads where the lane form is the aligned one (VEC > 1)
template <int VEC>
__device__ inline Lanes<double, VEC> plane_load(const double *p)
{
    Lanes<double, VEC> r;
    if constexpr (VEC == 1) {
        r.x[0] = p[0];
    } else {
#pragma unroll
        for (int k = 0; k < VEC; k += 2) {
            const Lanes<double, 2> two = lane_load<double, 2, false>(p + k);
            r.x[k] = two.x[0];
            r.x[k + 1 < VEC ? k + 1 : k] = two.x[1];
        }
    }
    return r;
}

// the factor 1 + s / H of one face: sa, sb the sea surface heights of the two cells (sb = sa, tb = ta where there is no
// neighbour by geometry), ta, tb, f their areas and the face's, h the column depth at the face
template <typename T, bool AREAS>
__device__ inline double face_factor(T sa, T sb, double ta, double tb, double f, double h, T m1, T m2)
{
    const bool both = tr_present<T>(sa, m1, m2) && tr_present<T>(sb, m1, m2);
    double s;
    if (AREAS) {
        const double p = ta * (double)sa, q = tb * (double)sb;
        const bool ok = both && ta == ta && tb == tb && f > 0.0;      // a NaN f is not > 0
        s = ok ? (0.5 * (p + q)) / f : 0.0;
    } else {
        s = both ? 0.5 * ((double)sa + (double)sb) : 0.0;
    }
    const double r = h > 0.0 ? s / h : 0.0;       // a NaN h is not > 0
    return 1.0 + r;
}

}  // namespace

// 256 threads; a tile is one row x 256 * VEC columns x L levels.  tile -> (chunk fastest, then the level group, then the row).
// In the VEC > 1 form nx is a multiple of VEC, so a lane holds VEC values of a row or none.
template <typename T, int VEC, int L, bool AREAS>
__global__ __launch_bounds__(256) void k_ssh_thickness(T *e3u, T *e3v, SshIn<T, AREAS> in, long nz, long ny, long nx,
                                                       unsigned nchunks, unsigned ngroups, unsigned ntiles)
{
    const unsigned tile = xcd_tile(blockIdx.x, gridDim.x);
    if (tile >= ntiles) return;
    const unsigned c = tile % nchunks, rg = tile / nchunks;
    const long z0 = (long)(rg % ngroups) * L, j = rg / ngroups;
    const long x0 = (long)c * 256 * VEC + (long)threadIdx.x * VEC;
    if (x0 >= nx) return;
    const bool east_in = x0 + VEC < nx;
    const long xe = east_in ? x0 + VEC : 0;
    const bool has_e = east_in || in.wrap != 0, has_n = j + 1 < ny;
    const size_t row = (size_t)j * (size_t)nx, plane = (size_t)ny * (size_t)nx;
    const size_t north = has_n ? row + (size_t)nx : row;

    // the two factors of every value of the lane
    double fu[VEC], fv[VEC];
    {
        const Lanes<T, VEC> s = lane_load<T, VEC, false>(in.ssh + row + x0);
        const Lanes<T, VEC> sn = lane_load<T, VEC, false>(in.ssh + north + x0);
        const T se = in.ssh[row + xe];
        const Lanes<double, VEC> hu = plane_load<VEC>(in.hu0 + row + x0), hv = plane_load<VEC>(in.hv0 + row + x0);
        Lanes<double, VEC> t, tn, au, av;
        double te = 0.0;
        if constexpr (AREAS) {
            t = plane_load<VEC>(in.at + row + x0);
            tn = plane_load<VEC>(in.at + north + x0);
            te = in.at[row + xe];
            au = plane_load<VEC>(in.au + row + x0);
            av = plane_load<VEC>(in.av + row + x0);
        }
#pragma unroll
        for (int k = 0; k < VEC; ++k) {
            const bool he = k + 1 < VEC || has_e;
            const T sa = s.x[k];
            const T sb = k + 1 < VEC ? s.x[k + 1 < VEC ? k + 1 : k] : se;
            double ta = 0.0, tb = 0.0, tbn = 0.0, Fu = 0.0, Fv = 0.0;
            if constexpr (AREAS) {
                ta = t.x[k];
                tb = k + 1 < VEC ? t.x[k + 1 < VEC ? k + 1 : k] : te;
                tbn = tn.x[k];
                Fu = au.x[k];
                Fv = av.x[k];
            }
            fu[k] = face_factor<T, AREAS>(sa, he ? sb : sa, ta, he ? tb : ta, Fu, hu.x[k], in.m1, in.m2);
            fv[k] = face_factor<T, AREAS>(sa, has_n ? sn.x[k] : sa, ta, has_n ? tbn : ta, Fv, hv.x[k], in.m1, in.m2);
        }
    }

    // the group's levels: every load before the first multiply, then one multiply per value and 2 L stores
    const size_t at0 = (size_t)z0 * plane + row + (size_t)x0;
    Lanes<T, VEC> u0[L], v0[L];
#pragma unroll
    for (int g = 0; g < L; ++g) {
        if (z0 + g >= nz) continue;
        u0[g] = lane_load<T, VEC, true>(in.e3u0 + at0 + (size_t)g * plane);
        v0[g] = lane_load<T, VEC, true>(in.e3v0 + at0 + (size_t)g * plane);
    }
#pragma unroll
    for (int g = 0; g < L; ++g) {
        if (z0 + g >= nz) continue;
        Lanes<T, VEC> ru, rv;
#pragma unroll
        for (int k = 0; k < VEC; ++k) {
            const T a = u0[g].x[k], b = v0[g].x[k];
            ru.x[k] = tr_present<T>(a, in.s1, in.s2) ? (T)((double)a * fu[k]) : (T)0.0;
            rv.x[k] = tr_present<T>(b, in.s1, in.s2) ? (T)((double)b * fv[k]) : (T)0.0;
        }
        lane_store<T, VEC>(e3u + at0 + (size_t)g * plane, ru);
        lane_store<T, VEC>(e3v + at0 + (size_t)g * plane, rv);
    }
}

// 256 threads; a tile is one row x 256 * VEC columns; h[j, i] = the sum over the levels, in ascending order, of the present
// values of column (j, i)
template <typename T, int VEC>
__global__ __launch_bounds__(256) void k_column_depth(double *h, const T *e3, T m1, T m2, long nz, long ny, long nx,
                                                      unsigned nchunks)
{
    const long j = blockIdx.x / nchunks;
    const long x0 = (long)(blockIdx.x % nchunks) * 256 * VEC + (long)threadIdx.x * VEC;
    if (j >= ny || x0 >= nx) return;
    const size_t row = (size_t)j * (size_t)nx + (size_t)x0, plane = (size_t)ny * (size_t)nx;
    double sum[VEC];
#pragma unroll
    for (int k = 0; k < VEC; ++k) sum[k] = 0.0;
    for (long z = 0; z < nz; ++z) {
        const Lanes<T, VEC> a = lane_load<T, VEC, false>(e3 + (size_t)z * plane + row);
#pragma unroll
        for (int k = 0; k < VEC; ++k)
            if (tr_present<T>(a.x[k], m1, m2)) sum[k] = sum[k] + (double)a.x[k];
    }
#pragma unroll
    for (int k = 0; k < VEC; ++k) h[row + k] = sum[k];
}

namespace {

struct SshArgs {
    void *e3u, *e3v;
    const void *ssh, *e3u0, *e3v0;
    const double *hu0, *hv0, *at, *au, *av;
    long nz, ny, nx;
    int wrap;
    double fill, missing, fill0, missing0;
};

template <typename T, int VEC, bool AREAS>
int launch_ssh_v(const SshArgs &a, hipStream_t s)
{
    constexpr int L = NF_SSHTHICK_LEVELS;
    const size_t per_chunk = 256u * VEC;
    const size_t nchunks = ((size_t)a.nx + per_chunk - 1) / per_chunk, ngroups = ((size_t)a.nz + L - 1) / L;
    NF_REQUIRE(nchunks <= 0x7ffffff0u && ngroups <= 0x7ffffff0u && nchunks * ngroups <= 0x7ffffff0u / (size_t)a.ny, NF_ERR_ARG,
               "nf_ssh_thickness: the grid is too large for one launch");
    const size_t tiles = nchunks * ngroups * (size_t)a.ny;
    SshIn<T, AREAS> in;
    in.ssh = (const T *)a.ssh, in.e3u0 = (const T *)a.e3u0, in.e3v0 = (const T *)a.e3v0;
    in.hu0 = a.hu0, in.hv0 = a.hv0;
    in.m1 = (T)a.fill, in.m2 = (T)a.missing, in.s1 = (T)a.fill0, in.s2 = (T)a.missing0;
    in.wrap = a.wrap;
    if constexpr (AREAS) in.at = a.at, in.au = a.au, in.av = a.av;
    hipLaunchKernelGGL((k_ssh_thickness<T, VEC, L, AREAS>), dim3(xcd_grid((unsigned)tiles)), dim3(256), 0, s, (T *)a.e3u,
                       (T *)a.e3v, in, a.nz, a.ny, a.nx, (unsigned)nchunks, (unsigned)ngroups, (unsigned)tiles);
    NF_HIP(hipGetLastError());
    return NF_OK;
}

template <typename T, int VEC>
int launch_ssh_t(const SshArgs &a, hipStream_t s)
{
    // every base and every row start 16-byte aligned: else one value per lane
    const bool al16 = lanes_aligned16({a.e3u, a.e3v, a.ssh, a.e3u0, a.e3v0, a.hu0, a.hv0, a.at, a.au, a.av}) && a.nx % VEC == 0;
    if (a.at) return al16 ? launch_ssh_v<T, VEC, true>(a, s) : launch_ssh_v<T, 1, true>(a, s);
    return al16 ? launch_ssh_v<T, VEC, false>(a, s) : launch_ssh_v<T, 1, false>(a, s);
}

template <typename T, int VEC>
int launch_depth_v(double *h, const void *e3, long nz, long ny, long nx, double fill0, double missing0, hipStream_t s)
{
    const size_t per_chunk = 256u * VEC;
    const size_t nchunks = ((size_t)nx + per_chunk - 1) / per_chunk;
    NF_REQUIRE(nchunks <= 0x7ffffff0u && nchunks <= 0x7ffffff0u / (size_t)ny, NF_ERR_ARG,
               "nf_column_depth: the grid is too large for one launch");
    hipLaunchKernelGGL((k_column_depth<T, VEC>), dim3((unsigned)(nchunks * (size_t)ny)), dim3(256), 0, s, h, (const T *)e3,
                       (T)fill0, (T)missing0, nz, ny, nx, (unsigned)nchunks);
    NF_HIP(hipGetLastError());
    return NF_OK;
}

template <typename T, int VEC>
int launch_depth_t(double *h, const void *e3, long nz, long ny, long nx, double fill0, double missing0, hipStream_t s)
{
    const bool al16 = lanes_aligned16({e3}) && nx % VEC == 0;
    return al16 ? launch_depth_v<T, VEC>(h, e3, nz, ny, nx, fill0, missing0, s)
                : launch_depth_v<T, 1>(h, e3, nz, ny, nx, fill0, missing0, s);
}

// [p, p + pbytes) and [q, q + qbytes) share a byte; a null q is an array that is not there
inline bool ranges_share(const void *p, size_t pbytes, const void *q, size_t qbytes)
{
    if (!q) return false;
    const uintptr_t a = (uintptr_t)p, b = (uintptr_t)q;
    return a < b ? b - a < pbytes : a - b < qbytes;
}

// nz * ny * nx * size fits a size_t
inline bool volume_fits(long nz, long ny, long nx, size_t size)
{
    const size_t lim = std::numeric_limits<size_t>::max() / size;
    return (size_t)ny <= lim / (size_t)nz && (size_t)nx <= lim / ((size_t)nz * (size_t)ny);
}

}  // namespace

}  // namespace nf

using namespace nf;

extern "C" int nf_column_depth(double *h_out_dev, const void *e3_0_dev, long nz, long ny, long nx, int dtype, double fill0,
                               double missing0, void *hip_stream)
try {
    NF_REQUIRE(h_out_dev && e3_0_dev, NF_ERR_ARG, "nf_column_depth: null h_out_dev or e3_0_dev");
    NF_REQUIRE(dtype == NF_F64 || dtype == NF_F32, NF_ERR_ARG, "nf_column_depth: dtype must be NF_F64 or NF_F32");
    NF_REQUIRE(nz >= 1 && ny >= 1 && nx >= 1, NF_ERR_ARG, "nf_column_depth: nz, ny and nx must be >= 1");
    const size_t size = dtype == NF_F64 ? sizeof(double) : sizeof(float);
    NF_REQUIRE(volume_fits(nz, ny, nx, sizeof(double)), NF_ERR_ARG, "nf_column_depth: nz * ny * nx is too large");
    const size_t pbytes = (size_t)ny * (size_t)nx * sizeof(double), bytes = (size_t)nz * (size_t)ny * (size_t)nx * size;
    NF_REQUIRE(!ranges_share(h_out_dev, pbytes, e3_0_dev, bytes), NF_ERR_ARG, "nf_column_depth: h_out_dev overlaps e3_0_dev");
    NF_NEED_DEVICE();
    hipStream_t s = (hipStream_t)hip_stream;
    return dtype == NF_F64 ? launch_depth_t<double, 2>(h_out_dev, e3_0_dev, nz, ny, nx, fill0, missing0, s)
                           : launch_depth_t<float, 4>(h_out_dev, e3_0_dev, nz, ny, nx, fill0, missing0, s);
}
NF_API_CATCH

extern "C" int nf_ssh_thickness(void *e3u_out_dev, void *e3v_out_dev, const void *ssh_dev, const void *e3u0_dev,
                                const void *e3v0_dev, const double *hu0_dev, const double *hv0_dev, const double *area_t_dev,
                                const double *area_u_dev, const double *area_v_dev, long nz, long ny, long nx, int dtype,
                                int wrap_x, double fill, double missing, double fill0, double missing0, void *hip_stream)
try {
    NF_REQUIRE(e3u_out_dev && e3v_out_dev && ssh_dev, NF_ERR_ARG, "nf_ssh_thickness: null e3u_out_dev, e3v_out_dev or ssh_dev");
    NF_REQUIRE(e3u0_dev && e3v0_dev && hu0_dev && hv0_dev, NF_ERR_ARG,
               "nf_ssh_thickness: null e3u0_dev, e3v0_dev, hu0_dev or hv0_dev");
    const int nareas = (area_t_dev != nullptr) + (area_u_dev != nullptr) + (area_v_dev != nullptr);
    NF_REQUIRE(nareas == 0 || nareas == 3, NF_ERR_ARG,
               "nf_ssh_thickness: area_t_dev, area_u_dev and area_v_dev go together: all three or all NULL");
    NF_REQUIRE(dtype == NF_F64 || dtype == NF_F32, NF_ERR_ARG, "nf_ssh_thickness: dtype must be NF_F64 or NF_F32");
    NF_REQUIRE(nz >= 1 && ny >= 1 && nx >= 1, NF_ERR_ARG, "nf_ssh_thickness: nz, ny and nx must be >= 1");
    const size_t size = dtype == NF_F64 ? sizeof(double) : sizeof(float);
    NF_REQUIRE(volume_fits(nz, ny, nx, sizeof(double)), NF_ERR_ARG, "nf_ssh_thickness: nz * ny * nx is too large");
    const size_t cells = (size_t)ny * (size_t)nx, bytes = (size_t)nz * cells * size;
    bool meet = ranges_share(e3u_out_dev, bytes, e3v_out_dev, bytes);
    for (const void *out : {(const void *)e3u_out_dev, (const void *)e3v_out_dev}) {
        for (const void *q : {e3u0_dev, e3v0_dev}) meet = meet || ranges_share(out, bytes, q, bytes);
        meet = meet || ranges_share(out, bytes, ssh_dev, cells * size);
        for (const double *q : {hu0_dev, hv0_dev, area_t_dev, area_u_dev, area_v_dev})
            meet = meet || ranges_share(out, bytes, q, cells * sizeof(double));
    }
    NF_REQUIRE(!meet, NF_ERR_ARG, "nf_ssh_thickness: an output overlaps an input or the other output");
    NF_NEED_DEVICE();
    const SshArgs a{e3u_out_dev, e3v_out_dev, ssh_dev, e3u0_dev, e3v0_dev, hu0_dev, hv0_dev, area_t_dev, area_u_dev, area_v_dev,
                    nz,          ny,          nx,      wrap_x != 0, fill,   missing, fill0,  missing0};
    hipStream_t s = (hipStream_t)hip_stream;
    return dtype == NF_F64 ? launch_ssh_t<double, 2>(a, s) : launch_ssh_t<float, 4>(a, s);
}
NF_API_CATCH
