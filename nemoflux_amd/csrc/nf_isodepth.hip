// nf_isodepth.hip -- the depth at which a tracer first reaches a value, column by column (nf_iso_depth,
// nemoflux_amd.surfaces): the depth of an isotherm or an isopycnal, the mixed-layer depth by a threshold criterion.  One pass
// down the columns of one time step, m values at once, m planes out.  The definition is the header's (include/nemoflux_amd.h);
// all arithmetic is float64, every operation rounded on its own (-ffp-contract=off), float32 inputs widened first, the result
// rounded once at the store.  tests/iso_depth_reference.py states the same in numpy and reproduces the bits.
//
// Access pattern.  One lane per column; column i = y * nx + x, so the lanes of a wave run along x and the load of a level is
// 64 consecutive values (512 B at float64, 256 B at float32).  The level loop walks groups of 4 (float64) or 8 (float32) levels: the loads
// of the group (tracer, and thickness in the e3t form) are issued first, then the levels are taken in order.  The state of a
// lane -- interface depth, the level above (centre, value), the thresholds, one result and one found bit per value -- lives in
// registers, the value loop unrolled to 8 and guarded by j < m.  A lane stops loading once it has all m values or has left
// the wet column; after every group a wave-wide vote (__all) ends the loop of the wave when no lane needs more, so a mixed
// layer in the top tenth of the column costs the top tenth (plus at most one group) of the bytes.  The level vector travels as
// a kernel argument (at most NF_ISO_MAX_LEVELS levels) and is read with scalar loads: the level index is uniform.
// No LDS, no atomics, no dependence on the launch shape: a lane reads and writes its own column only.  All offsets are 64-bit.
// One column per lane at both dtypes; the two-columns-per-lane form (16-byte loads at float64) was not built, see
// docs/EXPERIMENTS.md.
// Launch shape, decided with -Rpass-analysis=kernel-resource-usage (no instantiation uses scratch memory) and measured at one
// step of the bench shape (tools/iso_depth_timing.py; the figures are in profiles/iso_depth_timing.txt and
// docs/EXPERIMENTS.md): block 256; 32 bytes of a column per group.
// Algorithmic bytes: levels read * n * sizeof(T) (twice that in the e3t form) + m * n * sizeof(T).
#include "nf_capi.h"

// bytes of one column that a lane has in flight: a group of 4 levels at float64, of 8 at float32
#ifndef NF_ISO_GROUP_BYTES
#define NF_ISO_GROUP_BYTES 32
#endif
#define NF_ISO_MAX_VALUES 8
#define NF_ISO_MAX_LEVELS 256

namespace nf {

namespace {

// the level vector as a kernel argument; the e3t form carries none
template <bool E3T> struct IsoLevels {
    double h[NF_ISO_MAX_LEVELS];
};
template <> struct IsoLevels<true> {
};

template <typename T> struct IsoIn {
    const T *tau, *e3t;
    T t1, t2, e1, e2;     // the markers of the tracer, of e3t
    T fill_out;
    double top, zref;
    double values[NF_ISO_MAX_VALUES];
    double sign;      // +1: the tracer rises downward; -1: it falls, and the kernel works on -tau and -theta
    int nz, m;
};

}  // namespace

// 256 threads, one column per lane; grid = ceil(n / 256).  REL: thresholds relative to the value at zref; E3T: thicknesses from
// the e3t array, else from lv.
// A falling tracer (sense -1) is searched as the rising tracer -tau against -theta: negation is exact and every IEEE operation
// of the definition is symmetric under it (a quotient of two negated numbers, a difference of two negated numbers), so the
// depths are the same bits and the level loop holds one comparison per value.
// The level loop is made for the levels where nothing is reached, which are nearly all: per level one comparison per value
// still sought, or-ed into one flag; only a lane whose flag is set goes through the values again to take its results.
template <typename T, bool REL, bool E3T, int U>
__global__ __launch_bounds__(256) void k_iso_depth(T *out, IsoIn<T> in, IsoLevels<E3T> lv, size_t n)
{
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    const bool mine = i < n;
    const int nz = in.nz, m = in.m;
    const double sign = in.sign;
    double th[NF_ISO_MAX_VALUES], res[NF_ISO_MAX_VALUES];
    bool fnd[NF_ISO_MAX_VALUES];
#pragma unroll
    for (int j = 0; j < NF_ISO_MAX_VALUES; ++j) {
        th[j] = sign * in.values[j];
        res[j] = 0.0;
        fnd[j] = j >= m;    // the values past m count as found
    }
    int left = m;           // values still sought
    bool active = mine;     // inside the leading run of wet levels and still looking for a value
    bool ref = !REL;        // the thresholds are known
    bool any_wet = false;
    double D = in.top;      // D_k, the upper interface of the level in hand
    double ca = 0.0, ta = 0.0, c0 = 0.0;   // centre and value of the level above; centre of level 0

    for (int kg = 0; kg < nz; kg += U) {
        T tv[U], hv[U];
#pragma unroll
        for (int u = 0; u < U; ++u) {
            const int k = kg + u;
            tv[u] = in.t1;
            hv[u] = (T)0;
            if (active && k < nz) {
                const size_t at = (size_t)k * n + i;
                tv[u] = __builtin_nontemporal_load(in.tau + at);
                if (E3T) hv[u] = __builtin_nontemporal_load(in.e3t + at);
            }
        }
#pragma unroll
        for (int u = 0; u < U; ++u) {
            const int k = kg + u;
            if (!active || k >= nz) continue;
            bool wet = tr_present<T>(tv[u], in.t1, in.t2);
            double h;
            if constexpr (E3T) h = (double)hv[u];
            else h = lv.h[k];
            if (E3T) wet = wet && tr_present<T>(hv[u], in.e1, in.e2) && h > 0.0 && h <= std::numeric_limits<double>::max();
            if (!wet) {
                active = false;     // the column ended at level k - 1
                continue;
            }
            const double t = sign * (double)tv[u];
            const double c = D + 0.5 * h;
            bool search = true;
            if (REL && !ref) {
                if (c <= in.zref) {
                    search = false;     // level k may be kref
                } else {
                    double tref;
                    if (!any_wet) {     // zref above c_0: kref = 0, the search begins at level 1
                        tref = t;
                        search = false;
                    } else {            // kref = k - 1, the search begins here
                        tref = in.zref <= c0 ? ta : ta + (t - ta) * ((in.zref - ca) / (c - ca));
                    }
#pragma unroll
                    for (int j = 0; j < NF_ISO_MAX_VALUES; ++j) th[j] = tref + sign * in.values[j];
                    ref = true;
                }
            }
            if (search) {
                bool hit = false;
#pragma unroll
                for (int j = 0; j < NF_ISO_MAX_VALUES; ++j) {
                    if (j >= m) break;
                    hit = hit | (!fnd[j] & (t >= th[j]));
                }
                if (hit) {
#pragma unroll
                    for (int j = 0; j < NF_ISO_MAX_VALUES; ++j) {
                        if (j < m && !fnd[j] && t >= th[j]) {
                            fnd[j] = true;
                            --left;
                            if (!any_wet) res[j] = D;     // level 0: the surface outcrops
                            else if (REL && ta >= th[j]) res[j] = in.zref;
                            else res[j] = ca + (c - ca) * ((th[j] - ta) / (t - ta));
                        }
                    }
                }
            }
            if (!any_wet) c0 = c;
            any_wet = true;
            D = D + h;
            ca = c;
            ta = t;
            if (left == 0) active = false;
        }
        if (__all(!active)) break;
    }
    if (!mine) return;
#pragma unroll
    for (int j = 0; j < NF_ISO_MAX_VALUES; ++j) {
        if (j >= m) continue;
        // not found: the sea bed D_{kb+1}; no wet level at all: fill_out
        const T v = !any_wet ? in.fill_out : (T)(fnd[j] ? res[j] : D);
        __builtin_nontemporal_store(v, out + (size_t)j * n + i);
    }
}

namespace {

struct IsoArgs {
    void *out;
    const void *tau, *e3t;
    const double *thickness;
    long nz;
    size_t n;
    double tau_fill, tau_missing, e3t_fill, e3t_missing, top, zref, fill_out;
    const double *values;
    int m, sense, relative;
};

template <typename T, bool REL, bool E3T>
int launch_iso_v(const IsoArgs &a, hipStream_t s)
{
    IsoIn<T> in{};
    in.tau = (const T *)a.tau;
    in.e3t = (const T *)a.e3t;
    in.t1 = (T)a.tau_fill;
    in.t2 = (T)a.tau_missing;
    in.e1 = (T)a.e3t_fill;
    in.e2 = (T)a.e3t_missing;
    in.fill_out = (T)a.fill_out;
    in.top = a.top;
    in.zref = a.zref;
    for (int j = 0; j < NF_ISO_MAX_VALUES; ++j) in.values[j] = j < a.m ? a.values[j] : 0.0;
    in.nz = (int)a.nz;
    in.m = a.m;
    in.sign = a.sense > 0 ? 1.0 : -1.0;
    IsoLevels<E3T> lv{};
    if constexpr (!E3T)
        for (long k = 0; k < a.nz; ++k) lv.h[k] = a.thickness[k];
    const size_t blocks = (a.n + 255) / 256;
    NF_REQUIRE(blocks <= 0x7ffffff0u, NF_ERR_ARG, "nf_iso_depth: ny * nx is too large for one launch");
    hipLaunchKernelGGL((k_iso_depth<T, REL, E3T, NF_ISO_GROUP_BYTES / (int)sizeof(T)>), dim3((unsigned)blocks), dim3(256), 0, s, (T *)a.out, in, lv,
                       a.n);
    NF_HIP(hipGetLastError());
    return NF_OK;
}

template <typename T>
int launch_iso_t(const IsoArgs &a, hipStream_t s)
{
    if (a.e3t) return a.relative ? launch_iso_v<T, true, true>(a, s) : launch_iso_v<T, false, true>(a, s);
    return a.relative ? launch_iso_v<T, true, false>(a, s) : launch_iso_v<T, false, false>(a, s);
}

// [p, p + pbytes) and [q, q + qbytes) share a byte
inline bool ranges_overlap(const void *p, size_t pbytes, const void *q, size_t qbytes)
{
    const uintptr_t a = (uintptr_t)p, b = (uintptr_t)q;
    return a < b ? b - a < pbytes : a - b < qbytes;
}

inline bool iso_finite(double x) { return x >= -std::numeric_limits<double>::max() && x <= std::numeric_limits<double>::max(); }

}  // namespace

}  // namespace nf

using namespace nf;

extern "C" int nf_iso_depth(void *out_dev, const void *tau_dev, const double *thickness_host, const void *e3t_dev, long nz, long ny,
                            long nx, int dtype, double tau_fill, double tau_missing, double e3t_fill, double e3t_missing,
                            double top, const double *values, int m, int sense, int relative, double zref, double fill_out,
                            void *hip_stream)
try {
    NF_REQUIRE(dtype == NF_F64 || dtype == NF_F32, NF_ERR_ARG, "nf_iso_depth: dtype must be NF_F64 or NF_F32");
    NF_REQUIRE(out_dev && tau_dev && values, NF_ERR_ARG, "nf_iso_depth: null out_dev, tau_dev or values");
    NF_REQUIRE((thickness_host != nullptr) != (e3t_dev != nullptr), NF_ERR_ARG,
               "nf_iso_depth: give exactly one of thickness_host (nz level thicknesses) and e3t_dev ((nz, ny, nx) in HBM)");
    NF_REQUIRE(m >= 1 && m <= NF_ISO_MAX_VALUES, NF_ERR_ARG, "nf_iso_depth: m must be 1 .. 8");
    NF_REQUIRE(sense == 1 || sense == -1, NF_ERR_ARG, "nf_iso_depth: sense must be +1 (rising downward) or -1 (falling)");
    NF_REQUIRE(relative == 0 || relative == 1, NF_ERR_ARG, "nf_iso_depth: relative must be 0 or 1");
    NF_REQUIRE(iso_finite(top), NF_ERR_ARG, "nf_iso_depth: top must be finite");
    NF_REQUIRE(iso_finite(zref), NF_ERR_ARG, "nf_iso_depth: zref must be finite");
    for (int j = 0; j < m; ++j) NF_REQUIRE(iso_finite(values[j]), NF_ERR_ARG, "nf_iso_depth: every value must be finite");
    NF_REQUIRE(nz >= 1 && ny >= 1 && nx >= 1, NF_ERR_ARG, "nf_iso_depth: nz, ny and nx must be >= 1");
    NF_REQUIRE(thickness_host == nullptr || nz <= NF_ISO_MAX_LEVELS, NF_ERR_ARG,
               "nf_iso_depth: the level-vector form takes at most 256 levels; give e3t_dev");
    NF_REQUIRE(nz <= 0x7fffffffl, NF_ERR_ARG, "nf_iso_depth: nz is too large");
    if (thickness_host)
        for (long k = 0; k < nz; ++k)
            NF_REQUIRE(thickness_host[k] > 0.0 && iso_finite(thickness_host[k]), NF_ERR_ARG,
                       "nf_iso_depth: every thickness of thickness_host must be finite and > 0");
    const size_t size = dtype == NF_F64 ? sizeof(double) : sizeof(float);
    const size_t lim = std::numeric_limits<size_t>::max() / size;
    NF_REQUIRE((size_t)ny <= lim / (size_t)nx && (size_t)ny * (size_t)nx <= lim / (size_t)nz, NF_ERR_ARG,
               "nf_iso_depth: nz * ny * nx is too large");
    const size_t n = (size_t)ny * (size_t)nx;
    const size_t in_bytes = (size_t)nz * n * size, out_bytes = (size_t)m * n * size;
    NF_REQUIRE(!ranges_overlap(out_dev, out_bytes, tau_dev, in_bytes) &&
                   !(e3t_dev && ranges_overlap(out_dev, out_bytes, e3t_dev, in_bytes)),
               NF_ERR_ARG, "nf_iso_depth: out_dev overlaps tau_dev or e3t_dev");
    NF_NEED_DEVICE();
    const IsoArgs a{out_dev, tau_dev, e3t_dev, thickness_host, nz, n, tau_fill, tau_missing, e3t_fill, e3t_missing, top, zref,
                    fill_out, values, m, sense, relative};
    hipStream_t s = (hipStream_t)hip_stream;
    return dtype == NF_F64 ? launch_iso_t<double>(a, s) : launch_iso_t<float>(a, s);
}
NF_API_CATCH
