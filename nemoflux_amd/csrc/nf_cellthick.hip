// nf_cellthick.hip -- K1e3: the vertical integral of one time step with PER-CELL layer thicknesses (partial steps, z* /
// variable-volume runs: e3u / e3v, or thkcello on the U and V grids), fused with K1's edge-flux assembly.
//
// Definition.  e3u sits on the index of uo (the east face of cell c), e3v on the index of vo: no interpolation, no neighbour.
//   fixth(x) = 0 if x is NaN or one of the thickness's two markers (compared in the field dtype), else (double)x
//   accU(c) = fma(fixth(e3u[z, c]), fixed(uo[z, c]), accU(c)),  accV(c) likewise with e3v and vo,  z ascending over [z0, z1)
//   eU = +accU * arcE, eV = -accV * arcN, each times the Sverdrup scale when it is on -- K1's epilogue, in K1's order.
// With e3u[z, c] == e3v[z, c] == thickness[z] the planes are K1's bit for bit.
//
// Access pattern: K1's.  A lane owns VEC consecutive cells (16 B of the field dtype) and walks z with stride ncell; all
// loads of a batch of UZ levels -- four aligned non-temporal streams per level (u, v, e3u, e3v) -- are issued before the first
// use.  The kernel stores the two signed planes and raises the running max, as the signed-only form of K1 does;
// launch_expand_planes derives the south / west copies and the |.| planes behind it.
//
// Algorithmic bytes per (t,z,j,i): 4*sizeof(T) read + (16 arc + 16 planes)/nz.
#include "nf_lanes.h"

namespace nf {

// 256 threads, one chunk of VEC cells per lane: c0 = (tile * 256 + tid) * VEC; ncell % VEC == 0 (the launcher picks VEC = 1
// otherwise), so a lane's cells are all there or all absent
template <typename T, int VEC, int UZ>
__global__ __launch_bounds__(256) void k_cellthick_flux(const T *__restrict__ u, const T *__restrict__ v,
                                                        const T *__restrict__ e3u, const T *__restrict__ e3v, long ncell,
                                                        int z0, int z1, const double *__restrict__ arcE,
                                                        const double *__restrict__ arcN, T fill, T fill2, T thfill,
                                                        T thfill2, double scale, int sverdrup, double *__restrict__ planes,
                                                        unsigned long long *maxbits, unsigned ntiles)
{
    const unsigned tile = xcd_tile(blockIdx.x, gridDim.x);
    double tmax = 0.0;
    const long c0 = ((long)tile * 256 + threadIdx.x) * VEC;
    if (tile < ntiles && c0 < ncell) {
        double accU[VEC], accV[VEC];
#pragma unroll
        for (int k = 0; k < VEC; ++k) accU[k] = accV[k] = 0.0;
        const long o0 = (long)z0 * ncell + c0;
        const T *pu = u + o0, *pv = v + o0, *pe = e3u + o0, *pf = e3v + o0;
        for (int z = z0; z < z1; z += UZ) {
            const int nlev = z1 - z < UZ ? z1 - z : UZ;   // wave-uniform
            Lanes<T, VEC> lu[UZ], lv[UZ], le[UZ], lf[UZ];
#pragma unroll
            for (int r = 0; r < UZ; ++r)
                if (r < nlev) {
                    const long o = (long)r * ncell;
                    lu[r] = lane_load<T, VEC, true>(pu + o);
                    le[r] = lane_load<T, VEC, true>(pe + o);
                    lv[r] = lane_load<T, VEC, true>(pv + o);
                    lf[r] = lane_load<T, VEC, true>(pf + o);
                }
#pragma unroll
            for (int r = 0; r < UZ; ++r)
                if (r < nlev) {
#pragma unroll
                    for (int k = 0; k < VEC; ++k) {
                        accU[k] = fma(thick_fixed<T>(le[r].x[k], thfill, thfill2), uv_fixed<T>(lu[r].x[k], fill, fill2), accU[k]);
                        accV[k] = fma(thick_fixed<T>(lf[r].x[k], thfill, thfill2), uv_fixed<T>(lv[r].x[k], fill, fill2), accV[k]);
                    }
                }
            const long adv = (long)UZ * ncell;
            pu += adv, pv += adv, pe += adv, pf += adv;
        }
        // edge terms in K1's order (field.py:195-196, 225-228)
        double eU[VEC], eV[VEC];
#pragma unroll
        for (int k = 0; k < VEC; ++k) {
            eU[k] = +accU[k] * arcE[c0 + k];
            eV[k] = -accV[k] * arcN[c0 + k];
            if (sverdrup) {
                eU[k] *= scale;
                eV[k] *= scale;
            }
            tmax = fmax(tmax, fmax(fabs(eU[k]), fabs(eV[k])));
        }
        double *pU = planes + c0, *pV = planes + ncell + c0;
        if (VEC == 1) {
            __builtin_nontemporal_store(eU[0], pU);
            __builtin_nontemporal_store(eV[0], pV);
        } else {
#pragma unroll
            for (int k = 0; k < VEC; k += 2) {
                const dvec2 a = {eU[k], eU[k + 1 < VEC ? k + 1 : k]}, b = {eV[k], eV[k + 1 < VEC ? k + 1 : k]};
                __builtin_nontemporal_store(a, reinterpret_cast<dvec2 *>(pU + k));
                __builtin_nontemporal_store(b, reinterpret_cast<dvec2 *>(pV + k));
            }
        }
    }
    // running max (field.py:234), as K1 keeps it: wavefront butterfly, at most one atomic per wavefront, issued only by a
    // wave that would raise it (non-negative doubles order like their bits)
    for (int o = 32; o > 0; o >>= 1) tmax = fmax(tmax, __shfl_xor(tmax, o, kWave));
    if ((threadIdx.x & (kWave - 1)) == 0 && tmax > 0.0) {
        unsigned long long b;
        __builtin_memcpy(&b, &tmax, 8);
        if (b > __hip_atomic_load(maxbits, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)) atomicMax(maxbits, b);
    }
}

namespace {
// levels per batch: four 16-byte streams per level.  Six levels: 114 (float64) / 122 (float32) VGPRs, 4 waves per SIMD, no
// scratch (-Rpass-analysis=kernel-resource-usage): the most loads in flight (24 per lane) that keep the kernel under 128 VGPRs;
// four levels take 82 / 90 VGPRs (5 waves), eight 147 / 154 (3 waves), ten 179 / 187 (2 waves).  Measured on the bench step,
// 4 / 6 / 8 / 10 levels: 2.36 / 2.41 / 2.34 / 2.31 ms at float64, 1.30 / 1.29 / 1.28 / 1.32 ms at float32, each in a process
// of its own -- inside the 4 % by which one build differs between two processes, so the count is not decided by time
constexpr int kCellThickLevels = 6;

template <typename T, int VEC>
int launch_cellthick_t(const CellThickArgs &a, hipStream_t s)
{
    const StepInput &in = a.in;
    const ThickIn<T> th = thick_in<T>(a.th);
    const long per_tile = 256l * VEC;
    const unsigned ntiles = (unsigned)((in.ncell + per_tile - 1) / per_tile);
    hipLaunchKernelGGL((k_cellthick_flux<T, VEC, kCellThickLevels>), dim3(xcd_grid(ntiles)), dim3(256), 0, s, (const T *)in.u,
                       (const T *)in.v, th.e3u, th.e3v, in.ncell, in.z0, in.z1, in.arcE, in.arcN, (T)in.fill, (T)in.fill2, th.m1,
                       th.m2, in.scale, in.sverdrup, a.planes, a.maxbits, ntiles);
    NF_HIP(hipGetLastError());
    return NF_OK;
}

template <typename T, int VEC>
int launch_cellthick_v(const CellThickArgs &a, hipStream_t s)
{
    if (lanes_aligned16({a.in.u, a.in.v, a.th.e3u, a.th.e3v}) && a.in.ncell % VEC == 0) return launch_cellthick_t<T, VEC>(a, s);
    return launch_cellthick_t<T, 1>(a, s);   // odd sizes / unaligned arrays: one cell per lane
}
}  // namespace

int launch_cellthick_flux(const CellThickArgs &a, hipStream_t s)
{
    const StepInput &in = a.in;
    NF_REQUIRE(in.ncell > 0 && in.ncell == in.ny * in.nx && in.ncell < (1l << 31), NF_ERR_ARG, "cell-thickness flux: bad grid sizes");
    NF_REQUIRE(in.z1 > in.z0 && in.z0 >= 0, NF_ERR_ARG, "cell-thickness flux: empty z range");
    NF_REQUIRE(in.u && in.v && a.th.e3u && a.th.e3v && a.planes && a.maxbits && in.arcE && in.arcN, NF_ERR_ARG,
               "cell-thickness flux: null argument");
    if (in.dtype == NF_F64) return launch_cellthick_v<double, 2>(a, s);
    if (in.dtype == NF_F32) return launch_cellthick_v<float, 4>(a, s);
    NF_REQUIRE(false, NF_ERR_ARG, "cell-thickness flux: dtype must be NF_F64 or NF_F32");
}

}  // namespace nf
