// nf_tracer.hip -- K1tau: tracer transport across the cell faces of one time step (heat, salt): the vertical integral of
// u * tau_face over the owned levels, fused with the edge-flux assembly of K1.  K3 (planes = 2) reduces its two planes.
//
// Definition.  tau sits at T-points, (nt, nz, ny, nx) like uo / vo.  For cell c = (j, i) and level z,
// a = tau[z, j, i]; the east face's b = tau[z, j, i+1] (column nx-1: tau[z, j, 0] when wrap_x, else none), the north face's
// b = tau[z, j+1, i] (last row: none).  A value is present when it is not NaN and not one of the tracer's two markers.
//   tf = 0.5 (a + b) - ref  (both present),  the present one - ref  (one),  0  (neither)
//   accU = fma(th_z, fixed(u) * tfE, accU), z ascending; eU_tau = +accU * arcE (* scale), eV_tau = -accV * arcN (* scale)
// fixed() is K1's masking of uo / vo.  With tau == ref + 1 every tf is exactly 1 and the planes are K1's eU, eV bit for bit.
//
// Access pattern: K1's.  A lane owns VEC consecutive cells (16 B of the field dtype) and walks z with stride ncell, issuing
// all loads of a batch of UZ levels before the first use.  Per level it loads u, v, tau and the tau of the row above (a second
// contiguous stream at +nx, which the waves nx cells further on read as their own row at about the same time: served on
// die).  The east neighbour of a lane's last cell is the first cell of the next lane (a cross-lane shift); the last lane of
// a wavefront loads it itself, and the lane that holds a row's last column loads the row's first cell for the wrap.
//
// Algorithmic bytes per (t,z,j,i): 3*sizeof(T) read + (16 arc + 16 planes)/nz.
//
// Cell-thickness form (nf_field_set_cell_thickness; trailing kernel argument ThickIn<T>): th_z becomes the thickness read at
// the face, accU = fma(fixth(e3u[z, c]), fixed(u) * tfE, accU) and accV with e3v -- two more aligned non-temporal streams,
// 5*sizeof(T) per (t,z,j,i).  The form without the argument is the kernel as it was, instruction for instruction.
#include "nf_lanes.h"

namespace nf {

// 256 threads, one chunk of VEC cells per lane: lane c0 = (tile * 256 + tid) * VEC.  ncell % VEC == 0 and nx >= VEC (the
// launcher picks VEC = 1 otherwise), so a lane's cells hold at most one row end.  NAL: nx % VEC == 0, the north stream is
// 16-byte aligned too.  TH: empty (per-level thickness) or one ThickIn<T>.
template <typename T>
__device__ inline ThickIn<T> tr_thick() { return ThickIn<T>{}; }
template <typename T>
__device__ inline ThickIn<T> tr_thick(const ThickIn<T> &th) { return th; }

template <typename T, int VEC, int UZ, bool NAL, typename... TH>
__global__ __launch_bounds__(256) void k_tracer_flux(const T *__restrict__ u, const T *__restrict__ v,
                                                     const T *__restrict__ tau, long ncell, unsigned nx, int z0, int z1,
                                                     const double *__restrict__ thickness, const double *__restrict__ arcE,
                                                     const double *__restrict__ arcN, T fill, T fill2, T tfill, T tfill2,
                                                     double ref, int wrap_x, double scale, int sverdrup,
                                                     double *__restrict__ planes, unsigned ntiles, TH... thick)
{
    constexpr bool CT = sizeof...(TH) > 0;
    const ThickIn<T> ct = tr_thick<T>(thick...);
    const unsigned tile = xcd_tile(blockIdx.x, gridDim.x);
    if (tile >= ntiles) return;   // workgroup-uniform
    const int lane = threadIdx.x & (kWave - 1);
    const long c0 = ((long)tile * 256 + threadIdx.x) * VEC;
    const bool on = c0 < ncell;   // a lane's cells are all there or all absent
    // neighbour bookkeeping, once per lane
    const long cs = on ? c0 : 0;
    const unsigned i0 = (unsigned)(cs % nx);
    const int kend = (nx - 1 - i0 < (unsigned)VEC) ? (int)(nx - 1 - i0) : -1;   // the cell in column nx-1, if any
    const bool wrap = on && kend >= 0 && wrap_x;                                // it loads its row's first cell
    const long cwrap = cs + kend + 1 - (long)nx;
    // the east neighbour of the last cell comes from the next lane, except at the end of a wavefront
    const bool own_next = on && lane == kWave - 1 && kend != VEC - 1 && c0 + VEC < ncell;
    const bool north_all = on && c0 + VEC - 1 + (long)nx < ncell;
    bool has_n[VEC];
#pragma unroll
    for (int k = 0; k < VEC; ++k) has_n[k] = on && c0 + k + (long)nx < ncell;

    double accU[VEC], accV[VEC];
#pragma unroll
    for (int k = 0; k < VEC; ++k) accU[k] = accV[k] = 0.0;
    const T *pu = u + (long)z0 * ncell + cs;
    const T *pv = v + (long)z0 * ncell + cs;
    const T *pt = tau + (long)z0 * ncell + cs;
    const T *pe = CT ? ct.e3u + (long)z0 * ncell + cs : nullptr;
    const T *pf = CT ? ct.e3v + (long)z0 * ncell + cs : nullptr;
    for (int z = z0; z < z1; z += UZ) {
        const int nlev = z1 - z < UZ ? z1 - z : UZ;
        Lanes<T, VEC> lu[UZ], lv[UZ], lt[UZ], ln[UZ];
        Lanes<T, VEC> le[CT ? UZ : 1], lf[CT ? UZ : 1];
        T nx1[UZ], wv[UZ];
#pragma unroll
        for (int r = 0; r < UZ; ++r)
            if (r < nlev) {
                const long o = (long)r * ncell;
                if (on) {
                    lu[r] = lane_load<T, VEC, true>(pu + o);
                    lv[r] = lane_load<T, VEC, true>(pv + o);
                    lt[r] = lane_load<T, VEC, false>(pt + o);
                    if constexpr (CT) {
                        le[r] = lane_load<T, VEC, true>(pe + o);
                        lf[r] = lane_load<T, VEC, true>(pf + o);
                    }
                } else {
#pragma unroll
                    for (int k = 0; k < VEC; ++k) lu[r].x[k] = lv[r].x[k] = lt[r].x[k] = T(0);
                    if constexpr (CT) {
#pragma unroll
                        for (int k = 0; k < VEC; ++k) le[r].x[k] = lf[r].x[k] = T(0);
                    }
                }
                if (north_all) {
                    ln[r] = lane_load<T, VEC, false, NAL>(pt + o + nx);
                } else {
#pragma unroll
                    for (int k = 0; k < VEC; ++k) ln[r].x[k] = has_n[k] ? pt[o + nx + k] : T(0);
                }
                nx1[r] = own_next ? pt[o + VEC] : T(0);
                wv[r] = wrap ? pt[o + (cwrap - cs)] : T(0);
            }
#pragma unroll
        for (int r = 0; r < UZ; ++r)
            if (r < nlev) {
                const double th = thickness[z + r];
                // every lane takes part in the shift (inactive lanes hand on zeros)
                const T sh = __shfl_down(lt[r].x[0], 1, kWave);
                const T next = own_next ? nx1[r] : sh;
#pragma unroll
                for (int k = 0; k < VEC; ++k) {
                    const T a = lt[r].x[k];
                    const T be = k == kend ? wv[r] : (k + 1 < VEC ? lt[r].x[k + 1 < VEC ? k + 1 : k] : next);
                    const bool has_e = k != kend || wrap_x;
                    const double tfE = tr_face<T>(a, be, has_e, tfill, tfill2, ref);
                    const double tfN = tr_face<T>(a, ln[r].x[k], has_n[k], tfill, tfill2, ref);
                    if constexpr (CT) {
                        accU[k] = fma(thick_fixed<T>(le[r].x[k], ct.m1, ct.m2), uv_fixed<T>(lu[r].x[k], fill, fill2) * tfE, accU[k]);
                        accV[k] = fma(thick_fixed<T>(lf[r].x[k], ct.m1, ct.m2), uv_fixed<T>(lv[r].x[k], fill, fill2) * tfN, accV[k]);
                    } else {
                        accU[k] = fma(th, uv_fixed<T>(lu[r].x[k], fill, fill2) * tfE, accU[k]);
                        accV[k] = fma(th, uv_fixed<T>(lv[r].x[k], fill, fill2) * tfN, accV[k]);
                    }
                }
            }
        pu += (long)UZ * ncell;
        pv += (long)UZ * ncell;
        pt += (long)UZ * ncell;
        if constexpr (CT) {
            pe += (long)UZ * ncell;
            pf += (long)UZ * ncell;
        }
    }
    if (!on) return;
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
    }
    double *pU = planes + c0, *pV = planes + ncell + c0;
    if (VEC == 1) {
        pU[0] = eU[0];
        pV[0] = eV[0];
    } else {
#pragma unroll
        for (int k = 0; k < VEC; k += 2) {
            *reinterpret_cast<double2 *>(pU + k) = make_double2(eU[k], eU[k + 1 < VEC ? k + 1 : k]);
            *reinterpret_cast<double2 *>(pV + k) = make_double2(eV[k], eV[k + 1 < VEC ? k + 1 : k]);
        }
    }
}

namespace {
// levels per batch: four 16-byte streams per level.  Four levels: 110 VGPRs, 4 waves per SIMD, no scratch
// (-Rpass-analysis=kernel-resource-usage); five levels take 133 VGPRs and 3 waves
constexpr int kTracerLevels = 4;
// the cell-thickness form has six 16-byte streams per level.  Three levels: 114 (float64) / 127 (float32) VGPRs, 4 waves per
// SIMD, no scratch; four levels take 145 / 155 VGPRs and 3 waves, two 84 / 99 and 5 / 4 waves with a third fewer loads in flight
constexpr int kTracerLevelsCellThick = 3;

template <typename T, int VEC, bool NAL>
int launch_tracer_t(const TracerArgs &a, hipStream_t s)
{
    const StepInput &in = a.in;
    const long per_tile = 256l * VEC;
    const unsigned ntiles = (unsigned)((in.ncell + per_tile - 1) / per_tile);
    const unsigned grid = xcd_grid(ntiles);
    if (a.th.e3u)
        hipLaunchKernelGGL((k_tracer_flux<T, VEC, kTracerLevelsCellThick, NAL, ThickIn<T>>), dim3(grid), dim3(256), 0, s,
                           (const T *)in.u, (const T *)in.v, (const T *)a.t.tau, in.ncell, (unsigned)in.nx, in.z0, in.z1,
                           in.thickness, in.arcE, in.arcN, (T)in.fill, (T)in.fill2, (T)a.t.fill, (T)a.t.fill2, a.t.ref,
                           a.t.wrap_x ? 1 : 0, in.scale, in.sverdrup, a.planes, ntiles, thick_in<T>(a.th));
    else
        hipLaunchKernelGGL((k_tracer_flux<T, VEC, kTracerLevels, NAL>), dim3(grid), dim3(256), 0, s, (const T *)in.u,
                           (const T *)in.v, (const T *)a.t.tau, in.ncell, (unsigned)in.nx, in.z0, in.z1, in.thickness, in.arcE,
                           in.arcN, (T)in.fill, (T)in.fill2, (T)a.t.fill, (T)a.t.fill2, a.t.ref, a.t.wrap_x ? 1 : 0, in.scale,
                           in.sverdrup, a.planes, ntiles);
    NF_HIP(hipGetLastError());
    return NF_OK;
}

template <typename T, int VEC>
int launch_tracer_v(const TracerArgs &a, hipStream_t s)
{
    const StepInput &in = a.in;
    if (lanes_aligned16({in.u, in.v, a.t.tau, a.th.e3u, a.th.e3v}) && in.ncell % VEC == 0 && in.nx >= VEC)
        return in.nx % VEC == 0 ? launch_tracer_t<T, VEC, true>(a, s) : launch_tracer_t<T, VEC, false>(a, s);
    return launch_tracer_t<T, 1, true>(a, s);   // odd sizes / unaligned fields: one cell per lane
}
}  // namespace

int launch_tracer_flux(const TracerArgs &a, hipStream_t s)
{
    const StepInput &in = a.in;
    NF_REQUIRE(in.ncell > 0 && in.nx > 0 && in.ncell == in.ny * in.nx && in.ncell < (1l << 31), NF_ERR_ARG,
               "tracer flux: bad grid sizes");
    NF_REQUIRE(in.z1 > in.z0 && in.z0 >= 0, NF_ERR_ARG, "tracer flux: empty z range");
    NF_REQUIRE(in.u && in.v && a.t.tau && a.planes && in.thickness && in.arcE && in.arcN && (!a.th.e3u || a.th.e3v), NF_ERR_ARG,
               "tracer flux: null argument");
    if (in.dtype == NF_F64) return launch_tracer_v<double, 2>(a, s);
    if (in.dtype == NF_F32) return launch_tracer_v<float, 4>(a, s);
    NF_REQUIRE(false, NF_ERR_ARG, "tracer flux: dtype must be NF_F64 or NF_F32");
}

}  // namespace nf
