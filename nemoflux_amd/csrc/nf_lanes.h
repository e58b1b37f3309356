// nf_lanes.h -- the lane loader of the streaming kernels that are built like K1 (nf_tracer.hip, nf_cellthick.hip,
// nf_timemean.hip, nf_eos.hip; internal).  A lane owns VEC consecutive values -- 16 bytes: 2 doubles, 4 floats or 4 counts -- or one value
// where some array is not 16-byte aligned.  K1 keeps its own copy: nf_flux.hip is fingerprinted by the benchmark.
#pragma once
#include "nf_common.h"

#include <initializer_list>

namespace nf {

namespace {   // as in the files that include this: nothing here has a name outside its translation unit

typedef double dvec2 __attribute__((ext_vector_type(2)));   // clang vectors: accepted by the non-temporal builtins
typedef float fvec4 __attribute__((ext_vector_type(4)));
typedef unsigned uvec2 __attribute__((ext_vector_type(2)));
typedef unsigned uvec4 __attribute__((ext_vector_type(4)));
template <typename T, int VEC> struct lane_vec;
template <> struct lane_vec<double, 2> { using type = dvec2; };
template <> struct lane_vec<float, 4> { using type = fvec4; };
template <> struct lane_vec<unsigned, 2> { using type = uvec2; };
template <> struct lane_vec<unsigned, 4> { using type = uvec4; };
template <> struct lane_vec<double, 1> { using type = double; };
template <> struct lane_vec<float, 1> { using type = float; };
template <> struct lane_vec<unsigned, 1> { using type = unsigned; };

template <typename T, int VEC> struct Lanes {
    T x[VEC];
};

// VEC consecutive values at p; ALIGNED: p is aligned to VEC * sizeof(T) and they come in one load; NT: read once (non-temporal)
template <typename T, int VEC, bool NT, bool ALIGNED = true>
__device__ inline Lanes<T, VEC> lane_load(const T *p)
{
    Lanes<T, VEC> r;
    if (ALIGNED) {
        using V = typename lane_vec<T, VEC>::type;
        V v = NT ? __builtin_nontemporal_load(reinterpret_cast<const V *>(p)) : *reinterpret_cast<const V *>(p);
        __builtin_memcpy(&r, &v, sizeof(V));
    } else {
#pragma unroll
        for (int k = 0; k < VEC; ++k) r.x[k] = p[k];
    }
    return r;
}
// VEC values to p (aligned to VEC * sizeof(T)) in one non-temporal store
template <typename T, int VEC>
__device__ inline void lane_store(T *p, const Lanes<T, VEC> &r)
{
    using V = typename lane_vec<T, VEC>::type;
    V v;
    __builtin_memcpy(&v, &r, sizeof(V));
    __builtin_nontemporal_store(v, reinterpret_cast<V *>(p));
}

// Host side: may a lane take 16 bytes at a time?  Every pointer is 16-byte aligned (a null one is an array that is not read)
// and, with more than one step, so is every stride in bytes.
inline bool lanes_aligned16(std::initializer_list<const void *> ptrs, long nsteps = 1,
                            std::initializer_list<long long> stride_bytes = {})
{
    bool al16 = true;
    for (const void *p : ptrs) al16 = al16 && (uintptr_t)p % 16 == 0;
    if (nsteps > 1)
        for (long long b : stride_bytes) al16 = al16 && b % 16 == 0;
    return al16;
}

}  // namespace

}  // namespace nf
