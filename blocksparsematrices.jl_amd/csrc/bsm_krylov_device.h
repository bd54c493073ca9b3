// bsm_krylov_device.h -- the device-side pieces of a classical Gram-Schmidt pass that bsm_krylov.hip (bsm_krylov_orth: one
// column of any alignment) and bsm_gmres_multi.hip (the GMRES solvers: padded workspace columns in lockstep) share: the
// update of a tile on the elements of one 16-byte group, the fixed-order sum of a pass's partials, and the dot of a tile
// as a statement macro at the end of this file.  The units differ in how they reach their vectors (guarded groups of any
// alignment there, unguarded groups of padded workspace columns here).  For the kernel units only.
#pragma once
#include <hip/hip_runtime.h>

#include "bsm_krylov.h"

namespace bsm {

// w += v h over the VE elements of one group, h = (hr, hi)
template <typename R, int NC, int VE> __device__ __forceinline__ void gs_axpy(const R *v, R hr, R hi, R *w) {
#pragma unroll
    for (int e = 0; e < VE; ++e) {
        if (NC == 1) {
            w[e] = fma(v[e], hr, w[e]);
        } else {
            const R vr = v[e * NC], vi = v[e * NC + NC - 1];
            w[e * NC] = fma(vr, hr, w[e * NC]);
            w[e * NC] = fma(-vi, hi, w[e * NC]);
            w[e * NC + NC - 1] = fma(vr, hi, w[e * NC + NC - 1]);
            w[e * NC + NC - 1] = fma(vi, hr, w[e * NC + NC - 1]);
        }
    }
}

// The sum of the G partials part[(c * G + g) * NC ..] of each of k <= BSM_GMRES_MAX_RESTART columns by a workgroup of
// `threads` (a multiple of 64) in one fixed order: S threads per column (a power of two, at most a wave), column c = t / S --
// its lanes are neighbours in one wave --, strided, then xor-shuffles.  -> true in the one thread per column (c < k) that
// holds the sum in a.
template <typename R, int NC>
__device__ __forceinline__ bool gs_sum_partials(const R *__restrict__ part, int k, int G, int t, int threads, int &c, R (&a)[NC]) {
    int kp = 1;
    while (kp < k) kp <<= 1;
    int S = threads / kp;
    if (S > 64) S = 64;
    c = t / S;
    const int sl = t % S;
#pragma unroll
    for (int q = 0; q < NC; ++q) a[q] = R(0);
    if (c < k)
        for (int g = sl; g < G; g += S) {
#pragma unroll
            for (int q = 0; q < NC; ++q) a[q] += part[((long long)c * G + g) * NC + q];
        }
    for (int d = S >> 1; d >= 1; d >>= 1) {
#pragma unroll
        for (int q = 0; q < NC; ++q) a[q] += __shfl_xor(a[q], d, 64);
    }
    return c < k && sl == 0;
}

// ---- a statement both units expand in place.  A macro, not a function: as a function the dot tile compiled to another
// register count in bsm_krylov.hip (docs/experiments_r25.md); an expansion is the very statements that unit had.
// s[0 .. NC) += conj(v) w over the VE elements of one group (v, w: arrays of reals; s: NC sums)
#define BSM_GS_DOT(R, NC, VE, v, w, s)                                      \
    _Pragma("unroll") for (int e = 0; e < VE; ++e) {                        \
        if (NC == 1) {                                                      \
            (s)[0] = fma((v)[e], (w)[e], (s)[0]);                           \
        } else { /* conj(v) * w */                                          \
            const R vr = (v)[e * NC], vi = (v)[e * NC + NC - 1];            \
            const R wr = (w)[e * NC], wi = (w)[e * NC + NC - 1];            \
            (s)[0] = fma(vr, wr, (s)[0]);                                   \
            (s)[0] = fma(vi, wi, (s)[0]);                                   \
            (s)[NC - 1] = fma(vr, wi, (s)[NC - 1]);                         \
            (s)[NC - 1] = fma(-vi, wr, (s)[NC - 1]);                        \
        }                                                                   \
    }

}  // namespace bsm
