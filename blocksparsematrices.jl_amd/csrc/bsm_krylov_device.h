// bsm_krylov_device.h -- the device-side arithmetic of a classical Gram-Schmidt pass on the elements of one group, as
// plain functions over arrays of reals, and the fixed-order sum of a pass's partials.  bsm_krylov.hip (bsm_krylov_orth: one
// column of any alignment, guarded groups) uses them as they are; the lockstep units reach them through the Vec16 forms of
// bsm_lockstep_device.h (unguarded groups of padded workspace columns).  For the kernel units only.
#pragma once
#include <hip/hip_runtime.h>

#include "bsm_krylov.h"

namespace bsm {

// y += a x on one element: each component takes its ar term first, then its ai term.  (The one place the order of a complex
// multiply-add is written down: axpy16 has the scalar as a, the Gram-Schmidt update the vector.)
template <typename R, int NC> __device__ __forceinline__ void gs_madd(R ar, R ai, R xr, R xi, R &yr, R &yi) {
    if (NC == 1) {
        yr = fma(ar, xr, yr);
    } else {
        yr = fma(-ai, xi, fma(ar, xr, yr));
        yi = fma(ai, xr, fma(ar, xi, yi));
    }
}

// w += v h over the VE elements of one group, h = (hr, hi)
template <typename R, int NC, int VE> __device__ __forceinline__ void gs_axpy(const R *v, R hr, R hi, R *w) {
#pragma unroll
    for (int e = 0; e < VE; ++e) gs_madd<R, NC>(v[e * NC], v[e * NC + NC - 1], hr, hi, w[e * NC], w[e * NC + NC - 1]);
}

// s[0 .. NC) += conj(v) w over the VE elements of one group
template <typename R, int NC, int VE> __device__ __forceinline__ void gs_dot(const R *v, const R *w, R *s) {
#pragma unroll
    for (int e = 0; e < VE; ++e) {
        if (NC == 1) {
            s[0] = fma(v[e], w[e], s[0]);
        } else {
            const R vr = v[e * NC], vi = v[e * NC + NC - 1], wr = w[e * NC], wi = w[e * NC + NC - 1];
            s[0] = fma(vr, wr, s[0]);
            s[0] = fma(vi, wi, s[0]);
            s[NC - 1] = fma(vr, wi, s[NC - 1]);
            s[NC - 1] = fma(-vi, wr, s[NC - 1]);
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

}  // namespace bsm
