// bsm_krylov_device.h -- the device-side pieces of restarted GMRES that bsm_krylov.hip (one column: bsm_krylov_orth,
// bsm_gmres_solve) and bsm_gmres_multi.hip (several columns in lockstep) share: the update of a Gram-Schmidt tile on the
// elements of one 16-byte group, the fixed-order sum of a pass's partials, and the body of the one-wave back substitution
// around the plain C++ of bsm_krylov.h.  The units differ in how they reach their vectors (guarded groups of any alignment
// there, unguarded groups of padded workspace columns here) and in who decides.  The dot of a tile and the body of the hess
// kernel are shared as statement macros at the end of this file.  For the kernel units only.
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

// y[0 .. k) = R^-1 g[0 .. k) by one wave on the rotated Hessenberg matrix Hm (leading dimension m + 1): lane 0 divides, the
// column update of every step is spread over the lanes.  ys (BSM_GMRES_MAX_RESTART * NC) and q (2) are LDS.
template <typename R, int NC>
__device__ __forceinline__ void trsolve_wave(int m, int k, const R *__restrict__ Hm, const R *__restrict__ g, R *__restrict__ y, R *ys, R *q,
                                             int lane) {
    const long long ldh = m + 1;
    for (int i = lane; i < k * NC; i += 64) ys[i] = g[i];
    __syncthreads();
    for (int i = k - 1; i >= 0; --i) {
        if (lane == 0) {
            R d[2] = {R(0), R(0)};
            k_div<R, NC>(ys + i * NC, Hm + ((long long)i + i * ldh) * NC, d);
            for (int c = 0; c < NC; ++c) q[c] = ys[i * NC + c] = d[c];
        }
        __syncthreads();
        const R qr = q[0], qi = q[NC - 1];
        for (int r = lane; r < i; r += 64) {
            const R *a = Hm + ((long long)r + i * ldh) * NC;
            if (NC == 1) {
                ys[r] -= a[0] * qr;
            } else {
                ys[r * NC] -= a[0] * qr - a[NC - 1] * qi;
                ys[r * NC + NC - 1] -= a[0] * qi + a[NC - 1] * qr;
            }
        }
        __syncthreads();
    }
    for (int i = lane; i < k * NC; i += 64) y[i] = ys[i];
}

// ---- statements both units expand in place.  Macros, not functions: as functions the dot tile and the hess body compiled to
// other register counts in bsm_krylov.hip (docs/experiments_r25.md); an expansion is the very statements that unit had.
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
// Iteration j of a cycle by one wave, in three pieces around what a unit does with the estimate (lane 0, between ROTATE and
// SCATTER).  GATHER: the column hsum[0 .. j] (zeroed behind it), the stored rotations and g[j] into LDS -- col
// ((BSM_GMRES_MAX_RESTART + 1) * NC), rot (BSM_GMRES_MAX_RESTART * 3), gg (2 * NC) --, then a barrier.
#define BSM_HESS_GATHER(R, NC, j, lane, hsum, cs, sn, g, col, rot, gg)                        \
    for (int i = lane; i < (j + 1) * NC; i += 64) {                                          \
        col[i] = hsum[i];                                                                    \
        hsum[i] = R(0);                                                                      \
    }                                                                                        \
    for (int i = lane; i < j; i += 64) rot[i] = cs[i];                                       \
    for (int i = lane; i < j * NC; i += 64) rot[BSM_GMRES_MAX_RESTART + i] = sn[i];          \
    if (lane < NC) gg[lane] = g[j * NC + lane];                                              \
    __syncthreads();
// ROTATE (lane 0): declares est = krylov_hess_column(..) and writes cs[j], sn[j], g[j], g[j + 1]
#define BSM_HESS_ROTATE(R, NC, j, hn, cs, sn, g, col, rot, gg, est)                                                      \
    const R est = krylov_hess_column<R, NC>(j, col, hn, rot, rot + BSM_GMRES_MAX_RESTART, gg - (long long)j * NC);      \
    cs[j] = rot[j];                                                                                                     \
    for (int q = 0; q < NC; ++q) {                                                                                      \
        sn[j * NC + q] = rot[BSM_GMRES_MAX_RESTART + j * NC + q];                                                       \
        g[j * NC + q] = gg[q];                                                                                          \
        g[(j + 1) * NC + q] = gg[NC + q];                                                                               \
    }
// SCATTER: behind a barrier, column j of the rotated Hessenberg matrix Hm (leading dimension m + 1) from col
#define BSM_HESS_SCATTER(R, NC, m, j, lane, Hm, col)                      \
    __syncthreads();                                                     \
    R *const dst = Hm + (long long)j * (m + 1) * NC;                      \
    for (int i = lane; i < (j + 1) * NC; i += 64) dst[i] = col[i];

}  // namespace bsm
