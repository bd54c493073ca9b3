// bsm_krylov.h -- what bsm_krylov.hip (the kernels of bsm_krylov_orth), bsm_krylov.cpp (bsm_krylov_orth; include/bsm_rocm.h),
// the kernels of the GMRES solvers (bsm_gmres_multi.hip) and tools/krylov_host_check.cpp share: the launch interface of the
// Gram-Schmidt pass, and the small dense arithmetic of restarted GMRES -- Givens rotations of one Hessenberg column, back
// substitution -- in plain C++, compiled for the host (bsm_debug_krylov_lsq_host, the tests' and the sanitizer run's form) and
// for the one-wave kernels of bsm_gmres_multi.hip alike.
// (No counterpart in the reference: its operators are LinearMaps handed to a Julia solver package.)
//
// Everything works on REAL components: an element is NC = 1 (real) or NC = 2 (re, im) values of R = float / double.
//
// The rotation.  Column j of the Hessenberg matrix arrives as (h[0 .. j], hn) with hn = ||w|| >= 0 REAL (the norm left by
// the orthogonalisation).  After the j stored rotations have been applied to h, rotation j is formed from a = h[j], b = hn:
//     t = |a| = hypot(re a, im a),   r = hypot(t, b),
//     c = t / r  (real),   s = (a / t) * b / r  (complex: the phase of a),        a == 0:  c = 0, s = 1  (also when b == 0: a
//     column that is zero from the diagonal down leaves the estimate where it was, and the back substitution skips it)
// and applied as   [ c        s ] [x]   so that  (a, b) -> ((a / t) r, 0),   g[j + 1] = -conj(s) g[j],  g[j] = c g[j].
//                  [ -conj(s) c ] [y]
// Both c and s are scaled by the hypot, never by a sum of squares: no overflow below the range of R.
#pragma once
#include <cmath>
#include <cstdint>

#include "bsm_types.h"

#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#define BSM_HD __host__ __device__ inline
#else
#define BSM_HD inline
#endif

#ifndef BSM_GMRES_MAX_RESTART
#define BSM_GMRES_MAX_RESTART 128
#endif

namespace bsm {

BSM_HD float k_hypot(float a, float b) { return ::hypotf(a, b); }
BSM_HD double k_hypot(double a, double b) { return ::hypot(a, b); }
BSM_HD float k_abs(float a) { return ::fabsf(a); }
BSM_HD double k_abs(double a) { return ::fabs(a); }

// |a| of one element
template <typename R, int NC> BSM_HD R k_mag(const R *a) {
    if (NC == 1) return k_abs(a[0]);
    return k_hypot(a[0], a[NC - 1]);
}

// Applies the j stored rotations (cs[i] real, sn[i * NC ..] complex) to the column col[0 .. j] (elements), forms rotation
// j from (col[j], hn), applies it to the column and to g (g[j], g[j + 1]) and returns |g[j + 1]|, the residual estimate.
// col is left holding column j of R (upper triangular).
template <typename R, int NC> BSM_HD R krylov_hess_column(int j, R *col, R hn, R *cs, R *sn, R *g) {
    for (int i = 0; i < j; ++i) {
        const R c = cs[i];
        R *x = col + (long long)i * NC, *y = x + NC;
        const R *s = sn + (long long)i * NC;
        if (NC == 1) {
            const R a = x[0], b = y[0];
            x[0] = c * a + s[0] * b;
            y[0] = c * b - s[0] * a;
        } else {
            const R ar = x[0], ai = x[NC - 1], br = y[0], bi = y[NC - 1], sr = s[0], si = s[NC - 1];
            x[0] = c * ar + (sr * br - si * bi);
            x[NC - 1] = c * ai + (sr * bi + si * br);
            // -conj(s) a + c b
            y[0] = c * br - (sr * ar + si * ai);
            y[NC - 1] = c * bi - (sr * ai - si * ar);
        }
    }
    R *a = col + (long long)j * NC, *s = sn + (long long)j * NC;
    const R t = k_mag<R, NC>(a);
    const R r = k_hypot(t, hn);
    R c;
    if (t == R(0)) {
        c = R(0);
        s[0] = R(1);
        if (NC == 2) s[NC - 1] = R(0);
        a[0] = hn;
        if (NC == 2) a[NC - 1] = R(0);
    } else {
        c = t / r;
        const R f = hn / r;
        const R pr = a[0] / t, pi = NC == 2 ? a[NC - 1] / t : R(0);
        s[0] = pr * f;
        if (NC == 2) s[NC - 1] = pi * f;
        a[0] = pr * r;
        if (NC == 2) a[NC - 1] = pi * r;
    }
    cs[j] = c;
    R *gj = g + (long long)j * NC, *gn = gj + NC;
    if (NC == 1) {
        gn[0] = -s[0] * gj[0];
        gj[0] = c * gj[0];
    } else {
        const R gr = gj[0], gi = gj[NC - 1], sr = s[0], si = s[NC - 1];
        gn[0] = -(sr * gr + si * gi);
        gn[NC - 1] = -(sr * gi - si * gr);
        gj[0] = c * gr;
        gj[NC - 1] = c * gi;
    }
    return k_mag<R, NC>(gn);
}

// q = x / d for one element; complex: on operands scaled by |re d| + |im d|.  d == 0 gives 0 (a column the lucky
// breakdown left empty contributes nothing; no NaN leaves a solve)
template <typename R, int NC> BSM_HD void k_div(const R *x, const R *d, R *q) {
    if (NC == 1) {
        q[0] = d[0] == R(0) ? R(0) : x[0] / d[0];
        return;
    }
    const R sc = k_abs(d[0]) + k_abs(d[NC - 1]);
    if (sc == R(0)) {
        q[0] = q[NC - 1] = R(0);
        return;
    }
    const R a = x[0] / sc, b = x[NC - 1] / sc, c = d[0] / sc, e = d[NC - 1] / sc;
    const R den = c * c + e * e;
    q[0] = (a * c + b * e) / den;
    q[NC - 1] = (b * c - a * e) / den;
}

// Back substitution R y = g[0 .. k) on the rotated Hessenberg matrix Hm (column-major, leading dimension ldh elements),
// serially: the host form.  (The kernel spreads the column update of every step over the lanes of its wave.)
template <typename R, int NC> inline void krylov_trsolve_host(int k, const R *Hm, long long ldh, const R *g, R *y) {
    for (int i = 0; i < k * NC; ++i) y[i] = g[i];
    for (int i = k - 1; i >= 0; --i) {
        R q[2] = {R(0), R(0)};
        k_div<R, NC>(y + (long long)i * NC, Hm + ((long long)i + i * ldh) * NC, q);
        for (int c = 0; c < NC; ++c) y[(long long)i * NC + c] = q[c];
        for (int r = 0; r < i; ++r) {
            const R *a = Hm + ((long long)r + i * ldh) * NC;
            R *t = y + (long long)r * NC;
            if (NC == 1) {
                t[0] -= a[0] * q[0];
            } else {
                t[0] -= a[0] * q[0] - a[NC - 1] * q[NC - 1];
                t[NC - 1] -= a[0] * q[NC - 1] + a[NC - 1] * q[0];
            }
        }
    }
}

// min || beta e_1 - H y || for a (k + 1) x k upper Hessenberg H whose subdiagonal is real and >= 0, by the rotations and
// the back substitution above, column by column as the solver does: H (ldh >= k + 1 elements) is overwritten by R,
// y[0 .. k), res[j] = the estimate after column j.  work: (3 k + 1) elements (cs, sn, g).
template <typename R, int NC> inline void krylov_lsq_host(int k, R *H, long long ldh, R beta, R *y, double *res, R *work) {
    R *cs = work, *sn = cs + (long long)k * NC, *g = sn + (long long)k * NC;
    for (int i = 0; i < (k + 1) * NC; ++i) g[i] = R(0);
    g[0] = beta;
    for (int j = 0; j < k; ++j) {
        R *col = H + (long long)j * ldh * NC;
        const R hn = col[(long long)(j + 1) * NC];
        res[j] = (double)krylov_hess_column<R, NC>(j, col, hn, cs, sn, g);
        col[(long long)(j + 1) * NC] = R(0);
        if (NC == 2) col[(long long)(j + 1) * NC + 1] = R(0);
    }
    krylov_trsolve_host<R, NC>(k, H, ldh, g, y);
}

#if defined(__HIPCC__) || defined(BSM_KRYLOV_LAUNCH)
// ---- launch interface (bsm_krylov.hip); dtype BSM_F32 .. BSM_C128; everything enqueues on `stream` and returns ----
// workgroups of every sweep over a vector of n elements of `es` bytes: one per 512 sixteen-byte groups, at most
// kKrylovMaxGrid, at least 1 -- a vector of 400 entries is one workgroup
constexpr int kKrylovMaxGrid = 256;
inline int krylov_grid(long long n, int es) {
    const long long per = 512LL * (16 / es);
    const long long g = (n + per - 1) / per;
    return (int)(g < 1 ? 1 : g > kKrylovMaxGrid ? kKrylovMaxGrid : g);
}
// part[c * G + wg] = the workgroup's share of V[:, c]^H w, c < k (G = krylov_grid)
hipError_t launch_krylov_dot(int dtype, long long n, int k, const void *V, long long ldv, const void *w, void *part,
                             hipStream_t stream);
// w -= V[:, 0:k] h,  h[c] = the sum of part[c * G + 0 .. G) in a fixed order (every workgroup forms the same h);
// hsum[0:k] += h (workgroup 0; may be null);  nrmpart[wg] = the workgroup's share of ||w||^2 (may be null).  k == 0: the norm alone.
hipError_t launch_krylov_update(int dtype, long long n, int k, const void *V, long long ldv, void *w, const void *part, void *hsum,
                                void *nrmpart, hipStream_t stream);
// nrm[0] = sqrt(sum of nrmpart[0 .. G)), one real, summed in a fixed order by one wave
hipError_t launch_krylov_norm(int dtype, int G, const void *nrmpart, void *nrm, hipStream_t stream);
#endif

}  // namespace bsm
