// bsm_eigh.h -- what bsm_eigh.hip (eigh_kernel, spectral_kernel), bsm_eigh.cpp (bsm_eigh_blocks, bsm_spectral_blocks;
// include/bsm_rocm.h) and tools/eigh_host_check.cpp share: the order of the rotations of the batched Hermitian Jacobi
// eigensolver, the arithmetic of one step -- compiled for the host and for the kernel alike, so that both run the same
// sequence of rotations --, the function of the eigenvalues bsm_spectral_blocks applies, the host route of both entries in
// plain C++, and the launch interface.  Depends on the standard library only (the launch interface aside): a stand-alone
// program can include it.
// (No counterpart in the reference: its LinearMap surface offers A[I, J] and leaves factorisations to the caller.)
//
// Everything works on REAL components: an element is NC = 1 (real) or NC = 2 (re, im) values of R = float / double.
//
// The method (include/bsm_rocm.h states it for callers).  H = (B + B^H) / 2, the imaginary part of the diagonal dropped.
// Two-sided Jacobi in the block's own type, round-robin order: m = n rounded up to even, a sweep has m - 1 steps, step
// t = 0 .. m-2 holds the m / 2 disjoint pairs of eigh_pair -- (t, m-1) and ((t + k) mod (m-1), (t - k) mod (m-1)), k = 1 ..
// m/2 - 1, p = min, q = max, a pair with q >= n idles.  Every pair of a step derives its rotation from the entries (p, p),
// (q, q), (p, q) as they stand before the step (eigh_rotation: the rule of eig_jacobi_h, bsm_lobpcg.h); then the column
// phase of every pair runs (A and V: x = col_p, y = conj(omega) col_q, col_p <- c x - s y, col_q <- s x + c y), then the
// row phase of every pair (A: the same with omega on rows p, q), then every pair sets a_pp, a_qq and zeroes a_pq, a_qp:
// J^H (A J) with J the product of the step's commuting rotations.  The method ends with the first sweep that rotates
// nothing; `sweeps` counts the sweeps that rotated, BSM_EIGH_MAX_SWEEPS of them is the cap (info 2).  The eigenvalues are the
// diagonal, sorted ascending by rank_i = #{j : w_j < w_i or (w_j == w_i and j < i)} -- stable --, the columns of V go with them.
#pragma once
#include <cmath>
#include <cstdint>
#include <vector>

#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#endif
#ifndef BSM_HD
#if defined(__HIPCC__)
#define BSM_HD __host__ __device__ inline
#else
#define BSM_HD inline
#endif
#endif

#ifndef BSM_EIGH_LDS_BYTES
#define BSM_EIGH_LDS_BYTES 131072
#define BSM_EIGH_MAX_N 512
#define BSM_EIGH_MAX_SWEEPS 60
#endif

namespace bsm {

enum { kSpecValues = 0, kSpecInv = 1, kSpecAbsInv = 2, kSpecPinv = 3 };  // BSM_SPEC_*

BSM_HD float eh_abs(float a) { return ::fabsf(a); }
BSM_HD double eh_abs(double a) { return ::fabs(a); }
BSM_HD float eh_sqrt(float a) { return ::sqrtf(a); }
BSM_HD double eh_sqrt(double a) { return ::sqrt(a); }
BSM_HD float eh_hypot(float a, float b) { return ::hypotf(a, b); }
BSM_HD double eh_hypot(double a, double b) { return ::hypot(a, b); }
BSM_HD float eh_fma(float a, float b, float c) { return ::fmaf(a, b, c); }
BSM_HD double eh_fma(double a, double b, double c) { return ::fma(a, b, c); }
#if defined(__HIP_DEVICE_COMPILE__)
BSM_HD bool eh_finite(float a) { return isfinite(a); }
BSM_HD bool eh_finite(double a) { return isfinite(a); }
#else
BSM_HD bool eh_finite(float a) { return std::isfinite(a); }
BSM_HD bool eh_finite(double a) { return std::isfinite(a); }
#endif

// pair k = 0 .. m/2 - 1 of step t = 0 .. m-2 of a sweep over m (even) indices: p < q
BSM_HD void eigh_pair(int m, int t, int k, int &p, int &q) {
    int a = t, b = m - 1;
    if (k > 0) {
        a = (t + k) % (m - 1);
        b = (t - k + (m - 1)) % (m - 1);
    }
    p = a < b ? a : b;
    q = a < b ? b : a;
}

// what a pair does in its step.  kind 0: nothing (a_pq is zero, or an entry is not finite);  1: a_pq is negligible beside
// both diagonal entries -- it is set to zero, nothing rotates;  2: the rotation (c, s) with the phase omega = (wre, wim) of
// a_pq, after which the diagonal entries are dpp, dqq
template <typename R> struct EighRot {
    R c, s, wre, wim, dpp, dqq;
    int kind;
};
template <typename R, int NC> BSM_HD EighRot<R> eigh_rotation(R app, R aqq, R are, R aim) {
    EighRot<R> o;
    o.c = R(1), o.s = R(0), o.wre = R(1), o.wim = R(0), o.dpp = app, o.dqq = aqq, o.kind = 0;
    const R g = NC == 1 ? eh_abs(are) : eh_hypot(are, aim);
    if (g == R(0)) return o;
    const R fp = eh_abs(app), fq = eh_abs(aqq);
    const R sp = fp + g, sq = fq + g;
    if (sp == fp && sq == fq) {
        o.kind = 1;
        return o;
    }
    if (!eh_finite(g) || !eh_finite(app) || !eh_finite(aqq)) return o;
    const R tau = (aqq - app) / (R(2) * g);
    const R t = (tau >= R(0) ? R(1) : R(-1)) / (eh_abs(tau) + eh_sqrt(R(1) + tau * tau));
    o.c = R(1) / eh_sqrt(R(1) + t * t);
    o.s = t * o.c;
    o.wre = are / g;
    o.wim = NC == 1 ? R(0) : aim / g;
    o.dpp = app - t * g;
    o.dqq = aqq + t * g;
    o.kind = 2;
    return o;
}

// (x, y) <- (c x - s y', s x + c y') with y' = (wre + i sgn wim) y: sgn = -1 in the column phase (conj(omega)), +1 in the
// row phase.  x, y: NC components each.
template <typename R, int NC> BSM_HD void eigh_apply(R c, R s, R wre, R wim, R sgn, R *x, R *y) {
    if (NC == 1) {
        const R yy = wre * y[0], xx = x[0];
        x[0] = c * xx - s * yy;
        y[0] = s * xx + c * yy;
    } else {
        const R wi = sgn * wim;
        const R yr = wre * y[0] - wi * y[NC - 1], yi = wre * y[NC - 1] + wi * y[0];
        const R xr = x[0], xi = x[NC - 1];
        x[0] = c * xr - s * yr;
        x[NC - 1] = c * xi - s * yi;
        y[0] = s * xr + c * yr;
        y[NC - 1] = s * xi + c * yi;
    }
}

// ---- the function of the eigenvalues (bsm_spectral_blocks) --------------------------------------------------------------------
// wmax = the largest |w_k| over the FINITE w_k (0 when there is none), bound = rcond * wmax (0 when rcond == 0, whatever wmax).
// -> whether f is defined at w;  f = 0 where it is not.
template <typename R> BSM_HD bool spectral_f(int func, R w, R bound, R &f) {
    f = R(0);
    const R a = eh_abs(w);
    switch (func) {
        case kSpecValues: f = w; return true;
        case kSpecInv:
            if (w == R(0) || !eh_finite(w)) return false;
            f = R(1) / w;
            return true;
        case kSpecAbsInv: {
            const R b = a > bound ? a : bound;
            if (!eh_finite(w) || b == R(0) || !eh_finite(b)) return false;
            f = R(1) / b;
            return true;
        }
        default:
            if (!eh_finite(w)) return false;
            f = a > bound ? R(1) / w : R(0);
            return true;
    }
}
template <typename R> BSM_HD R spectral_bound(double rcond, R wmax) { return rcond > 0 ? R(rcond) * wmax : R(0); }

// ---- the host route ---------------------------------------------------------------------------------------------------------
// a: n x n block of NC-component elements, column-major, leading dimension ld elements; w: n reals.  The same rotations as
// eigh_kernel, serially.  -> info (0, 1, 2 as in include/bsm_rocm.h), sweeps.  Writes nothing outside the n x n window and w.
template <typename R, int NC> int eigh_block_host(R *a, int64_t n64, int64_t ld, R *w, bool vectors, int32_t &sweeps) {
    sweeps = 0;
    const int n = (int)n64;
    if (n <= 0) return 0;
    for (int j = 0; j < n; j++)
        for (int i = 0; i < n; i++)
            for (int c = 0; c < NC; c++)
                if (!std::isfinite(a[((int64_t)i + (int64_t)j * ld) * NC + c])) {
                    for (int k = 0; k < n; k++) w[k] = std::nan("");
                    return 1;
                }
    // the working copies: H with leading dimension n, V = I
    std::vector<R> H((size_t)n * n * NC), V(vectors ? (size_t)n * n * NC : 0, R(0));
    auto h = [&](int i, int j) { return H.data() + ((size_t)i + (size_t)j * n) * NC; };
    auto v = [&](int i, int j) { return V.data() + ((size_t)i + (size_t)j * n) * NC; };
    for (int j = 0; j < n; j++)
        for (int i = j; i < n; i++) {
            const R *x = a + ((int64_t)i + (int64_t)j * ld) * NC, *y = a + ((int64_t)j + (int64_t)i * ld) * NC;
            h(i, j)[0] = h(j, i)[0] = (x[0] + y[0]) / R(2);
            if (NC == 2) {
                const R im = i == j ? R(0) : (x[NC - 1] - y[NC - 1]) / R(2);
                h(i, j)[NC - 1] = im;
                h(j, i)[NC - 1] = i == j ? R(0) : -im;
            }
        }
    if (vectors)
        for (int i = 0; i < n; i++) v(i, i)[0] = R(1);
    const int m = (n + 1) & ~1, np = m / 2;
    std::vector<EighRot<R>> rot((size_t)np);
    std::vector<int> P((size_t)np), Q((size_t)np);
    int info = 2;
    while (sweeps < BSM_EIGH_MAX_SWEEPS) {
        int rotated = 0;
        for (int t = 0; t < m - 1; t++) {
            for (int k = 0; k < np; k++) {
                eigh_pair(m, t, k, P[k], Q[k]);
                rot[k].kind = 0;
                if (Q[k] >= n) continue;
                const R *apq = h(P[k], Q[k]);
                rot[k] = eigh_rotation<R, NC>(h(P[k], P[k])[0], h(Q[k], Q[k])[0], apq[0], NC == 2 ? apq[NC - 1] : R(0));
            }
            for (int k = 0; k < np; k++) {  // the column phase of every pair
                if (rot[k].kind != 2) continue;
                const EighRot<R> &r = rot[k];
                for (int i = 0; i < n; i++) {
                    eigh_apply<R, NC>(r.c, r.s, r.wre, r.wim, R(-1), h(i, P[k]), h(i, Q[k]));
                    if (vectors) eigh_apply<R, NC>(r.c, r.s, r.wre, r.wim, R(-1), v(i, P[k]), v(i, Q[k]));
                }
            }
            for (int k = 0; k < np; k++) {  // the row phase of every pair
                if (rot[k].kind != 2) continue;
                const EighRot<R> &r = rot[k];
                for (int j = 0; j < n; j++) eigh_apply<R, NC>(r.c, r.s, r.wre, r.wim, R(1), h(P[k], j), h(Q[k], j));
            }
            for (int k = 0; k < np; k++) {
                if (rot[k].kind == 0) continue;
                for (int c = 0; c < NC; c++) h(P[k], Q[k])[c] = h(Q[k], P[k])[c] = R(0);
                if (rot[k].kind != 2) continue;
                rotated++;
                h(P[k], P[k])[0] = rot[k].dpp, h(Q[k], Q[k])[0] = rot[k].dqq;
                if (NC == 2) h(P[k], P[k])[NC - 1] = h(Q[k], Q[k])[NC - 1] = R(0);
            }
        }
        if (!rotated) {
            info = 0;
            break;
        }
        sweeps++;
    }
    for (int i = 0; i < n; i++) {
        const R wi = h(i, i)[0];
        int rank = 0;
        for (int j = 0; j < n; j++) {
            const R wj = h(j, j)[0];
            rank += (wj < wi || (wj == wi && j < i)) ? 1 : 0;
        }
        w[rank] = wi;
        if (vectors)
            for (int r = 0; r < n; r++)
                for (int c = 0; c < NC; c++) a[((int64_t)r + (int64_t)rank * ld) * NC + c] = v(r, i)[c];
    }
    return info;
}

// out = V diag(f(w)) V^H of one block: out[i, j] = sum_k f_k V[i, k] conj(V[j, k]), k ascending, fused multiply-adds, computed
// for i >= j and mirrored.  -> 0, or the 1-based index of the first w_k at which f is undefined (out is then not written).
template <typename R, int NC>
int64_t spectral_block_host(const R *V, int64_t n64, int64_t ldv, const R *w, int func, double rcond, R *out, int64_t ldo) {
    const int n = (int)n64;
    if (n <= 0) return 0;
    R wmax = R(0);
    for (int k = 0; k < n; k++)
        if (std::isfinite(w[k]) && std::fabs(w[k]) > wmax) wmax = std::fabs(w[k]);
    const R bound = spectral_bound<R>(rcond, wmax);
    std::vector<R> f((size_t)n);
    for (int k = 0; k < n; k++)
        if (!spectral_f<R>(func, w[k], bound, f[k])) return k + 1;
    for (int j = 0; j < n; j++)
        for (int i = j; i < n; i++) {
            R re = R(0), im = R(0);
            for (int k = 0; k < n; k++) {
                const R *vi = V + ((int64_t)i + (int64_t)k * ldv) * NC, *vj = V + ((int64_t)j + (int64_t)k * ldv) * NC;
                const R tr = f[k] * vi[0];
                re = eh_fma(tr, vj[0], re);
                if (NC == 2) {
                    const R ti = f[k] * vi[NC - 1];
                    re = eh_fma(ti, vj[NC - 1], re);
                    im = eh_fma(ti, vj[0], im);
                    im = eh_fma(-tr, vj[NC - 1], im);
                }
            }
            R *o = out + ((int64_t)i + (int64_t)j * ldo) * NC, *ot = out + ((int64_t)j + (int64_t)i * ldo) * NC;
            o[0] = ot[0] = re;
            if (NC == 2) {
                o[NC - 1] = i == j ? R(0) : im;
                ot[NC - 1] = i == j ? R(0) : -im;
            }
        }
    return 0;
}

// ---- the device side --------------------------------------------------------------------------------------------------------
// one record per non-empty block, sorted by descending order
struct EighBlock {
    uint64_t ptr;   // the block (eigh) / V (spectral)
    uint64_t w;     // its eigenvalues, n reals
    uint64_t aux;   // eigh: n x n elements of scratch for V, leading dimension n (larger blocks only, else 0); spectral: out
    long long ld;   // leading dimension of ptr, elements
    long long ld2;  // spectral: leading dimension of out
    int n, id;      // order; position in the launch's info array
};
static_assert(sizeof(EighBlock) == 48, "EighBlock must be 48 bytes");

// the leading dimension of A and V of a resident block in LDS: odd, so that the stride of the row phase -- ld elements of 1, 2
// or 4 dwords -- puts consecutive columns into different banks (docs/experiments_r38.md)
BSM_HD int eigh_ld(int n) { return n | 1; }
BSM_HD bool eigh_resident(long long n, int es) { return 2 * n * n * es <= (long long)BSM_EIGH_LDS_BYTES; }
BSM_HD bool spectral_staged(long long n, int es) { return n * n * es <= (long long)BSM_EIGH_LDS_BYTES; }
// byte offsets into the dynamic LDS of an eigh launch whose largest block has order nmax (es / rs: bytes of an element / of a
// real): 64 bytes of counters, one rotation record per pair, the diagonal and its ranks, and -- resident launches -- A and V
struct EighLds {
    int rot, wv, rank, mat, total;
};
BSM_HD EighLds eigh_lds(int nmax, int es, int rs, bool resident) {
    const int np = (nmax + 1) / 2;
    EighLds l;
    l.rot = 64;
    l.wv = l.rot + ((np * (6 * rs + 4) + 15) & ~15);
    l.rank = l.wv + ((nmax * rs + 15) & ~15);
    l.mat = l.rank + ((nmax * 4 + 15) & ~15);
    l.total = l.mat + (resident ? 2 * nmax * eigh_ld(nmax) * es : 0);
    return l;
}
// spectral launches: 64 bytes of counters, f (nmax reals), V (nmax x nmax, staged launches)
BSM_HD int spectral_lds(int nmax, int es, int rs, bool staged) {
    return 64 + ((nmax * rs + 15) & ~15) + (staged ? nmax * nmax * es : 0);
}

#if defined(BSM_EIGH_LAUNCH)
// d_table[0 .. count): the blocks of ONE launch, one 256-thread workgroup each, all of one regime and none larger than nmax,
// which sizes the launch's dynamic LDS.  d_info[2 * id] = info, d_info[2 * id + 1] = sweeps (eigh);  d_info[id] = info (spectral).
hipError_t launch_eigh(int dtype, const void *d_table, long long count, int nmax, bool resident, int vectors, void *d_info,
                       hipStream_t stream);
hipError_t launch_spectral(int dtype, const void *d_table, long long count, int nmax, bool staged, int func, double rcond,
                           void *d_info, hipStream_t stream);
#endif

}  // namespace bsm
