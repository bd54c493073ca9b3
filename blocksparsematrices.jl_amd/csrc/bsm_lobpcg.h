// bsm_lobpcg.h -- what bsm_lobpcg.hip (the kernels), bsm_lobpcg.cpp (bsm_block_gram, bsm_block_combine, bsm_lobpcg_*, the test
// hooks bsm_debug_lobpcg_rr / bsm_debug_eig_jacobi_h; include/bsm_rocm.h) and tools/lobpcg_host_check.cpp share: the geometry of
// the two tall-skinny products, the launch interface, and the small dense side of LOBPCG in plain C++ on doubles / complex
// doubles -- the cyclic Hermitian Jacobi eigensolver (eig_jacobi's complex sibling) and the Rayleigh-Ritz step of one
// iteration (lob_rr).
// (No counterpart in the reference: its operators are LinearMaps handed to a Julia eigensolver package.)
#pragma once
#include <algorithm>
#include <cmath>
#include <complex>
#include <cstdint>
#include <vector>

#include "bsm_eig.h"

namespace bsm {

constexpr int kGramMaxP = 48, kGramMaxQ = 96;  // columns of U / of W in one bsm_block_gram; bsm_block_combine: p <= kGramMaxP
constexpr int kGramThreads = 256;
// rows a workgroup of the Gram stages per pass through LDS, by the bytes of a REAL of the type and its components: the
// (p + q) columns of such a chunk, padded by 4 rows, stay below 48 KiB in every type
constexpr int gram_chunk_rows(int rs, int nc) { return rs == 4 ? (nc == 1 ? 64 : 32) : (nc == 1 ? 32 : 16); }
// elements of the row tile of the complex bsm_block_combine: whole waves of rows of p columns in 128 KiB of LDS, at most 512
inline int block_combine_tile_complex(long long p, int es) {
    long long rows = kEigLdsBytes / (std::max<long long>(p, 1) * es) / 64 * 64;
    return (int)std::min<long long>(rows, 512);
}

// ---- the Hermitian eigen-decomposition --------------------------------------------------------------------------------------
inline double lob_re(double a) { return a; }
inline double lob_re(const std::complex<double> &a) { return a.real(); }
inline double lob_conj(double a) { return a; }
inline std::complex<double> lob_conj(const std::complex<double> &a) { return std::conj(a); }
inline double lob_abs(double a) { return std::fabs(a); }
inline double lob_abs(const std::complex<double> &a) { return std::hypot(a.real(), a.imag()); }
inline bool lob_finite(double a) { return std::isfinite(a); }
inline bool lob_finite(const std::complex<double> &a) { return std::isfinite(a.real()) && std::isfinite(a.imag()); }

// Cyclic Jacobi on the Hermitian A (m x m, column-major, leading dimension m; both triangles read, destroyed), T = double or
// std::complex<double>: sweeps over (p, q), p < q, row by row, as eig_jacobi.  With A[p, q] = g w, g = |A[p, q]|, the rotation
// is J = diag(1, conj(w)) [c s; -s c] on the columns (p, q): the phase makes the 2 x 2 block real symmetric, (c, s) are
// eig_jacobi's.  A <- J^H A J, Q <- Q J.  A rotation is skipped -- and the entry set to zero -- when adding g changes neither
// |A[p, p]| nor |A[q, q]|; the method ends with the first sweep that rotates nothing.
// -> theta ascending (stable), Q (m x m, column-major) its orthonormal eigenvectors.  Fixed order: the same input gives the
// same bytes.  Returns the sweeps taken; kEigMaxSweeps means the cap was hit.
template <typename T> inline int eig_jacobi_h(int m, T *A, double *theta, T *Q) {
    auto a = [&](int r, int c) -> T & { return A[(size_t)r + (size_t)c * m]; };
    for (int c = 0; c < m; c++)
        for (int r = 0; r < m; r++) Q[(size_t)r + (size_t)c * m] = r == c ? T(1) : T(0);
    int sweeps = 0;
    for (; sweeps < kEigMaxSweeps; sweeps++) {
        int rotated = 0;
        for (int p = 0; p < m - 1; p++) {
            for (int q = p + 1; q < m; q++) {
                const T apq = a(p, q);
                const double g = lob_abs(apq);
                if (g == 0.0) continue;
                const double app = lob_re(a(p, p)), aqq = lob_re(a(q, q));
                if (std::fabs(app) + g == std::fabs(app) && std::fabs(aqq) + g == std::fabs(aqq)) {
                    a(p, q) = a(q, p) = T(0);
                    continue;
                }
                if (!std::isfinite(g) || !std::isfinite(app) || !std::isfinite(aqq)) continue;  // (the caller reports status 2)
                rotated++;
                const T w = apq / g, wc = lob_conj(w);
                const double tau = (aqq - app) / (2.0 * g);
                const double t = (tau >= 0 ? 1.0 : -1.0) / (std::fabs(tau) + std::sqrt(1.0 + tau * tau));
                const double c = 1.0 / std::sqrt(1.0 + t * t), s = t * c;
                for (int r = 0; r < m; r++) {  // A J
                    const T x = a(r, p), y = wc * a(r, q);
                    a(r, p) = c * x - s * y;
                    a(r, q) = s * x + c * y;
                }
                for (int r = 0; r < m; r++) {  // J^H (A J)
                    const T x = a(p, r), y = w * a(q, r);
                    a(p, r) = c * x - s * y;
                    a(q, r) = s * x + c * y;
                }
                a(p, p) = T(app - t * g);
                a(q, q) = T(aqq + t * g);
                a(p, q) = a(q, p) = T(0);
                T *qp = Q + (size_t)p * m, *qq = Q + (size_t)q * m;
                for (int r = 0; r < m; r++) {
                    const T x = qp[r], y = wc * qq[r];
                    qp[r] = c * x - s * y;
                    qq[r] = s * x + c * y;
                }
            }
        }
        if (!rotated) break;
    }
    std::vector<int> ord((size_t)m);
    for (int i = 0; i < m; i++) ord[i] = i;
    for (int i = 1; i < m; i++) {
        const int o = ord[i];
        int k = i;
        for (; k > 0 && lob_re(a(ord[k - 1], ord[k - 1])) > lob_re(a(o, o)); k--) ord[k] = ord[k - 1];
        ord[k] = o;
    }
    std::vector<T> tmp((size_t)m * m);
    for (int i = 0; i < m; i++) {
        theta[i] = lob_re(a(ord[i], ord[i]));
        std::copy(Q + (size_t)ord[i] * m, Q + (size_t)(ord[i] + 1) * m, tmp.begin() + (size_t)i * m);
    }
    std::copy(tmp.begin(), tmp.end(), Q);
    return sweeps;
}

// ---- the Rayleigh-Ritz step of one iteration --------------------------------------------------------------------------------
// GB = S^H S, GA = S^H A S (p x p, column-major, leading dimensions ldb / lda), `use`: p flags, the basis columns in use (m of
// them).  On those: both symmetrised, scaled by d_i = 1 / sqrt(GB[i, i]); the scaled GB = Q Lambda Q^H by eig_jacobi_h; the
// directions with lambda > tau lambda_max are kept (the others counted in drops); L = Q_kept Lambda^{-1/2};
// L^H GA L = Z Mu Z^H by eig_jacobi_h; the k extreme Ritz values of `which` (kEigSA: smallest first, kEigLA: largest first)
// -> theta[0 .. k), C = diag(d) L Z_sel (p x k, leading dimension p, zero rows for columns not in use); mu_abs = max |Mu|.
// Returns the status of the solve: 0;  2: an entry or a Ritz value is not finite, or Jacobi hit its sweep cap;  3: a GB[i, i]
// that is not positive, or fewer than k directions kept.  theta, C, mu_abs are written with status 0 only.
template <typename T>
inline int lob_rr(int p, int k, int which, const T *GB, long long ldb, const T *GA, long long lda, const unsigned char *use, double tau,
                  double *theta, T *C, int *drops, double *mu_abs) {
    std::vector<int> at;
    for (int i = 0; i < p; i++)
        if (use[i]) at.push_back(i);
    const int m = (int)at.size();
    *drops = 0;
    if (m < k) return 3;
    std::vector<T> B((size_t)m * m), A((size_t)m * m), Q((size_t)m * m);
    std::vector<double> d((size_t)m), lam((size_t)m);
    for (int j = 0; j < m; j++)
        for (int i = 0; i < m; i++) {
            const T b = (GB[at[i] + at[j] * ldb] + lob_conj(GB[at[j] + at[i] * ldb])) * 0.5;
            const T a = (GA[at[i] + at[j] * lda] + lob_conj(GA[at[j] + at[i] * lda])) * 0.5;
            if (!lob_finite(b) || !lob_finite(a)) return 2;
            B[(size_t)i + (size_t)j * m] = b;
            A[(size_t)i + (size_t)j * m] = a;
        }
    for (int i = 0; i < m; i++) {
        const double bii = lob_re(B[(size_t)i + (size_t)i * m]);
        if (!(bii > 0)) return 3;
        d[i] = 1.0 / std::sqrt(bii);
    }
    for (int j = 0; j < m; j++)
        for (int i = 0; i < m; i++) {
            B[(size_t)i + (size_t)j * m] *= d[i] * d[j];
            A[(size_t)i + (size_t)j * m] *= d[i] * d[j];
        }
    if (eig_jacobi_h(m, B.data(), lam.data(), Q.data()) >= kEigMaxSweeps) return 2;
    for (int i = 0; i < m; i++)
        if (!std::isfinite(lam[i])) return 2;
    const double cut = tau * lam[m - 1];
    int first = 0;  // lam ascending: the kept directions are first .. m - 1
    while (first < m && !(lam[first] > cut)) first++;
    const int r = m - first;
    *drops = first;
    if (r < k) return 3;
    // L = Q[:, first:] Lambda^{-1/2}  (m x r)
    std::vector<T> L((size_t)m * r), AL((size_t)m * r), H((size_t)r * r), Z((size_t)r * r);
    for (int l = 0; l < r; l++) {
        const double s = 1.0 / std::sqrt(lam[first + l]);
        for (int i = 0; i < m; i++) L[(size_t)i + (size_t)l * m] = Q[(size_t)i + (size_t)(first + l) * m] * s;
    }
    for (int l = 0; l < r; l++)
        for (int i = 0; i < m; i++) {
            T s = T(0);
            for (int j = 0; j < m; j++) s += A[(size_t)i + (size_t)j * m] * L[(size_t)j + (size_t)l * m];
            AL[(size_t)i + (size_t)l * m] = s;
        }
    for (int l = 0; l < r; l++)
        for (int e = 0; e <= l; e++) {
            T s = T(0);
            for (int i = 0; i < m; i++) s += lob_conj(L[(size_t)i + (size_t)e * m]) * AL[(size_t)i + (size_t)l * m];
            H[(size_t)e + (size_t)l * r] = s;
        }
    for (int l = 0; l < r; l++) {  // Hermitian from the upper triangle, real diagonal
        H[(size_t)l + (size_t)l * r] = T(lob_re(H[(size_t)l + (size_t)l * r]));
        for (int e = 0; e < l; e++) H[(size_t)l + (size_t)e * r] = lob_conj(H[(size_t)e + (size_t)l * r]);
    }
    std::vector<double> mu((size_t)r);
    if (eig_jacobi_h(r, H.data(), mu.data(), Z.data()) >= kEigMaxSweeps) return 2;
    double big = 0;
    for (int i = 0; i < r; i++) {
        if (!std::isfinite(mu[i])) return 2;
        big = std::max(big, std::fabs(mu[i]));
    }
    *mu_abs = big;
    for (size_t i = 0; i < (size_t)p * k; i++) C[i] = T(0);
    for (int c = 0; c < k; c++) {
        const int sel = which == kEigLA ? r - 1 - c : c;
        theta[c] = mu[sel];
        for (int i = 0; i < m; i++) {
            T s = T(0);
            for (int l = 0; l < r; l++) s += L[(size_t)i + (size_t)l * m] * Z[(size_t)l + (size_t)sel * r];
            C[(size_t)at[i] + (size_t)c * p] = s * d[i];
        }
    }
    return 0;
}

#if defined(__HIPCC__) || defined(BSM_KRYLOV_LAUNCH)
// ---- launch interface (bsm_lobpcg.hip); everything enqueues on `stream` and returns -----------------------------------------
// workgroups of the first launch of the Gram: krylov_grid, one per 8192 bytes of a column
inline int gram_grid(int dtype, long long n) { return krylov_grid(n, elem_bytes(dtype)); }
// part[g] (p x q elements of dtype, column-major, leading dimension p) = workgroup g's share of U^H W;  then
// G[i, j] = the sum of the shares over g ascending, in double (G: p x q of the wide type, leading dimension ldg)
hipError_t launch_block_gram(int dtype, long long n, int p, const void *U, long long ldu, int q, const void *W, long long ldw, void *G,
                             long long ldg, void *part, hipStream_t stream);
// Out[:, c] = sum_{j < p} V[:, j] C[j, c], c < q, complex types, C complex (p x q, leading dimension ldc)
hipError_t launch_block_combine_complex(int dtype, long long n, int p, int q, const void *V, long long ldv, const void *C, long long ldc,
                                        void *Out, long long ldo, hipStream_t stream);
// R[:, c] = AX[:, c] - theta[c] X[:, c], c < k (R may be neither);  part[c * G + g] = workgroup g's share of ||R[:, c]||^2;  then
// res[c] = the root of their sum in a fixed order, as a double (one wave per column).  theta: k reals of dtype's real type.
hipError_t launch_lob_resid(int dtype, long long n, int k, const void *AX, long long ldax, const void *X, long long ldx, const void *theta,
                            void *R, long long ldr, void *part, double *res, hipStream_t stream);
#endif

}  // namespace bsm
