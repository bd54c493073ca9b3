// bsm_eig.h -- what bsm_eig.hip (the kernels), bsm_eig.cpp (bsm_krylov_combine, bsm_eigsh_*, the test hooks bsm_debug_eig_*;
// include/bsm_rocm.h) and tools/eig_host_check.cpp share: the tile of the basis compression, the launch interface, and the
// small dense side of thick-restart Lanczos in plain C++ on doubles -- the cyclic Jacobi eigensolver of the projected
// matrix, the selection of Ritz pairs, and the bookkeeping of one cycle (EigProjected).
// (No counterpart in the reference: its operators are LinearMaps handed to KrylovKit's eigsolve.)
#pragma once
#include <algorithm>
#include <cmath>
#include <cstdint>
#include <vector>

#include "bsm_krylov.h"

namespace bsm {

// ---- the tile of bsm_krylov_combine ---------------------------------------------------------------------------------------
// A workgroup stages `rows` REAL rows of the m columns in LDS (a complex column is 2 n reals): as many whole waves of rows as
// fit into kEigLdsBytes (the budget of bsm_invert.hip: 128 KiB of the CU's 160 KiB), at most kEigMaxTileRows.  m <= 128
// leaves at least 128 rows of doubles.
constexpr int kEigLdsBytes = 131072;
constexpr int kEigMaxTileRows = 1024;
constexpr int kEigThreads = 256;
inline int combine_tile_reals(long long m, int rs) {
    long long rows = kEigLdsBytes / (std::max<long long>(m, 1) * rs) / 64 * 64;
    return (int)std::min<long long>(rows, kEigMaxTileRows);
}

// ---- selection ------------------------------------------------------------------------------------------------------------
enum { kEigLA = 0, kEigSA = 1, kEigBE = 2, kEigLM = 3 };

// The `count` Ritz values of theta[0 .. m) (ASCENDING) that `which` wants, in the order it reports them:
//   LA  the largest, largest first;   SA  the smallest, smallest first;
//   BE  ceil(count / 2) from the top, largest first, then the rest from the bottom, smallest first;
//   LM  the largest |theta|, largest first; of two equal magnitudes the positive one first.
inline void eig_select(int which, int m, const double *theta, int count, int *idx) {
    count = std::min(count, m);
    if (which == kEigLA) {
        for (int i = 0; i < count; i++) idx[i] = m - 1 - i;
    } else if (which == kEigSA) {
        for (int i = 0; i < count; i++) idx[i] = i;
    } else if (which == kEigBE) {
        const int top = (count + 1) / 2;
        for (int i = 0; i < top; i++) idx[i] = m - 1 - i;
        for (int i = top; i < count; i++) idx[i] = i - top;
    } else {
        // ascending values: the largest magnitude is at one of the two ends
        int lo = 0, hi = m - 1;
        for (int i = 0; i < count; i++) idx[i] = std::fabs(theta[hi]) >= std::fabs(theta[lo]) ? hi-- : lo++;
    }
}
// Ritz pairs a restart keeps
inline int eig_keep(int nev, int ncv) { return std::min(ncv - 1, nev + (ncv - nev) / 2); }

// ---- the eigen-decomposition of the projected matrix ----------------------------------------------------------------------
// Cyclic Jacobi on the real symmetric T (m x m, column-major, leading dimension m; both triangles read, destroyed):
// sweeps over (p, q), p < q, row by row; a rotation is skipped -- and the entry set to zero -- when adding |T[p, q]| changes
// neither |T[p, p]| nor |T[q, q]|; the method ends with the first sweep that rotates nothing (at most kEigMaxSweeps).
// -> theta ascending, S (m x m, column-major) its orthonormal eigenvectors.  Fixed order, no data-dependent shortcut
// besides the skip: the same input gives the same bytes.  Returns the sweeps taken.
constexpr int kEigMaxSweeps = 60;
inline int eig_jacobi(int m, double *T, double *theta, double *S) {
    auto a = [&](int r, int c) -> double & { return T[(size_t)r + (size_t)c * m]; };
    for (int c = 0; c < m; c++)
        for (int r = 0; r < m; r++) S[(size_t)r + (size_t)c * m] = r == c ? 1.0 : 0.0;
    int sweeps = 0;
    for (; sweeps < kEigMaxSweeps; sweeps++) {
        int rotated = 0;
        for (int p = 0; p < m - 1; p++) {
            for (int q = p + 1; q < m; q++) {
                const double apq = a(p, q);
                if (apq == 0.0) continue;
                const double app = a(p, p), aqq = a(q, q), g = std::fabs(apq);
                if (std::fabs(app) + g == std::fabs(app) && std::fabs(aqq) + g == std::fabs(aqq)) {
                    a(p, q) = a(q, p) = 0.0;
                    continue;
                }
                if (!std::isfinite(apq) || !std::isfinite(app) || !std::isfinite(aqq)) continue;  // (the caller reports status 2)
                rotated++;
                const double tau = (aqq - app) / (2.0 * apq);
                const double t = (tau >= 0 ? 1.0 : -1.0) / (std::fabs(tau) + std::sqrt(1.0 + tau * tau));
                const double c = 1.0 / std::sqrt(1.0 + t * t), s = t * c;
                a(p, p) = app - t * apq;
                a(q, q) = aqq + t * apq;
                a(p, q) = a(q, p) = 0.0;
                for (int r = 0; r < m; r++) {
                    if (r == p || r == q) continue;
                    const double arp = a(r, p), arq = a(r, q);
                    a(r, p) = a(p, r) = c * arp - s * arq;
                    a(r, q) = a(q, r) = s * arp + c * arq;
                }
                double *sp = S + (size_t)p * m, *sq = S + (size_t)q * m;
                for (int r = 0; r < m; r++) {
                    const double x = sp[r], y = sq[r];
                    sp[r] = c * x - s * y;
                    sq[r] = s * x + c * y;
                }
            }
        }
        if (!rotated) break;
    }
    // ascending, by a stable insertion sort of the column order
    std::vector<int> ord((size_t)m);
    for (int i = 0; i < m; i++) ord[i] = i;
    for (int i = 1; i < m; i++) {
        const int o = ord[i];
        int k = i;
        for (; k > 0 && a(ord[k - 1], ord[k - 1]) > a(o, o); k--) ord[k] = ord[k - 1];
        ord[k] = o;
    }
    std::vector<double> tmp((size_t)m * m);
    for (int i = 0; i < m; i++) {
        theta[i] = a(ord[i], ord[i]);
        std::copy(S + (size_t)ord[i] * m, S + (size_t)(ord[i] + 1) * m, tmp.begin() + (size_t)i * m);
    }
    std::copy(tmp.begin(), tmp.end(), S);
    return sweeps;
}

// ---- the projected matrix of one solve ------------------------------------------------------------------------------------
// T after a cycle of a thick-restart Lanczos run: the leading keep x keep part is diag(kept theta) with the arrow row
// beta_m S[m - 1, i] (taken analytically from the cycle before), the columns start .. d - 1 take alpha_j = Re H[j, j] on the
// diagonal and beta_j beside it.  d: the dimension the cycle reached -- ncv, or j + 1 for the first step j whose beta_j is
// exactly zero (the Krylov space ended).
struct EigProjected {
    int ncv = 0, start = 0, d = 0;
    double anorm = 0;
    std::vector<double> kept, arrow;      // start entries each
    std::vector<double> T, S, theta;      // d x d, d x d, d
    bool finite = true;

    void reset(int ncv_) {
        ncv = ncv_, start = 0, d = 0, anorm = 0, finite = true;
        kept.clear(), arrow.clear();
    }
    // alpha[j], beta[j] for j in start .. ncv - 1 (entries below start are not read)
    void cycle(const double *alpha, const double *beta) {
        d = ncv;
        for (int j = start; j < ncv; j++)
            if (beta[j] == 0.0) {
                d = j + 1;
                break;
            }
        finite = true;
        for (int j = start; j < d; j++) finite = finite && std::isfinite(alpha[j]) && std::isfinite(beta[j]);
        T.assign((size_t)d * d, 0.0);
        S.assign((size_t)d * d, 0.0);
        theta.assign((size_t)d, 0.0);
        if (d == 0 || !finite) return;
        auto t = [&](int r, int c) -> double & { return T[(size_t)r + (size_t)c * d]; };
        for (int i = 0; i < start; i++) {
            t(i, i) = kept[i];
            t(i, start) = t(start, i) = arrow[i];
        }
        for (int j = start; j < d; j++) {
            t(j, j) = alpha[j];
            if (j + 1 < d) t(j, j + 1) = t(j + 1, j) = beta[j];
        }
        std::vector<double> work(T);
        eig_jacobi(d, work.data(), theta.data(), S.data());
        for (int i = 0; i < d; i++) {
            finite = finite && std::isfinite(theta[i]);
            if (std::isfinite(theta[i])) anorm = std::max(anorm, std::fabs(theta[i]));
        }
    }
    // |beta_m S[d - 1, i]|, the residual estimate of Ritz pair i (beta_m: the last beta of the cycle)
    double estimate(int i, double beta_m) const { return std::fabs(beta_m * S[(size_t)(d - 1) + (size_t)i * d]); }
    // The columns idx[0 .. k) of S made orthonormal to working precision, in that order: two modified Gram-Schmidt passes
    // and a normalisation each.  The Jacobi rotations leave S orthonormal to about d eps only, and V S inherits that; the
    // columns that go to the device -- the kept ones of a restart, the wanted ones at the end -- pass through here first.
    void orthonormalise(const int *idx, int k) {
        for (int c = 0; c < k; c++) {
            double *x = S.data() + (size_t)idx[c] * d;
            for (int pass = 0; pass < 2; pass++)
                for (int p = 0; p < c; p++) {
                    const double *y = S.data() + (size_t)idx[p] * d;
                    double h = 0;
                    for (int r = 0; r < d; r++) h += y[r] * x[r];
                    for (int r = 0; r < d; r++) x[r] -= h * y[r];
                }
            double s = 0;
            for (int r = 0; r < d; r++) s += x[r] * x[r];
            s = std::sqrt(s);
            if (s > 0 && std::isfinite(s))
                for (int r = 0; r < d; r++) x[r] /= s;
        }
    }
    // the restart on the Ritz pairs idx[0 .. keep): the next cycle starts at column keep
    void restart(const int *idx, int keep, double beta_m) {
        kept.resize((size_t)keep), arrow.resize((size_t)keep);
        for (int i = 0; i < keep; i++) {
            kept[i] = theta[idx[i]];
            arrow[i] = beta_m * S[(size_t)(d - 1) + (size_t)idx[i] * d];
        }
        start = keep;
    }
};

#if defined(__HIPCC__) || defined(BSM_KRYLOV_LAUNCH)
// ---- launch interface (bsm_eig.hip); everything enqueues on `stream` and returns ------------------------------------------
// Out[:, c] = sum_{j < m} V[:, j] S[j, c], c < k, j ascending, one fma per term;  carry >= 0: Out[:, k] = V[:, carry].
// S: real m x k (leading dimension lds) of the real type of dtype.  Out == V with ldo == ldv works in place.
hipError_t launch_eig_combine(int dtype, long long n, int m, int k, const void *V, long long ldv, const void *S, long long lds, void *Out,
                              long long ldo, int carry, hipStream_t stream);
// w[0 .. n) *= 1 / nrm[0]; nrm[0] zero or not finite: w = 0 and nothing is divided
hipError_t launch_eig_scale(int dtype, long long n, void *w, const void *nrm, hipStream_t stream);
// pack[j] = Re H[j, j], pack[m + j] = beta[j], j < m, pack[2 m] = beta[m] (where the solver keeps ||v0||), as doubles (one wave)
hipError_t launch_eig_pack(int dtype, int m, const void *H, const void *beta, double *pack, hipStream_t stream);
// part[c * G + g] = workgroup g's share of ||Q[:, c] - theta[c] X[:, c]||^2, c < k;  then res[c] = the root of their sum in a
// fixed order, as a double (one wave per column).  theta: k reals of dtype's real type.
hipError_t launch_eig_resid(int dtype, long long n, int k, const void *Q, long long ldq, const void *X, long long ldx, const void *theta,
                            void *part, double *res, hipStream_t stream);
#endif

}  // namespace bsm
