// bsm_svds.h -- what bsm_svds.hip (the kernels), bsm_svds.cpp (bsm_svds_*, the test hooks bsm_debug_svds_*; include/bsm_rocm.h)
// and tools/svds_host_check.cpp share: the launch interface, and the small dense side of thick-restart Golub-Kahan-Lanczos
// bidiagonalisation in plain C++ on doubles -- the one-sided (Hestenes) Jacobi SVD of the projected matrix, the selection of
// singular triplets, and the bookkeeping of one cycle (SvdProjected).
// (No counterpart in the reference: its operators are LinearMaps handed to KrylovKit's svdsolve.)
#pragma once
#include <algorithm>
#include <cmath>
#include <cstdint>
#include <limits>
#include <vector>

#include "bsm_eig.h"

namespace bsm {

// ---- selection ------------------------------------------------------------------------------------------------------------
enum { kSvdsLM = 0, kSvdsSM = 1 };

// The `count` singular values of sigma[0 .. m) (DESCENDING) that `which` wants, in the order it reports them:
//   LM  the largest, largest first;   SM  the smallest, smallest first.
inline void svds_select(int which, int m, int count, int *idx) {
    count = std::min(count, m);
    for (int i = 0; i < count; i++) idx[i] = which == kSvdsLM ? i : m - 1 - i;
}
// triplets a restart keeps: the rule of eig_keep
inline int svds_keep(int nsv, int ncv) { return eig_keep(nsv, ncv); }

// ---- the singular value decomposition of the projected matrix -------------------------------------------------------------
// One-sided (Hestenes) Jacobi on the real B (m x m, column-major, leading dimension m; not written):  W = B, Y = I;  sweeps over
// the column pairs (p, q), p < q, row by row; with a = w_p . w_p, b = w_q . w_q, c = w_p . w_q the pair is rotated -- W and Y
// alike -- by the rotation of eig_jacobi for the 2 x 2 matrix [a c; c b], and skipped when |c| <= sqrt(m) eps sqrt(a b) (the
// columns are orthogonal to the accuracy their inner product is computed with) or when one of the two columns has a norm
// <= m eps max_c ||B[:, c]|| (it is zero to the accuracy of the method: its direction is rounding noise no rotation settles);
// the method ends with the first sweep that rotates nothing (at most kSvdsMaxSweeps).  Then sigma_i = ||w_i||, sorted
// DESCENDING by a stable insertion sort, x_i = w_i / sigma_i; a column with sigma_i <= m eps sigma_max has no direction of its
// own: its x_i is completed by Gram-Schmidt from the unit vectors e_0, e_1, .. in index order against every other column.
// -> B Y = X diag(sigma), X and Y (m x m, column-major) orthonormal.  Fixed order, no data-dependent shortcut besides the skip:
// the same input gives the same bytes.  Returns the sweeps taken (kSvdsMaxSweeps: the cap was hit).
constexpr int kSvdsMaxSweeps = 60;
inline int svds_jacobi(int m, const double *B, double *sigma, double *X, double *Y) {
    const double eps = std::numeric_limits<double>::epsilon(), tol = std::sqrt((double)m) * eps;
    std::vector<double> W(B, B + (size_t)m * m);
    double amax = 0;  // the largest squared column norm of B: <= sigma_max^2, so a column skipped for good is completed below
    for (int c = 0; c < m; c++) {
        double s = 0;
        for (int r = 0; r < m; r++) s += W[(size_t)r + (size_t)c * m] * W[(size_t)r + (size_t)c * m];
        if (std::isfinite(s)) amax = std::max(amax, s);
    }
    const double floor2 = (m * eps) * (m * eps) * amax;
    for (int c = 0; c < m; c++)
        for (int r = 0; r < m; r++) Y[(size_t)r + (size_t)c * m] = r == c ? 1.0 : 0.0;
    int sweeps = 0;
    for (; sweeps < kSvdsMaxSweeps; sweeps++) {
        int rotated = 0;
        for (int p = 0; p < m - 1; p++) {
            for (int q = p + 1; q < m; q++) {
                double *wp = W.data() + (size_t)p * m, *wq = W.data() + (size_t)q * m;
                double a = 0, b = 0, c = 0;
                for (int r = 0; r < m; r++) {
                    a += wp[r] * wp[r];
                    b += wq[r] * wq[r];
                    c += wp[r] * wq[r];
                }
                if (c == 0.0 || !std::isfinite(a) || !std::isfinite(b) || !std::isfinite(c)) continue;  // (not finite: the caller reports status 2)
                if (a <= floor2 || b <= floor2) continue;
                if (std::fabs(c) <= tol * std::sqrt(a) * std::sqrt(b)) continue;
                rotated++;
                const double tau = (b - a) / (2.0 * c);
                const double t = (tau >= 0 ? 1.0 : -1.0) / (std::fabs(tau) + std::sqrt(1.0 + tau * tau));
                const double cs = 1.0 / std::sqrt(1.0 + t * t), sn = t * cs;
                for (int r = 0; r < m; r++) {
                    const double x = wp[r], y = wq[r];
                    wp[r] = cs * x - sn * y;
                    wq[r] = sn * x + cs * y;
                }
                double *yp = Y + (size_t)p * m, *yq = Y + (size_t)q * m;
                for (int r = 0; r < m; r++) {
                    const double x = yp[r], y = yq[r];
                    yp[r] = cs * x - sn * y;
                    yq[r] = sn * x + cs * y;
                }
            }
        }
        if (!rotated) break;
    }
    std::vector<double> nrm((size_t)m);
    for (int c = 0; c < m; c++) {
        double s = 0;
        for (int r = 0; r < m; r++) s += W[(size_t)r + (size_t)c * m] * W[(size_t)r + (size_t)c * m];
        nrm[c] = std::sqrt(s);
    }
    // descending, by a stable insertion sort of the column order
    std::vector<int> ord((size_t)m);
    for (int i = 0; i < m; i++) ord[i] = i;
    for (int i = 1; i < m; i++) {
        const int o = ord[i];
        int k = i;
        for (; k > 0 && nrm[ord[k - 1]] < nrm[o]; k--) ord[k] = ord[k - 1];
        ord[k] = o;
    }
    std::vector<double> tmp((size_t)m * m);
    for (int i = 0; i < m; i++) {
        sigma[i] = nrm[ord[i]];
        std::copy(Y + (size_t)ord[i] * m, Y + (size_t)(ord[i] + 1) * m, tmp.begin() + (size_t)i * m);
        std::copy(W.begin() + (size_t)ord[i] * m, W.begin() + (size_t)(ord[i] + 1) * m, X + (size_t)i * m);
    }
    std::copy(tmp.begin(), tmp.end(), Y);
    // X: the columns with a direction of their own first, then the completion of the others
    const double floor_ = m * eps * (m > 0 && std::isfinite(sigma[0]) ? sigma[0] : 0.0);
    int full = 0;
    for (; full < m && sigma[full] > floor_; full++) {
        double *x = X + (size_t)full * m;
        for (int r = 0; r < m; r++) x[r] /= sigma[full];
    }
    int unit = 0;
    for (int i = full; i < m; i++) {
        double *x = X + (size_t)i * m;
        for (; unit < m; unit++) {
            for (int r = 0; r < m; r++) x[r] = r == unit ? 1.0 : 0.0;
            for (int pass = 0; pass < 2; pass++)
                for (int p = 0; p < i; p++) {
                    const double *y = X + (size_t)p * m;
                    double h = 0;
                    for (int r = 0; r < m; r++) h += y[r] * x[r];
                    for (int r = 0; r < m; r++) x[r] -= h * y[r];
                }
            double s = 0;
            for (int r = 0; r < m; r++) s += x[r] * x[r];
            s = std::sqrt(s);
            if (s > 0.5 / std::sqrt((double)m)) {  // (one of the m unit vectors keeps at least 1 / sqrt(m) of its length)
                for (int r = 0; r < m; r++) x[r] /= s;
                unit++;
                break;
            }
        }
    }
    return sweeps;
}

// ---- the projected matrix of one solve ------------------------------------------------------------------------------------
// Bp after a cycle of a thick-restart Golub-Kahan-Lanczos run, real and upper triangular: the leading keep x keep part is
// diag(kept sigma), column keep holds the arrow rho_i = beta_m X[m - 1, i] (taken analytically from the cycle before), the
// columns start .. d - 1 take alpha_j on the diagonal and beta_j beside it (row j, column j + 1).  d: the dimension the cycle
// reached -- ncv, or j + 1 for the first step j whose beta_j is exactly zero (the space ended; an alpha_j that is exactly zero
// leaves q_j = 0, and B^H q_j = 0 gives beta_j = 0 with it).
struct SvdProjected {
    int ncv = 0, start = 0, d = 0, sweeps = 0;
    double anorm = 0;
    std::vector<double> kept, arrow;          // start entries each
    std::vector<double> Bp, X, Y, sigma;      // d x d thrice, d
    bool finite = true;

    void reset(int ncv_) {
        ncv = ncv_, start = 0, d = 0, sweeps = 0, anorm = 0, finite = true;
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
        Bp.assign((size_t)d * d, 0.0);
        X.assign((size_t)d * d, 0.0);
        Y.assign((size_t)d * d, 0.0);
        sigma.assign((size_t)d, 0.0);
        sweeps = 0;
        if (d == 0 || !finite) return;
        auto b = [&](int r, int c) -> double & { return Bp[(size_t)r + (size_t)c * d]; };
        for (int i = 0; i < start; i++) {
            b(i, i) = kept[i];
            b(i, start) = arrow[i];
        }
        for (int j = start; j < d; j++) {
            b(j, j) = alpha[j];
            if (j + 1 < d) b(j, j + 1) = beta[j];
        }
        sweeps = svds_jacobi(d, Bp.data(), sigma.data(), X.data(), Y.data());
        finite = sweeps < kSvdsMaxSweeps;  // (the cap is reported like a value that is not finite: status 2)
        for (int i = 0; i < d; i++) {
            finite = finite && std::isfinite(sigma[i]);
            if (std::isfinite(sigma[i])) anorm = std::max(anorm, sigma[i]);
        }
    }
    // |beta_m X[d - 1, i]|, the residual estimate of triplet i (beta_m: the last beta of the cycle)
    double estimate(int i, double beta_m) const { return std::fabs(beta_m * X[(size_t)(d - 1) + (size_t)i * d]); }
    // The columns idx[0 .. k) of M (X or Y) made orthonormal to working precision, in that order: two modified Gram-Schmidt
    // passes and a normalisation each, as EigProjected::orthonormalise.
    void orthonormalise(std::vector<double> &M, const int *idx, int k) const {
        for (int c = 0; c < k; c++) {
            double *x = M.data() + (size_t)idx[c] * d;
            for (int pass = 0; pass < 2; pass++)
                for (int p = 0; p < c; p++) {
                    const double *y = M.data() + (size_t)idx[p] * d;
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
    void orthonormalise(const int *idx, int k) {
        orthonormalise(X, idx, k);
        orthonormalise(Y, idx, k);
    }
    // the restart on the triplets idx[0 .. keep): the next cycle starts at column keep
    void restart(const int *idx, int keep, double beta_m) {
        kept.resize((size_t)keep), arrow.resize((size_t)keep);
        for (int i = 0; i < keep; i++) {
            kept[i] = sigma[idx[i]];
            arrow[i] = beta_m * X[(size_t)(d - 1) + (size_t)idx[i] * d];
        }
        start = keep;
    }
};

#if defined(__HIPCC__) || defined(BSM_KRYLOV_LAUNCH)
// ---- launch interface (bsm_svds.hip); everything enqueues on `stream` and returns -----------------------------------------
// pack[j] = alpha[j], pack[m + j] = beta[j], j < m, pack[2 m] = beta[m] (where the solver keeps ||v0||), as doubles (one wave)
hipError_t launch_svds_pack(int dtype, int m, const void *alpha, const void *beta, double *pack, hipStream_t stream);
// The two true residuals of k <= BSM_CG_MAX_RHS triplets in one launch pair.  RM = op(A) V (mrows x k, leading dimension ldrm),
// RN = op(A)^H U (nrows x k, ldrn), U (mrows x k, ldu), V (nrows x k, ldv), sigma: k reals of dtype's real type.
//   part[c * (Gm + Gn) + g] = workgroup g's share of ||RM[:, c] - sigma[c] U[:, c]||^2 for g < Gm = krylov_grid(mrows), of
//   ||RN[:, c] - sigma[c] V[:, c]||^2 for Gm <= g < Gm + Gn, Gn = krylov_grid(nrows);  then, one wave per column in a fixed order,
//   res_av[c] = the root of the sum of the first Gm, res_ahu[c] = of the other Gn, as doubles.  Any element alignment.
hipError_t launch_svds_resid(int dtype, long long mrows, long long nrows, int k, const void *RM, long long ldrm, const void *U,
                             long long ldu, const void *RN, long long ldrn, const void *V, long long ldv, const void *sigma, void *part,
                             double *res_av, double *res_ahu, hipStream_t stream);
#endif

}  // namespace bsm
