// svds_host_check.cpp -- the host side of bsm_svds_solve (csrc/bsm_svds.h: the one-sided Jacobi SVD, the selection of singular
// triplets, the bookkeeping of the projected matrix across thick restarts) on heap buffers, for a run under AddressSanitizer /
// UBSan on a CPU: every buffer is allocated at its exact size, so an access outside an array is an access outside its
// allocation.  Stand-alone (own main, standard library only):
//   c++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all -I blocksparsematrices.jl_amd/csrc \
//       tools/svds_host_check.cpp -o svds_host_check && ./svds_host_check
// 1. svds_jacobi on arrow-plus-bidiagonal upper triangular matrices of order 1, 2, 3, 12, 128, on one with an exactly zero
//    column, one with a zero last row, one with a double singular value, and on the all-ones upper triangle (its largest
//    column norm is far below sigma_max) with one column below the skip rule's floor and one between that floor and the
//    completion's threshold: |B Y - X diag(sigma)|, ||X^T X - I||, ||Y^T Y - I|| and the order of sigma, without a reference solver.
// 2. svds_select / svds_keep over every (which, m, count), m <= 9, and every (nsv, ncv).
// 3. SvdProjected driven by an EXACT Golub-Kahan-Lanczos process on a 90 x 60 operator diag(s) over zero rows (all arithmetic
//    on the host, full two-sided reorthogonalisation, the restart by Y and X as the device does it): the wanted values must
//    reach the singular values, the analytic arrow entries must equal q_i^T B p_keep, and the start vector e_1 must end the
//    space with d = 1.
// Prints the worst figures and exits non-zero when a check fails.
#include <algorithm>
#include <cmath>
#include <cstdio>
#include <random>
#include <vector>

#include "bsm_svds.h"

using namespace bsm;

namespace {
std::mt19937_64 gen(39);
int failures = 0;
void expect(bool ok, const char *what) {
    if (!ok) {
        std::printf("FAILED: %s\n", what);
        failures++;
    }
}

enum { kPlain, kZeroColumn, kZeroRow, kDouble, kFlat };

void jacobi_case(int m, int kind) {
    std::uniform_real_distribution<double> u(-1, 1);
    const int keep = m / 3;
    std::vector<double> B((size_t)m * m, 0.0), sigma((size_t)m), X((size_t)m * m), Y((size_t)m * m);
    auto b = [&](int r, int c) -> double & { return B[(size_t)r + (size_t)c * m]; };
    for (int i = 0; i < m; i++) b(i, i) = 3.0 * std::fabs(u(gen)) + 0.1;
    for (int i = 0; i < keep; i++) b(i, keep) = u(gen) * std::pow(10.0, -3.0 * (i % 5));
    for (int j = keep; j + 1 < m; j++) b(j, j + 1) = 0.1 + std::fabs(u(gen));
    if (kind == kZeroColumn)
        for (int r = 0; r < m; r++) b(r, m / 2) = 0.0;
    if (kind == kZeroRow) b(m - 1, m - 1) = 0.0;
    if (kind == kDouble) {
        std::fill(B.begin(), B.end(), 0.0);
        for (int i = 0; i < m; i++) b(i, i) = i < 2 ? 2.0 : 1.0 + i;
        b(0, m - 1) = 0.5;
    }
    if (kind == kFlat) {
        // all ones on and above the diagonal: the largest column norm (sqrt(m)) is well below sigma_max (about 0.64 m), so the
        // floor of the skip rule (m eps sqrt(m)) lies below the completion's (m eps sigma_max); two columns scaled down to
        // 1e-18 and to half the completion's threshold lie below the one and between the two
        for (int c = 0; c < m; c++)
            for (int r = 0; r < m; r++) b(r, c) = r <= c ? 1.0 : 0.0;
        const double between = 0.5 * m * 2.2e-16 * 0.64 * m;
        for (int r = 0; r < m; r++) b(r, m / 2) *= 1e-18, b(r, m / 3) *= between / std::sqrt(m / 3 + 1.0);
    }
    const int sweeps = svds_jacobi(m, B.data(), sigma.data(), X.data(), Y.data());
    double res = 0, orth = 0;
    for (int c = 0; c < m; c++)
        for (int r = 0; r < m; r++) {
            double by = 0, xx = 0, yy = 0;
            for (int k = 0; k < m; k++) {
                by += B[(size_t)r + (size_t)k * m] * Y[(size_t)k + (size_t)c * m];
                xx += X[(size_t)k + (size_t)r * m] * X[(size_t)k + (size_t)c * m];
                yy += Y[(size_t)k + (size_t)r * m] * Y[(size_t)k + (size_t)c * m];
            }
            res = std::max(res, std::fabs(by - X[(size_t)r + (size_t)c * m] * sigma[c]));
            orth = std::max(orth, std::max(std::fabs(xx - (r == c ? 1.0 : 0.0)), std::fabs(yy - (r == c ? 1.0 : 0.0))));
        }
    const double scale = m * 2.3e-16 * std::max(sigma[0], 1.0);
    std::printf("jacobi m %3d kind %d: %2d sweeps, max |B Y - X sigma| / (m eps smax) %.3f, max |X^T X - I|, |Y^T Y - I| / (m eps) %.3f, smin %.3e\n", m,
                kind, sweeps, res / scale, orth / (m * 2.3e-16), sigma[m - 1]);
    expect(sweeps < kSvdsMaxSweeps, "the sweeps end");
    expect(res <= scale && orth <= m * 2.3e-16 * 4, "jacobi residual / orthogonality");
    for (int i = 1; i < m; i++) expect(sigma[i - 1] >= sigma[i] && sigma[i] >= 0, "sigma descending and not negative");
    if (kind == kZeroColumn) expect(sigma[m - 1] == 0.0, "a zero column gives an exactly zero singular value");
    if (kind == kZeroRow) expect(sigma[m - 1] <= scale && std::fabs(std::fabs(X[(size_t)(m - 1) + (size_t)(m - 1) * m]) - 1.0) <= m * 2.3e-16 * 4,
                                 "a zero last row: sigma_min = 0 with the left vector e_{m-1}");
}

void select_cases() {
    for (int m = 0; m <= 9; m++)
        for (int which = kSvdsLM; which <= kSvdsSM; which++)
            for (int count = 0; count <= m; count++) {
                std::vector<int> idx((size_t)count);
                svds_select(which, m, count, idx.data());
                for (int i = 0; i < count; i++) expect(idx[i] == (which == kSvdsLM ? i : m - 1 - i), "selection");
            }
    for (int nsv = 1; nsv <= 126; nsv++)
        for (int ncv = nsv + 2; ncv <= 128; ncv++) {
            const int keep = svds_keep(nsv, ncv);
            expect(keep >= nsv && keep <= ncv - 1, "keep in nsv .. ncv - 1");
        }
}

// Golub-Kahan-Lanczos with full reorthogonalisation on B = [diag(s); 0] (l x n), all on the host, restarted through SvdProjected
void gkl_case(int which, int nsv, int ncv, bool invariant) {
    const int n = 60, l = 90;
    std::vector<double> s((size_t)n);
    for (int i = 0; i < n; i++) s[i] = 2.0 + i / (double)n;
    s[0] = 0.1, s[1] = 0.4, s[2] = 0.7, s[n - 3] = 4.0, s[n - 2] = 5.1, s[n - 1] = 6.6;
    std::uniform_real_distribution<double> u(-1, 1);
    std::vector<double> P((size_t)n * (ncv + 1), 0.0), Q((size_t)l * ncv, 0.0), alpha((size_t)ncv), beta((size_t)ncv), W;
    double nrm = 0;
    for (int i = 0; i < (invariant ? 1 : n); i++) P[i] = invariant ? 1.0 : u(gen), nrm += P[i] * P[i];
    for (int i = 0; i < n; i++) P[i] /= std::sqrt(nrm);
    SvdProjected S;
    S.reset(ncv);
    std::vector<int> idx((size_t)ncv);
    double worst_arrow = 0;
    // w orthogonalised twice against the k leading columns of M (rows x *); first[c]: the first pass's coefficient
    auto orth = [](const std::vector<double> &M, int rows, int k, double *w, std::vector<double> *first) {
        for (int pass = 0; pass < 2; pass++)
            for (int c = 0; c < k; c++) {
                const double *mc = M.data() + (size_t)c * rows;
                double h = 0;
                for (int i = 0; i < rows; i++) h += mc[i] * w[i];
                for (int i = 0; i < rows; i++) w[i] -= h * mc[i];
                if (first && pass == 0) (*first)[c] = h;
            }
        double b = 0;
        for (int i = 0; i < rows; i++) b += w[i] * w[i];
        return std::sqrt(b);
    };
    for (int cycle = 1; cycle <= 300; cycle++) {
        for (int j = S.start; j < ncv; j++) {
            double *q = Q.data() + (size_t)j * l, *r = P.data() + (size_t)(j + 1) * n;
            const double *pj = P.data() + (size_t)j * n;
            for (int i = 0; i < l; i++) q[i] = i < n ? s[i] * pj[i] : 0.0;
            std::vector<double> first((size_t)ncv, 0.0);
            double a = orth(Q, l, j, q, &first);
            if (cycle > 1 && j == S.start)
                for (int c = 0; c < S.start; c++) worst_arrow = std::max(worst_arrow, std::fabs(first[c] - S.arrow[c]));
            if (invariant && a < 1e-12) a = 0;
            for (int i = 0; i < l; i++) q[i] = a > 0 ? q[i] / a : 0.0;
            for (int i = 0; i < n; i++) r[i] = s[i] * q[i];
            double b = orth(P, n, j + 1, r, nullptr);
            if (invariant && b < 1e-12) b = 0;  // (rounding noise of an exact breakdown)
            for (int i = 0; i < n; i++) r[i] = b > 0 ? r[i] / b : 0.0;
            alpha[j] = a, beta[j] = b;
        }
        S.cycle(alpha.data(), beta.data());
        expect(S.finite, "finite");
        if (S.d < ncv) {
            expect(invariant && S.d == 1 && std::fabs(S.sigma[0] - s[0]) <= 1e-15, "e_1 ends the space with d = 1 and sigma = s_1");
            return;
        }
        expect(!invariant, "an invariant start vector must end the space");
        const double beta_m = beta[ncv - 1];
        svds_select(which, S.d, nsv, idx.data());
        bool all = true;
        for (int i = 0; i < nsv; i++) all = all && S.estimate(idx[i], beta_m) <= 1e-10 * S.anorm;
        if (all) {
            std::vector<double> sorted(s);
            std::sort(sorted.begin(), sorted.end(), [](double x, double y) { return x > y; });
            std::vector<int> want((size_t)nsv);
            svds_select(which, n, nsv, want.data());
            double err = 0;
            for (int i = 0; i < nsv; i++) err = std::max(err, std::fabs(S.sigma[idx[i]] - sorted[want[i]]));
            std::printf("gkl which %d nsv %d ncv %2d: %3d cycles, max |sigma - s| %.2e, max |arrow - q_i^T B p_keep| %.2e, anorm %.6f\n", which, nsv, ncv,
                        cycle, err, worst_arrow, S.anorm);
            expect(err <= 1e-9 && worst_arrow <= 1e-12 && S.anorm <= 6.6 * (1 + 1e-14), "converged to the singular values");
            return;
        }
        const int keep = svds_keep(nsv, ncv);
        svds_select(which, S.d, keep, idx.data());
        S.orthonormalise(idx.data(), keep);
        auto compress = [&](std::vector<double> &M, int rows, const std::vector<double> &small) {
            W.assign((size_t)rows * keep, 0.0);
            for (int c = 0; c < keep; c++)
                for (int j = 0; j < ncv; j++) {
                    const double f = small[(size_t)j + (size_t)idx[c] * S.d];
                    for (int i = 0; i < rows; i++) W[(size_t)i + (size_t)c * rows] += M[(size_t)i + (size_t)j * rows] * f;
                }
        };
        compress(P, n, S.Y);
        std::copy(P.begin() + (size_t)ncv * n, P.begin() + (size_t)(ncv + 1) * n, P.begin() + (size_t)keep * n);
        std::copy(W.begin(), W.end(), P.begin());
        compress(Q, l, S.X);
        std::copy(W.begin(), W.end(), Q.begin());
        S.restart(idx.data(), keep, beta_m);
    }
    expect(false, "gkl did not converge in 300 cycles");
}
}  // namespace

int main() {
    for (int m : {1, 2, 3, 12, 128}) jacobi_case(m, kPlain);
    jacobi_case(12, kZeroColumn);
    jacobi_case(12, kZeroRow);
    jacobi_case(12, kDouble);
    jacobi_case(128, kZeroColumn);
    jacobi_case(12, kFlat);
    jacobi_case(128, kFlat);
    select_cases();
    for (int which = kSvdsLM; which <= kSvdsSM; which++) {
        gkl_case(which, 3, 12, false);
        gkl_case(which, 4, 20, false);
    }
    gkl_case(kSvdsLM, 1, 3, false);
    gkl_case(kSvdsLM, 1, 3, true);
    std::printf(failures ? "%d check(s) FAILED\n" : "all checks passed\n", failures);
    return failures ? 1 : 0;
}
