// eig_host_check.cpp -- the host side of bsm_eigsh_solve (csrc/bsm_eig.h: the cyclic Jacobi eigensolver, the selection of Ritz
// pairs, the bookkeeping of the projected matrix across thick restarts) on heap buffers, for a run under AddressSanitizer /
// UBSan on a CPU: every buffer is allocated at its exact size, so an access outside an array is an access outside its
// allocation.  Stand-alone (own main, standard library only):
//   c++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all -I blocksparsematrices.jl_amd/csrc \
//       tools/eig_host_check.cpp -o eig_host_check && ./eig_host_check
// 1. eig_jacobi on arrowhead-plus-tridiagonal matrices of order 1, 2, 3, 20, 128: ||T S - S diag(theta)||, ||S^T S - I|| and
//    the order of theta, without a reference solver.
// 2. eig_select / eig_keep over every (which, m, count), m <= 9: the indices are distinct, in range, and the rule's own.
// 3. EigProjected driven by an EXACT Lanczos process on a diagonal operator of order 60 (all arithmetic on the host, full
//    reorthogonalisation, the restart by S as the device does it): the wanted Ritz values must reach the eigenvalues, the
//    analytic arrow entries must equal v_m^T A y_i, and a start vector inside a 3-dimensional invariant subspace must end the
//    space with d = 3.
// Prints the worst figures and exits non-zero when a check fails.
#include <algorithm>
#include <cmath>
#include <cstdio>
#include <random>
#include <vector>

#include "bsm_eig.h"

using namespace bsm;

namespace {
std::mt19937_64 gen(36);
int failures = 0;
void expect(bool ok, const char *what) {
    if (!ok) {
        std::printf("FAILED: %s\n", what);
        failures++;
    }
}

void jacobi_case(int m) {
    std::uniform_real_distribution<double> u(-1, 1);
    const int keep = m / 3;
    std::vector<double> T((size_t)m * m, 0.0), work, theta((size_t)m), S((size_t)m * m);
    for (int i = 0; i < m; i++) T[(size_t)i + (size_t)i * m] = 4.5 * u(gen) + 1.5;
    for (int i = 0; i < keep; i++) T[(size_t)i + (size_t)keep * m] = T[(size_t)keep + (size_t)i * m] = u(gen) * std::pow(10.0, -3.0 * (i % 5));
    for (int j = keep; j + 1 < m; j++) T[(size_t)j + (size_t)(j + 1) * m] = T[(size_t)(j + 1) + (size_t)j * m] = 0.1 + std::fabs(u(gen));
    work = T;
    const int sweeps = eig_jacobi(m, work.data(), theta.data(), S.data());
    double norm = 0, res = 0, orth = 0;
    for (double v : T) norm += v * v;
    norm = std::sqrt(norm);
    for (int c = 0; c < m; c++)
        for (int r = 0; r < m; r++) {
            double ts = 0, ss = 0;
            for (int k = 0; k < m; k++) {
                ts += T[(size_t)r + (size_t)k * m] * S[(size_t)k + (size_t)c * m];
                ss += S[(size_t)k + (size_t)r * m] * S[(size_t)k + (size_t)c * m];
            }
            res = std::max(res, std::fabs(ts - S[(size_t)r + (size_t)c * m] * theta[c]));
            orth = std::max(orth, std::fabs(ss - (r == c ? 1.0 : 0.0)));
        }
    const double scale = m * 2.3e-16 * std::max(norm, 1.0);
    std::printf("jacobi m %3d: %2d sweeps, max |T S - S theta| / (m eps ||T||) %.3f, max |S^T S - I| / (m eps) %.3f\n", m, sweeps, res / scale,
                orth / (m * 2.3e-16));
    expect(sweeps < kEigMaxSweeps, "the sweeps end");
    expect(res <= scale && orth <= m * 2.3e-16 * 4, "jacobi residual / orthogonality");
    for (int i = 1; i < m; i++) expect(theta[i - 1] <= theta[i], "theta ascending");
}

void select_cases() {
    std::uniform_real_distribution<double> u(-3, 3);
    for (int m = 0; m <= 9; m++)
        for (int which = kEigLA; which <= kEigLM; which++)
            for (int count = 0; count <= m; count++) {
                std::vector<double> theta((size_t)m);
                for (double &t : theta) t = std::round(u(gen) * 2) / 2;  // (ties occur)
                std::sort(theta.begin(), theta.end());
                std::vector<int> idx((size_t)count);
                eig_select(which, m, theta.data(), count, idx.data());
                std::vector<int> seen((size_t)m, 0);
                for (int i = 0; i < count; i++) {
                    expect(idx[i] >= 0 && idx[i] < m && !seen[idx[i]]++, "indices distinct and in range");
                    if (which == kEigLA) expect(idx[i] == m - 1 - i, "LA");
                    if (which == kEigSA) expect(idx[i] == i, "SA");
                    if (which == kEigLM && i) expect(std::fabs(theta[idx[i]]) <= std::fabs(theta[idx[i - 1]]), "LM descending");
                }
                if (which == kEigLM)
                    for (int j = 0; j < m; j++)
                        if (!seen[j] && count) expect(std::fabs(theta[j]) <= std::fabs(theta[idx[count - 1]]), "LM takes the largest");
                if (which == kEigBE) {
                    int top = 0;
                    for (int i = 0; i < count; i++) top += idx[i] >= m - (count + 1) / 2;
                    expect(count == 0 || top >= (count + 1) / 2, "BE: ceil(count / 2) from the top");
                }
            }
    for (int nev = 1; nev <= 126; nev++)
        for (int ncv = nev + 2; ncv <= 128; ncv++) {
            const int keep = eig_keep(nev, ncv);
            expect(keep >= nev && keep <= ncv - 1, "keep in nev .. ncv - 1");
        }
}

// Lanczos with full reorthogonalisation on A = diag(lam), all on the host, restarted through EigProjected
void lanczos_case(int which, int nev, int ncv, bool invariant) {
    const int n = 60;
    std::vector<double> lam((size_t)n);
    for (int i = 0; i < n; i++) lam[i] = 1.0 + i / (double)n;
    lam[0] = -3.3, lam[1] = -2.2, lam[2] = -1.5, lam[n - 3] = 3.0, lam[n - 2] = 4.3, lam[n - 1] = 6.0;
    std::uniform_real_distribution<double> u(-1, 1);
    std::vector<double> V((size_t)n * (ncv + 1), 0.0), alpha((size_t)ncv), beta((size_t)ncv), W;
    double nrm = 0;
    for (int i = 0; i < (invariant ? 3 : n); i++) V[i] = u(gen), nrm += V[i] * V[i];
    for (int i = 0; i < n; i++) V[i] /= std::sqrt(nrm);
    EigProjected P;
    P.reset(ncv);
    std::vector<int> idx((size_t)ncv);
    double worst_arrow = 0;
    for (int cycle = 1; cycle <= 200; cycle++) {
        for (int j = P.start; j < ncv; j++) {
            double *w = V.data() + (size_t)(j + 1) * n;
            const double *vj = V.data() + (size_t)j * n;
            for (int i = 0; i < n; i++) w[i] = lam[i] * vj[i];
            double hj = 0;
            for (int pass = 0; pass < 2; pass++)
                for (int c = 0; c <= j; c++) {
                    const double *vc = V.data() + (size_t)c * n;
                    double h = 0;
                    for (int i = 0; i < n; i++) h += vc[i] * w[i];
                    for (int i = 0; i < n; i++) w[i] -= h * vc[i];
                    if (c == j) hj += h;
                    if (cycle > 1 && j == P.start && c < P.start && pass == 0) worst_arrow = std::max(worst_arrow, std::fabs(h - P.arrow[c]));
                }
            double b = 0;
            for (int i = 0; i < n; i++) b += w[i] * w[i];
            b = std::sqrt(b);
            if (invariant && b < 1e-12) b = 0;  // (rounding noise of an exact breakdown, as the exact tridiagonal case of the tests)
            alpha[j] = hj, beta[j] = b;
            for (int i = 0; i < n; i++) w[i] = b > 0 ? w[i] / b : 0.0;
        }
        P.cycle(alpha.data(), beta.data());
        expect(P.finite, "finite");
        if (P.d < ncv) {
            expect(invariant && P.d == 3, "the space ends with d = 3 for a start vector in a 3-dimensional invariant subspace");
            return;
        }
        expect(!invariant, "an invariant start vector must end the space");
        const double beta_m = beta[ncv - 1];
        eig_select(which, P.d, P.theta.data(), nev, idx.data());
        bool all = true;
        for (int i = 0; i < nev; i++) all = all && P.estimate(idx[i], beta_m) <= 1e-10 * P.anorm;
        if (all) {
            std::vector<double> sorted(lam);
            std::sort(sorted.begin(), sorted.end());
            std::vector<int> want((size_t)nev);
            eig_select(which, n, sorted.data(), nev, want.data());
            double err = 0;
            for (int i = 0; i < nev; i++) err = std::max(err, std::fabs(P.theta[idx[i]] - sorted[want[i]]));
            std::printf("lanczos which %d nev %d ncv %2d: %3d cycles, max |theta - lambda| %.2e, max |arrow - v_m^T A y_i| %.2e, anorm %.6f\n", which, nev,
                        ncv, cycle, err, worst_arrow, P.anorm);
            expect(err <= 1e-9 && worst_arrow <= 1e-12 && P.anorm <= 6.0 * (1 + 1e-14), "converged to the eigenvalues");
            return;
        }
        const int keep = eig_keep(nev, ncv);
        eig_select(which, P.d, P.theta.data(), keep, idx.data());
        P.orthonormalise(idx.data(), keep);
        W.assign((size_t)n * keep, 0.0);
        for (int c = 0; c < keep; c++)
            for (int j = 0; j < ncv; j++) {
                const double s = P.S[(size_t)j + (size_t)idx[c] * P.d];
                for (int i = 0; i < n; i++) W[(size_t)i + (size_t)c * n] += V[(size_t)i + (size_t)j * n] * s;
            }
        std::copy(V.begin() + (size_t)ncv * n, V.begin() + (size_t)(ncv + 1) * n, V.begin() + (size_t)keep * n);
        std::copy(W.begin(), W.end(), V.begin());
        P.restart(idx.data(), keep, beta_m);
    }
    expect(false, "lanczos did not converge in 200 cycles");
}
}  // namespace

int main() {
    for (int m : {1, 2, 3, 20, 128}) jacobi_case(m);
    select_cases();
    for (int which = kEigLA; which <= kEigLM; which++) {
        lanczos_case(which, 3, 12, false);
        lanczos_case(which, 1, 3, false);
    }
    lanczos_case(kEigLA, 4, 8, true);
    std::printf(failures ? "%d check(s) FAILED\n" : "all checks passed\n", failures);
    return failures ? 1 : 0;
}
