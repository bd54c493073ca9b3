// lobpcg_host_check.cpp -- the host side of bsm_lobpcg_solve (csrc/bsm_lobpcg.h: the cyclic Hermitian Jacobi eigensolver and the
// Rayleigh-Ritz step of one iteration) on heap buffers, for a run under AddressSanitizer / UBSan on a CPU: every buffer is
// allocated at its exact size, so an access outside an array is an access outside its allocation.  Stand-alone (own main,
// standard library only):
//   c++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all -I blocksparsematrices.jl_amd/csrc \
//       tools/lobpcg_host_check.cpp -o lobpcg_host_check && ./lobpcg_host_check
// 1. eig_jacobi_h on random real symmetric and complex Hermitian matrices of order 1, 2, 3, 20, 48: ||A Q - Q diag(theta)||,
//    ||Q^H Q - I|| and the order of theta, without a reference solver.
// 2. lob_rr on the Gram matrices of random bases S (64 x p, p = 3, 9, 18, 48) against A = diag: full bases, partly inactive ones
//    (a P and a W column out of use), a rank-deficient one (a W column that repeats an X column: one direction dropped), for SA
//    and LA, real and complex: C^H G_B C = I, C^H G_A C = diag(theta), zero rows for the columns not in use, theta in order.
// 3. The statuses: fewer columns in use than k, a basis of rank below k, a zero column (3); a NaN entry (2).
// Prints the worst figures and exits non-zero when a check fails.
#include <algorithm>
#include <cmath>
#include <complex>
#include <cstdio>
#include <limits>
#include <random>
#include <vector>

#include "bsm_lobpcg.h"

using namespace bsm;

namespace {
std::mt19937_64 gen(37);
int failures = 0;
void expect(bool ok, const char *what) {
    if (!ok) {
        std::printf("FAILED: %s\n", what);
        failures++;
    }
}
template <typename T> T draw();
template <> double draw<double>() { return std::uniform_real_distribution<double>(-1, 1)(gen); }
template <> std::complex<double> draw<std::complex<double>>() { return {draw<double>(), draw<double>()}; }
template <typename T> const char *kind() { return sizeof(T) == sizeof(double) ? "real" : "complex"; }

template <typename T> void jacobi_case(int m) {
    std::vector<T> A((size_t)m * m), work, Q((size_t)m * m);
    std::vector<double> theta((size_t)m);
    for (int c = 0; c < m; c++)
        for (int r = 0; r <= c; r++) {
            const T v = draw<T>();
            A[(size_t)r + (size_t)c * m] = r == c ? T(lob_re(v)) : v;
            A[(size_t)c + (size_t)r * m] = r == c ? T(lob_re(v)) : lob_conj(v);
        }
    work = A;
    const int sweeps = eig_jacobi_h<T>(m, work.data(), theta.data(), Q.data());
    double norm = 0, res = 0, orth = 0;
    for (const T &v : A) norm += lob_abs(v) * lob_abs(v);
    norm = std::sqrt(norm);
    for (int c = 0; c < m; c++)
        for (int r = 0; r < m; r++) {
            T aq = T(0), qq = T(0);
            for (int k = 0; k < m; k++) {
                aq += A[(size_t)r + (size_t)k * m] * Q[(size_t)k + (size_t)c * m];
                qq += lob_conj(Q[(size_t)k + (size_t)r * m]) * Q[(size_t)k + (size_t)c * m];
            }
            res = std::max(res, lob_abs(aq - Q[(size_t)r + (size_t)c * m] * theta[c]));
            orth = std::max(orth, lob_abs(qq - (r == c ? T(1) : T(0))));
        }
    const double scale = m * 2.3e-16 * std::max(norm, 1.0);
    std::printf("jacobi_h %-7s m %2d: %2d sweeps, max |A Q - Q theta| / (m eps ||A||) %.3f, max |Q^H Q - I| / (m eps) %.3f\n", kind<T>(), m, sweeps,
                res / scale, orth / (m * 2.3e-16));
    expect(sweeps < kEigMaxSweeps, "the sweeps end");
    expect(res <= scale && orth <= m * 2.3e-16 * 4, "jacobi residual / orthogonality");
    for (int i = 1; i < m; i++) expect(theta[i - 1] <= theta[i], "theta ascending");
}

// G_B = S^H S, G_A = S^H diag(lam) S for a random S (n x p); dup >= 0: column dup repeats column 0; zero >= 0: a zero column
template <typename T> void grams(int n, int p, int dup, int zero, std::vector<T> &GB, std::vector<T> &GA) {
    std::vector<T> S((size_t)n * p);
    std::vector<double> lam((size_t)n);
    for (T &v : S) v = draw<T>();
    for (int i = 0; i < n; i++) lam[i] = 2.5 * draw<double>() + 0.5;
    if (dup >= 0) std::copy(S.begin(), S.begin() + n, S.begin() + (size_t)dup * n);
    if (zero >= 0) std::fill(S.begin() + (size_t)zero * n, S.begin() + (size_t)(zero + 1) * n, T(0));
    GB.assign((size_t)p * p, T(0)), GA.assign((size_t)p * p, T(0));
    for (int c = 0; c < p; c++)
        for (int r = 0; r < p; r++) {
            T b = T(0), a = T(0);
            for (int i = 0; i < n; i++) {
                const T u = lob_conj(S[(size_t)i + (size_t)r * n]), w = S[(size_t)i + (size_t)c * n];
                b += u * w;
                a += u * (w * lam[i]);
            }
            GB[(size_t)r + (size_t)c * p] = b, GA[(size_t)r + (size_t)c * p] = a;
        }
}

template <typename T> void rr_case(int p, int which, int mode) {  // mode 0: full, 1: partly inactive, 2: rank-deficient
    const int k = p / 3, n = 64;
    std::vector<T> GB, GA, C((size_t)p * k);
    std::vector<unsigned char> use((size_t)p, 1);
    std::vector<double> theta((size_t)k);
    if (mode == 1 && p > 3) use[k + 1 < 2 * k ? k + 1 : k] = use[2 * k] = 0;
    grams<T>(n, p, mode == 2 ? p - 1 : -1, -1, GB, GA);
    int drops = -1;
    double big = 0;
    const int status = lob_rr<T>(p, k, which, GB.data(), p, GA.data(), p, use.data(), 64.0 * p * 2.3e-16, theta.data(), C.data(), &drops, &big);
    expect(status == 0, "status 0");
    expect(drops == (mode == 2 ? 1 : 0), "the repeated column is dropped, nothing else");
    if (status != 0) return;
    double worst_b = 0, worst_a = 0, scale_a = 0;
    for (const T &v : GA) scale_a = std::max(scale_a, lob_abs(v));
    for (int c = 0; c < k; c++)
        for (int r = 0; r < k; r++) {
            T b = T(0), a = T(0);
            for (int j = 0; j < p; j++)
                for (int i = 0; i < p; i++) {
                    b += lob_conj(C[(size_t)i + (size_t)r * p]) * GB[(size_t)i + (size_t)j * p] * C[(size_t)j + (size_t)c * p];
                    a += lob_conj(C[(size_t)i + (size_t)r * p]) * GA[(size_t)i + (size_t)j * p] * C[(size_t)j + (size_t)c * p];
                }
            worst_b = std::max(worst_b, lob_abs(b - (r == c ? T(1) : T(0))));
            worst_a = std::max(worst_a, lob_abs(a - (r == c ? T(theta[c]) : T(0))));
        }
    for (int i = 0; i < p; i++)
        if (!use[i])
            for (int c = 0; c < k; c++) expect(C[(size_t)i + (size_t)c * p] == T(0), "zero rows for the columns not in use");
    for (int c = 1; c < k; c++) expect(which == kEigSA ? theta[c - 1] <= theta[c] : theta[c - 1] >= theta[c], "theta in the order of which");
    expect(big + 1e-300 >= std::fabs(theta[0]), "mu_abs bounds the selected values");
    std::printf("rr %-7s p %2d which %d mode %d: drops %d, max |C^H G_B C - I| %.2e, max |C^H G_A C - theta| %.2e\n", kind<T>(), p, which, mode, drops,
                worst_b, worst_a);
    // (a random 64 x p basis, p <= 48, is well conditioned: cond below 1e4)
    expect(worst_b <= 1e-10 && worst_a <= 1e-10 * std::max(scale_a, 1.0), "the Ritz basis is G_B-orthonormal and diagonalises G_A");
}

template <typename T> void status_cases() {
    const int p = 9, k = 3;
    std::vector<T> GB, GA, C((size_t)p * k);
    std::vector<double> theta((size_t)k);
    std::vector<unsigned char> use((size_t)p, 1);
    int drops = 0;
    double big = 0;
    auto run = [&]() { return lob_rr<T>(p, k, kEigSA, GB.data(), p, GA.data(), p, use.data(), 64.0 * p * 2.3e-16, theta.data(), C.data(), &drops, &big); };
    grams<T>(40, p, -1, -1, GB, GA);
    std::fill(use.begin(), use.end(), 0);
    use[0] = use[1] = 1;
    expect(run() == 3, "fewer columns in use than k: status 3");
    std::fill(use.begin(), use.end(), 0);
    use[0] = use[3] = use[4] = use[5] = 1;  // rank 2 of 4 below: columns 3, 4, 5 repeat column 0
    {
        std::vector<T> B2, A2;
        grams<T>(40, p, 3, -1, B2, A2);
        // (one repeat only from grams: copy column / row 3 over 4 and 5)
        for (int t : {4, 5})
            for (int i = 0; i < p; i++) {
                B2[(size_t)i + (size_t)t * p] = B2[(size_t)i + (size_t)3 * p], A2[(size_t)i + (size_t)t * p] = A2[(size_t)i + (size_t)3 * p];
            }
        for (int t : {4, 5})
            for (int i = 0; i < p; i++) {
                B2[(size_t)t + (size_t)i * p] = B2[(size_t)3 + (size_t)i * p], A2[(size_t)t + (size_t)i * p] = A2[(size_t)3 + (size_t)i * p];
            }
        GB = B2, GA = A2;
    }
    expect(run() == 3 && drops == 3, "a basis of rank 1 where 3 directions are wanted: status 3");
    std::fill(use.begin(), use.end(), 1);
    grams<T>(40, p, -1, 4, GB, GA);
    expect(run() == 3, "a zero column: status 3");
    grams<T>(40, p, -1, -1, GB, GA);
    GA[5] = T(std::numeric_limits<double>::quiet_NaN());
    expect(run() == 2, "a NaN entry: status 2");
}
}  // namespace

int main() {
    for (int m : {1, 2, 3, 20, 48}) {
        jacobi_case<double>(m);
        jacobi_case<std::complex<double>>(m);
    }
    for (int p : {3, 9, 18, 48})
        for (int which : {(int)kEigSA, (int)kEigLA})
            for (int mode = 0; mode < 3; mode++) {
                if (mode == 2 && p == 3) continue;  // (k = 1 of 3 columns: a repeat leaves rank 2 >= k, covered by the larger cases)
                rr_case<double>(p, which, mode);
                rr_case<std::complex<double>>(p, which, mode);
            }
    status_cases<double>();
    status_cases<std::complex<double>>();
    std::printf(failures ? "%d check(s) FAILED\n" : "all checks passed\n", failures);
    return failures ? 1 : 0;
}
