// eigh_host_check.cpp -- the host route of bsm_eigh_blocks / bsm_spectral_blocks (csrc/bsm_eigh.h: the round-robin Jacobi
// eigensolver and V f(w) V^H in plain C++) on heap buffers, for a run under AddressSanitizer / UBSan on a CPU: every buffer is
// allocated at its exact size, so an access outside an array is an access outside its allocation.  Stand-alone (own main,
// standard library only):
//   c++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all -I blocksparsematrices.jl_amd/csrc \
//       tools/eigh_host_check.cpp -o eigh_host_check && ./eigh_host_check
// 1. eigh_pair: every step of a sweep over m = 2 .. 40 holds m / 2 disjoint pairs, a sweep meets every pair once.
// 2. eigh_block_host on uniform Hermitian blocks of order 1, 2, 3, 9, 64, 65 in the four types, leading dimension n + 3:
//    ||H V - V diag(w)||, ||V^H V - I||, the order of w and the padding rows, without a reference solver; a NaN entry.
// 3. spectral_block_host: V f(w) V^H of those pairs under the four functions -- INV gives the inverse (H X = I to rounding),
//    the output is Hermitian to the bit, a zero eigenvalue is named.
// Prints the worst figures and exits non-zero when a check fails.
#include <algorithm>
#include <cmath>
#include <complex>
#include <cstdio>
#include <limits>
#include <random>
#include <vector>

#include "bsm_eigh.h"

using namespace bsm;

namespace {
std::mt19937_64 gen(38);
int failures = 0;
void expect(bool ok, const char *what) {
    if (!ok) {
        std::printf("FAILED: %s\n", what);
        failures++;
    }
}

void pair_cases() {
    for (int m = 2; m <= 40; m += 2) {
        std::vector<int> met((size_t)m * m, 0);
        for (int t = 0; t < m - 1; t++) {
            std::vector<int> used((size_t)m, 0);
            for (int k = 0; k < m / 2; k++) {
                int p, q;
                eigh_pair(m, t, k, p, q);
                expect(0 <= p && p < q && q < m, "0 <= p < q < m");
                if (p < 0 || q >= m) continue;
                expect(!used[p]++ && !used[q]++, "the pairs of a step are disjoint");
                met[(size_t)p * m + q]++;
            }
        }
        for (int p = 0; p < m; p++)
            for (int q = p + 1; q < m; q++) expect(met[(size_t)p * m + q] == 1, "a sweep meets every pair once");
    }
}

template <typename R, int NC> void block_case(int n, const char *name) {
    using C = std::complex<double>;
    std::uniform_real_distribution<double> u(-1, 1);
    const int ld = n + 3;
    const R guard = R(-77);
    std::vector<R> a((size_t)ld * n * NC, guard), w((size_t)n), out((size_t)ld * n * NC, guard);
    std::vector<C> H((size_t)n * n);
    for (int j = 0; j < n; j++)
        for (int i = j; i < n; i++) {
            const C v(u(gen), NC == 2 && i != j ? u(gen) : 0.0);
            const C r((double)(R)v.real(), (double)(R)v.imag());
            H[(size_t)i + (size_t)j * n] = r, H[(size_t)j + (size_t)i * n] = std::conj(r);
        }
    for (int j = 0; j < n; j++)
        for (int i = 0; i < n; i++) {
            a[((size_t)i + (size_t)j * ld) * NC] = (R)H[(size_t)i + (size_t)j * n].real();
            if (NC == 2) a[((size_t)i + (size_t)j * ld) * NC + 1] = (R)H[(size_t)i + (size_t)j * n].imag();
        }
    int32_t sweeps = 0;
    const int info = eigh_block_host<R, NC>(a.data(), n, ld, w.data(), true, sweeps);
    auto V = [&](int i, int j) { return C(a[((size_t)i + (size_t)j * ld) * NC], NC == 2 ? a[((size_t)i + (size_t)j * ld) * NC + NC - 1] : R(0)); };
    double norm = 0, res = 0, orth = 0;
    for (const C &v : H) norm += std::norm(v);
    norm = std::sqrt(norm);
    for (int c = 0; c < n; c++)
        for (int r = 0; r < n; r++) {
            C hv = 0, vv = 0;
            for (int k = 0; k < n; k++) hv += H[(size_t)r + (size_t)k * n] * V(k, c), vv += std::conj(V(k, r)) * V(k, c);
            res += std::norm(hv - V(r, c) * (double)w[c]);
            orth += std::norm(vv - (r == c ? 1.0 : 0.0));
        }
    const double eps = std::numeric_limits<R>::epsilon();
    const double rho_r = std::sqrt(res) / (2 * n * eps * std::max(norm, 1e-300)), rho_o = std::sqrt(orth) / (2 * std::pow(n, 1.5) * eps);
    std::printf("eigh %s n %2d: info %d, %2d sweeps, rho_r %.3f rho_o %.3f\n", name, n, info, (int)sweeps, rho_r, rho_o);
    expect(info == 0 && sweeps <= 20, "the sweeps end");
    expect(rho_r <= 4 && rho_o <= 4, "residual / orthogonality");
    for (int i = 1; i < n; i++) expect(w[i - 1] <= w[i], "w ascending");
    for (int j = 0; j < n; j++)
        for (int i = n; i < ld; i++)
            for (int c = 0; c < NC; c++) expect(a[((size_t)i + (size_t)j * ld) * NC + c] == guard, "the padding rows are untouched");
    // V f(w) V^H: the inverse, bit-Hermitian; then a zero eigenvalue
    for (int func = kSpecValues; func <= kSpecPinv; func++) {
        std::fill(out.begin(), out.end(), guard);
        const int64_t bad = spectral_block_host<R, NC>(a.data(), n, ld, w.data(), func, 1e-3, out.data(), ld);
        expect(bad == 0, "f is defined on a uniform block");
        auto X = [&](int i, int j) { return C(out[((size_t)i + (size_t)j * ld) * NC], NC == 2 ? out[((size_t)i + (size_t)j * ld) * NC + NC - 1] : R(0)); };
        double worst = 0, big = 0;
        for (int c = 0; c < n; c++)
            for (int r = 0; r < n; r++) {
                expect(X(r, c) == std::conj(X(c, r)), "Hermitian to the bit");
                big = std::max(big, std::abs(X(r, c)));
                if (func != kSpecInv) continue;
                C hx = 0;
                for (int k = 0; k < n; k++) hx += H[(size_t)r + (size_t)k * n] * X(k, c);
                worst = std::max(worst, std::abs(hx - (r == c ? 1.0 : 0.0)));
            }
        if (func == kSpecInv) {
            std::printf("  inv: max |H X - I| / (n eps ||H|| max|X|) %.3f\n", worst / (n * eps * norm * big));
            expect(worst <= 16 * n * eps * norm * big, "V (1 / w) V^H is the inverse");
        }
        for (int j = 0; j < n; j++)
            for (int i = n; i < ld; i++)
                for (int c = 0; c < NC; c++) expect(out[((size_t)i + (size_t)j * ld) * NC + c] == guard, "the padding rows of out are untouched");
    }
    if (n >= 2) {
        std::vector<R> wz(w);
        wz[1] = R(0);
        std::fill(out.begin(), out.end(), guard);
        expect(spectral_block_host<R, NC>(a.data(), n, ld, wz.data(), kSpecInv, 0.0, out.data(), ld) == 2, "the zero eigenvalue is named");
        expect(std::all_of(out.begin(), out.end(), [&](R v) { return v == guard; }), "out is not written then");
        expect(spectral_block_host<R, NC>(a.data(), n, ld, wz.data(), kSpecPinv, 0.0, out.data(), ld) == 0, "pinv drops it");
    }
    // a NaN entry: info 1, the block untouched, w NaN
    std::vector<R> b(a);
    b[0] = std::numeric_limits<R>::quiet_NaN();
    const std::vector<R> was(b);
    expect((eigh_block_host<R, NC>(b.data(), n, ld, w.data(), true, sweeps)) == 1, "info 1 on a NaN entry");
    bool same = true;
    for (size_t i = 1; i < b.size(); i++) same = same && b[i] == was[i];
    expect(same && std::isnan(w[0]) && std::isnan(w[(size_t)n - 1]), "the block is untouched, w is NaN");
}
}  // namespace

int main() {
    pair_cases();
    for (int n : {1, 2, 3, 9, 64, 65}) {
        block_case<float, 1>(n, "float32");
        block_case<double, 1>(n, "float64");
        block_case<float, 2>(n, "complex64");
        block_case<double, 2>(n, "complex128");
    }
    std::printf(failures ? "%d check(s) FAILED\n" : "all checks passed\n", failures);
    return failures ? 1 : 0;
}
