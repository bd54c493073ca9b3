// krylov_host_check.cpp -- the small dense step of bsm_gmres_solve (csrc/bsm_krylov.h: Givens rotations of one Hessenberg
// column, back substitution) on heap buffers, for a run under AddressSanitizer / UBSan on a CPU: every buffer is allocated
// at its exact size (H with leading dimension k + 1 exactly, y of k, res of k, work of 3 k + 1 elements), so an access
// outside an array is an access outside its allocation.  Stand-alone (own main, standard library only):
//   c++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all -I blocksparsematrices.jl_amd/csrc \
//       tools/krylov_host_check.cpp -o krylov_host_check && ./krylov_host_check
// Sizes 1, 2, 20 and BSM_GMRES_MAX_RESTART in the four element types, each also with one exactly zero subdiagonal entry
// (the lucky breakdown) and once as the zero matrix.  Checked without a reference solver: the estimate res[k - 1] against
// the residual || beta e_1 - H y || of the returned y (evaluated in double on the untouched copy of H), and the normal
// equations H^H (beta e_1 - H y) = 0; prints the worst ratios per type and exits non-zero when a check fails.
#include <algorithm>
#include <cmath>
#include <complex>
#include <cstdio>
#include <limits>
#include <random>
#include <vector>

#include "bsm_krylov.h"

namespace {
std::mt19937_64 gen(19);
using cd = std::complex<double>;

template <typename R, int NC> int one(const char *name, int k, int zero_at, bool all_zero, double &worst) {
    std::uniform_real_distribution<double> u(-1, 1), sub(0.1, 1);
    const int ld = k + 1;
    std::vector<R> H((size_t)ld * k * NC, R(0)), y((size_t)k * NC), work((size_t)(3 * k + 1) * NC);
    std::vector<double> res((size_t)k);
    std::vector<cd> ref((size_t)ld * k, cd(0));
    if (!all_zero)
        for (int j = 0; j < k; j++)
            for (int i = 0; i <= j + 1; i++) {
                double re = u(gen) / std::sqrt((double)k) + (i == j ? 2.0 : 0.0), im = NC == 2 ? u(gen) / std::sqrt((double)k) : 0.0;
                if (i == j + 1) re = j == zero_at ? 0.0 : sub(gen), im = 0.0;
                H[((size_t)i + (size_t)j * ld) * NC] = (R)re;
                if (NC == 2) H[((size_t)i + (size_t)j * ld) * NC + NC - 1] = (R)im;
                ref[(size_t)i + (size_t)j * ld] = cd((double)(R)re, (double)(R)im);
            }
    const double beta = 1.75;
    bsm::krylov_lsq_host<R, NC>(k, H.data(), ld, (R)beta, y.data(), res.data(), work.data());
    // r = beta e_1 - H y and H^H r in double
    std::vector<cd> r((size_t)ld, cd(0));
    r[0] = beta;
    double ynorm = 0;
    for (int j = 0; j < k; j++) {
        const cd yj((double)y[(size_t)j * NC], NC == 2 ? (double)y[(size_t)j * NC + NC - 1] : 0.0);
        if (!std::isfinite(yj.real()) || !std::isfinite(yj.imag()) || !std::isfinite(res[(size_t)j])) {
            std::printf("%s k %d: non-finite result\n", name, k);
            return 1;
        }
        ynorm += std::norm(yj);
        for (int i = 0; i <= j + 1; i++) r[(size_t)i] -= ref[(size_t)i + (size_t)j * ld] * yj;
    }
    double rn = 0, ne = 0;
    for (int i = 0; i < ld; i++) rn += std::norm(r[(size_t)i]);
    rn = std::sqrt(rn);
    for (int j = 0; j < k; j++) {
        cd s = 0;
        for (int i = 0; i <= j + 1; i++) s += std::conj(ref[(size_t)i + (size_t)j * ld]) * r[(size_t)i];
        ne = std::max(ne, std::abs(s));
    }
    // backward stability of Givens QR: both within c k eps (|beta| + |H| |y|), |H| <= 4 here, c = 8
    const double scale = 8.0 * k * (double)std::numeric_limits<R>::epsilon() * (beta + 4.0 * std::sqrt(ynorm));
    const double a = std::fabs(res[(size_t)k - 1] - rn) / scale, b = ne / (4.0 * scale);
    worst = std::max(worst, std::max(a, b));
    int bad = !(a <= 1.0) || !(b <= 1.0);
    if (all_zero && res[(size_t)k - 1] != beta) bad = 1;
    if (zero_at >= 0 && !(res[(size_t)zero_at] <= scale)) bad = 1;
    if (bad) std::printf("%s k %d zero_at %d: estimate off by %g, normal equations by %g (bounds 1)\n", name, k, zero_at, a, b);
    return bad;
}

template <typename R, int NC> int run(const char *name) {
    int bad = 0;
    double worst = 0;
    for (int k : {1, 2, 20, BSM_GMRES_MAX_RESTART}) {
        bad += one<R, NC>(name, k, -1, false, worst);
        bad += one<R, NC>(name, k, k / 2, false, worst);
        bad += one<R, NC>(name, k, -1, true, worst);
    }
    std::printf("%s: worst ratio %.3f, %d failed\n", name, worst, bad);
    return bad;
}
}  // namespace

int main() {
    const int bad = run<float, 1>("float32") + run<double, 1>("float64") + run<float, 2>("complex64") + run<double, 2>("complex128");
    return bad ? 1 : 0;
}
