// invert_host_check.cpp -- the host elimination of bsm_invert_blocks (csrc/bsm_invert.h) on heap blocks, for a run
// under AddressSanitizer / UBSan on a CPU: every buffer is allocated at its exact size (leading dimension n + 3, NaN
// padding), so an access outside a block is an access outside its allocation.  Stand-alone (own main, standard library
// only):
//   c++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all -I blocksparsematrices.jl_amd/csrc \
//       tools/invert_host_check.cpp -o invert_host_check && ./invert_host_check
// Sizes 0 .. 257 and the singular cases of tests/test_invert_blocks_cpu.py in the four element types; prints the worst
// max|X B - I| / (n eps max(|X| |B|)) per type and exits non-zero when a check fails.
#include <algorithm>
#include <cmath>
#include <complex>
#include <cstdio>
#include <cstring>
#include <limits>
#include <random>
#include <vector>

#include "bsm_invert.h"

namespace {
std::mt19937_64 gen(18);

template <typename R, int NC> struct Block {
    int64_t n, ld;
    std::vector<R> buf;                      // ld * n elements, exactly
    std::vector<std::complex<double>> ref;   // the n x n values before the call, column-major
    R *at(int64_t i, int64_t j) { return buf.data() + (i + j * ld) * NC; }
};

// B = P (R + n I): R uniform in (-1, 1), P a random row permutation
template <typename R, int NC> Block<R, NC> good(int64_t n) {
    Block<R, NC> b;
    b.n = n, b.ld = n + 3;
    b.buf.assign((size_t)(b.ld * n * NC), std::numeric_limits<R>::quiet_NaN());
    b.ref.assign((size_t)(n * n), 0.0);
    std::uniform_real_distribution<double> u(-1, 1);
    std::vector<int64_t> perm((size_t)n);
    for (int64_t i = 0; i < n; i++) perm[(size_t)i] = i;
    std::shuffle(perm.begin(), perm.end(), gen);
    for (int64_t j = 0; j < n; j++)
        for (int64_t i = 0; i < n; i++) {
            const int64_t src = perm[(size_t)i];
            const R re = (R)(u(gen) + (src == j ? (double)n : 0.0)), im = NC == 2 ? (R)u(gen) : R(0);
            b.at(i, j)[0] = re;
            if (NC == 2) b.at(i, j)[NC - 1] = im;
            b.ref[(size_t)(i + j * n)] = {(double)re, (double)im};
        }
    return b;
}

template <typename R, int NC> double rho(Block<R, NC> &x) {
    const int64_t n = x.n;
    if (n == 0) return 0;
    double res = 0, scale = 0;
    for (int64_t i = 0; i < n; i++)
        for (int64_t j = 0; j < n; j++) {
            std::complex<double> s = 0;
            double a = 0;
            for (int64_t k = 0; k < n; k++) {
                const std::complex<double> v((double)x.at(i, k)[0], NC == 2 ? (double)x.at(i, k)[NC - 1] : 0.0);
                s += v * x.ref[(size_t)(k + j * n)];
                a += std::abs(v) * std::abs(x.ref[(size_t)(k + j * n)]);
            }
            res = std::max(res, std::abs(s - (i == j ? 1.0 : 0.0)));
            scale = std::max(scale, a);
        }
    return res / ((double)n * (double)std::numeric_limits<R>::epsilon() * scale);
}

template <typename R, int NC> bool padding_kept(Block<R, NC> &b) {
    for (int64_t j = 0; j < b.n; j++)
        for (int64_t i = b.n; i < b.ld; i++)
            for (int c = 0; c < NC; c++)
                if (!std::isnan(b.at(i, j)[c])) return false;
    return true;
}

template <typename R, int NC> int run(const char *name) {
    int bad = 0;
    double worst = 0;
    for (int64_t n : {0, 1, 2, 7, 8, 9, 63, 64, 65, 129, 255, 256, 257}) {
        Block<R, NC> b = good<R, NC>(n);
        const int info = bsm::invert_block_host<R, NC>(n ? b.buf.data() : nullptr, n, b.ld);
        const double r = rho(b);
        worst = std::max(worst, r);
        if (info != 0 || !(r <= 4.0) || !padding_kept(b)) bad++, std::printf("%s n %lld: info %d rho %g\n", name, (long long)n, info, r);
    }
    const int64_t n = 9;
    {  // an all-zero block: the first pivot
        Block<R, NC> z = good<R, NC>(n);
        for (int64_t j = 0; j < n; j++) std::memset(z.at(0, j), 0, sizeof(R) * NC * (size_t)n);
        const int info = bsm::invert_block_host<R, NC>(z.buf.data(), n, z.ld);
        if (info != 1 || !padding_kept(z)) bad++, std::printf("%s zero block: info %d\n", name, info);
    }
    {  // one row duplicated: some step runs out of pivots
        Block<R, NC> d = good<R, NC>(n);
        for (int64_t j = 0; j < n; j++) std::memcpy(d.at(5, j), d.at(2, j), sizeof(R) * NC);
        const int info = bsm::invert_block_host<R, NC>(d.buf.data(), n, d.ld);
        if (info < 1 || info > n || !padding_kept(d)) bad++, std::printf("%s duplicated row: info %d\n", name, info);
    }
    {  // a NaN entry
        Block<R, NC> q = good<R, NC>(n);
        q.at(3, 4)[0] = std::numeric_limits<R>::quiet_NaN();
        const int info = bsm::invert_block_host<R, NC>(q.buf.data(), n, q.ld);
        if (info == 0 || !padding_kept(q)) bad++, std::printf("%s NaN entry: info %d\n", name, info);
    }
    std::printf("%s: worst rho %.3f, %d failed\n", name, worst, bad);
    return bad;
}
}  // namespace

int main() {
    const int bad = run<float, 1>("float32") + run<double, 1>("float64") + run<float, 2>("complex64") + run<double, 2>("complex128");
    return bad ? 1 : 0;
}
