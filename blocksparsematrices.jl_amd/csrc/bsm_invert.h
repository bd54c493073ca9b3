// bsm_invert.h -- the host side of bsm_invert_blocks (include/bsm_rocm.h): in-place inverse of one dense column-major
// block by Gauss-Jordan elimination with partial row pivoting, the elimination invert_kernel (bsm_invert.hip) runs on
// the device, written down once more in plain C++ so that both choose the same pivots.  Depends on the standard
// library only: bsm_invert.cpp calls it for BSM_MEM_HOST, and a stand-alone program can include it.
//
// The elimination, step k = 0 .. n-1:
//   1. pivot = the entry of column k in rows k .. n-1 with the largest magnitude (|v| for real, |re| + |im| for complex:
//      LAPACK's cabs1; a NaN counts as +inf), ties to the smallest row; that row and row k are swapped;
//   2. a pivot that is exactly zero or not finite ends the block: info = k + 1;
//   3. every other row i is reduced by a rank-1 update with its multiplier l = A[i, k] / pivot (a true division: a row
//      that duplicates the pivot row has l = 1 and cancels exactly): A[i, j] -= l * A[k, j] for j != k, A[i, k] = -l;
//   4. row k is scaled by r = 1 / pivot, its entry in column k becomes r.
// After the last step the row swaps are undone as column swaps, in reverse order.
#pragma once
#include <cmath>
#include <cstdint>
#include <vector>

namespace bsm {

// 1 / (re + i im), scaled by the magnitude the pivot search used so that re^2 + im^2 neither overflows nor underflows
template <typename R> inline void invert_recip(R re, R im, R &ore, R &oim) {
    const R s = std::fabs(re) + std::fabs(im);
    const R a = re / s, b = im / s;
    const R d = a * a + b * b;
    ore = a / d / s;
    oim = -b / d / s;
}

// f / pivot of complex numbers by the textbook formula on operands scaled the same way, without contraction into FMAs:
// f == pivot gives exactly 1 + 0 i
template <typename R> inline void invert_div(R fre, R fim, R pre, R pim, R &ore, R &oim) {
#ifdef __clang__
#pragma clang fp contract(off)
#endif
    const R s = std::fabs(pre) + std::fabs(pim);
    const R a = fre / s, b = fim / s, c = pre / s, d = pim / s;
    const R den = c * c + d * d;
    ore = (a * c + b * d) / den;
    oim = (b * c - a * d) / den;
}

// a: n x n block of R (NC = 1) or of interleaved (re, im) pairs of R (NC = 2), column-major, leading dimension ld
// elements.  Returns 0 (a holds its inverse) or the 1-based step whose pivot was zero or not finite (a is then
// partly eliminated).  Writes nothing outside the n x n window.
template <typename R, int NC> int invert_block_host(R *a, int64_t n, int64_t ld) {
    if (n <= 0) return 0;
    auto at = [&](int64_t i, int64_t j) { return a + (i + j * ld) * NC; };
    std::vector<int64_t> piv((size_t)n);
    std::vector<R> prow((size_t)n * NC), pcol((size_t)n * NC);
    for (int64_t k = 0; k < n; k++) {
        int64_t p = k;
        R best = -1;
        for (int64_t i = k; i < n; i++) {
            const R *v = at(i, k);
            R mag = std::fabs(v[0]) + (NC == 2 ? std::fabs(v[NC - 1]) : R(0));
            if (std::isnan(mag)) mag = INFINITY;
            if (mag > best) best = mag, p = i;
        }
        const R pre = at(p, k)[0], pim = NC == 2 ? at(p, k)[NC - 1] : R(0);
        if (!std::isfinite(pre) || !std::isfinite(pim) || (pre == 0 && pim == 0)) return (int)(k + 1);
        piv[(size_t)k] = p;
        R rre, rim = 0;
        if (NC == 2)
            invert_recip(pre, pim, rre, rim);
        else
            rre = R(1) / pre;
        // the multipliers of the other rows as they stand after the swap; column k is taken as zero from here on
        for (int64_t i = 0; i < n; i++) {
            if (i == k) continue;
            R *v = at(i == p ? k : i, k);  // row p receives row k
            if (NC == 2)
                invert_div(v[0], v[NC - 1], pre, pim, pcol[(size_t)i * NC], pcol[(size_t)i * NC + NC - 1]);
            else
                pcol[(size_t)i * NC] = v[0] / pre;
            for (int c = 0; c < NC; c++) v[c] = 0;
        }
        // swap rows k and p, scale the pivot row (prow: as it was before the scaling, 1 in column k)
        for (int64_t j = 0; j < n; j++) {
            R *vk = at(k, j), *vp = at(p, j);
            R are = vp[0], aim = NC == 2 ? vp[NC - 1] : R(0);
            if (p != k)
                for (int c = 0; c < NC; c++) vp[c] = vk[c];
            prow[(size_t)j * NC] = j == k ? R(1) : are;
            if (NC == 2) prow[(size_t)j * NC + NC - 1] = j == k ? R(0) : aim;
            if (j == k) {
                are = rre, aim = rim;
            } else if (NC == 2) {
                const R x = are * rre - aim * rim, y = are * rim + aim * rre;
                are = x, aim = y;
            } else {
                are *= rre;
            }
            vk[0] = are;
            if (NC == 2) vk[NC - 1] = aim;
        }
        // rank-1 update of every other row
        for (int64_t j = 0; j < n; j++) {
            const R bre = prow[(size_t)j * NC], bim = NC == 2 ? prow[(size_t)j * NC + NC - 1] : R(0);
            for (int64_t i = 0; i < n; i++) {
                if (i == k) continue;
                R *v = at(i, j);
                const R fre = pcol[(size_t)i * NC];
                if (NC == 2) {
                    const R fim = pcol[(size_t)i * NC + NC - 1];
                    v[0] = v[0] - fre * bre + fim * bim;
                    v[NC - 1] = v[NC - 1] - fre * bim - fim * bre;
                } else {
                    v[0] -= fre * bre;
                }
            }
        }
    }
    for (int64_t k = n - 1; k >= 0; k--) {
        const int64_t p = piv[(size_t)k];
        if (p == k) continue;
        for (int64_t i = 0; i < n; i++)
            for (int c = 0; c < NC; c++) {
                const R t = at(i, k)[c];
                at(i, k)[c] = at(i, p)[c];
                at(i, p)[c] = t;
            }
    }
    return 0;
}

}  // namespace bsm
