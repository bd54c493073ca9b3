// bsm_invert.hip -- invert_kernel (bsm_invert_blocks, include/bsm_rocm.h): a batch of dense blocks of different sizes,
// each inverted in place by one workgroup.  Kept out of the product kernel units like bsm_extract.hip: the build id
// (Makefile BUILD_ID) names the kernels and schedule of the PRODUCTS, and a setup-time inverse changes neither.
#include "bsm_device.h"

namespace bsm {

// ========================================================================================
// Gauss-Jordan elimination with partial row pivoting, the elimination of bsm_invert.h step by step (so that host and
// device choose the same pivots): one 256-thread workgroup per block, n steps, three phases per step with a
// __syncthreads() behind each.
//   search  every thread scans the rows k + t, k + t + 256, ... of column k; the wave's arg-max by 6 xor-shuffles, its
//           lane 0 leaves (magnitude, row, value) in LDS; behind the barrier every thread folds the four records the
//           same way, so all 256 agree on the pivot row p and its value without another barrier.  Larger magnitude
//           wins, ties go to the smaller row, a NaN counts as +inf: the result does not depend on the order of the fold.
//   pivot   thread j swaps A[k, j] and A[p, j] and scales the new row k by r = 1 / pivot (A[k, k] = r); the row as it was
//           before the scaling is staged in LDS (prow, with prow[k] = 1), and so are the multipliers of the other rows
//           (pcol[i] = A[i, k] / pivot, a true division; A[i, k] is then zeroed: the update below leaves -pcol[i]
//           there).  No two threads touch one entry.
//   update  A[i, j] -= pcol[i] * prow[j] for i != k, LANES ALONG THE ROWS -- the contiguous direction of a column-major
//           block: a thread keeps row i = t mod P (P = n rounded up to a power of two, at most 256) and walks the
//           columns t / P, t / P + 256 / P, ..., U loads in flight before the first store.
// Every entry has one writer per phase and the order of the arithmetic is fixed: the result is bit-identical from run
// to run.  A zero or non-finite pivot is seen by all 256 threads alike: thread 0 writes info = k + 1 and the workgroup
// leaves (the block is then unspecified: partly eliminated in place, or untouched when it lived in LDS).
// Two regimes, one instantiation each (the host splits its launches at the seam):
//   RES   n * n * sizeof(T) <= BSM_INVERT_LDS_BYTES (128 KiB of the CU's 160 KiB; the staging arrays below need
//         less than 8 KiB more): the block is loaded into LDS (leading dimension n), eliminated there, and written back
//         with the column swaps applied on the way out (perm: the swaps of piv played backwards over the identity).
//   !RES  up to n = 1024: eliminated in place in global memory with PLAIN loads and stores -- the waves of the workgroup
//         re-read each other's writes behind every barrier, which the streaming (nontemporal) helpers of bsm_device.h
//         are not made for --, then the column swaps are undone one by one.
// Dynamic LDS, every offset a multiple of 16 (invert_lds): the four search records, prow, pcol, piv, perm, the block.
// ========================================================================================
template <typename T> struct RealOf {
    using type = T;
};
template <> struct RealOf<c64> {
    using type = float;
};
template <> struct RealOf<c128> {
    using type = double;
};

// |v|, |re| + |im| (cabs1); NaN -> +inf so that the arg-max is a total order
__device__ __forceinline__ float pivot_mag(float v) {
    const float m = fabsf(v);
    return m != m ? INFINITY : m;
}
__device__ __forceinline__ double pivot_mag(double v) {
    const double m = fabs(v);
    return m != m ? (double)INFINITY : m;
}
__device__ __forceinline__ float pivot_mag(c64 v) { return pivot_mag(fabsf(v.re) + fabsf(v.im)); }
__device__ __forceinline__ double pivot_mag(c128 v) { return pivot_mag(fabs(v.re) + fabs(v.im)); }

__device__ __forceinline__ bool bad_pivot(float v) { return v == 0.f || !isfinite(v); }
__device__ __forceinline__ bool bad_pivot(double v) { return v == 0.0 || !isfinite(v); }
__device__ __forceinline__ bool bad_pivot(c64 v) { return (v.re == 0.f && v.im == 0.f) || !isfinite(v.re) || !isfinite(v.im); }
__device__ __forceinline__ bool bad_pivot(c128 v) { return (v.re == 0.0 && v.im == 0.0) || !isfinite(v.re) || !isfinite(v.im); }

// 1 / pivot; complex: scaled by |re| + |im| first (invert_recip of bsm_invert.h)
__device__ __forceinline__ float recip(float v) { return 1.f / v; }
__device__ __forceinline__ double recip(double v) { return 1.0 / v; }
template <typename C, typename R> __device__ __forceinline__ C recip_c(C v) {
    const R s = fabs(v.re) + fabs(v.im);
    const R a = v.re / s, b = v.im / s;
    const R d = a * a + b * b;
    return C{a / d / s, -b / d / s};
}
__device__ __forceinline__ c64 recip(c64 v) { return recip_c<c64, float>(v); }
__device__ __forceinline__ c128 recip(c128 v) { return recip_c<c128, double>(v); }

// f / pivot, the multiplier of a row.  A true division, complex ones by the textbook formula on operands scaled by
// |re| + |im| of the pivot and WITHOUT contraction into FMAs: f == pivot gives exactly 1 (+ 0 i), so a row that duplicates
// the pivot row cancels exactly and the block is reported singular instead of being inverted into noise
__device__ __forceinline__ float pivot_div(float f, float p) { return f / p; }
__device__ __forceinline__ double pivot_div(double f, double p) { return f / p; }
template <typename C, typename R> __device__ __forceinline__ C pivot_div_c(C f, C p) {
#pragma clang fp contract(off)
    const R s = fabs(p.re) + fabs(p.im);
    const R a = f.re / s, b = f.im / s, c = p.re / s, d = p.im / s;
    const R den = c * c + d * d;
    return C{(a * c + b * d) / den, (b * c - a * d) / den};
}
__device__ __forceinline__ c64 pivot_div(c64 f, c64 p) { return pivot_div_c<c64, float>(f, p); }
__device__ __forceinline__ c128 pivot_div(c128 f, c128 p) { return pivot_div_c<c128, double>(f, p); }

__device__ __forceinline__ float one_of(float) { return 1.f; }
__device__ __forceinline__ double one_of(double) { return 1.0; }
__device__ __forceinline__ c64 one_of(c64) { return c64{1.f, 0.f}; }
__device__ __forceinline__ c128 one_of(c128) { return c128{1.0, 0.0}; }

// a - f * b
__device__ __forceinline__ float sub_mul(float a, float f, float b) { return fmaf(-f, b, a); }
__device__ __forceinline__ double sub_mul(double a, double f, double b) { return fma(-f, b, a); }
template <typename C> __device__ __forceinline__ C sub_mul_c(C a, C f, C b) { return madd(a, C{-f.re, -f.im}, b); }
__device__ __forceinline__ c64 sub_mul(c64 a, c64 f, c64 b) { return sub_mul_c(a, f, b); }
__device__ __forceinline__ c128 sub_mul(c128 a, c128 f, c128 b) { return sub_mul_c(a, f, b); }

template <typename T, bool RES>
__global__ void __launch_bounds__(256) invert_kernel(const InvertBlock *__restrict__ table, int *__restrict__ info, int nmax) {
    using R = typename RealOf<T>::type;
    constexpr int U = sizeof(T) == 16 ? 4 : 8;  // loads in flight per thread in the update
    constexpr int kNone = 0x7fffffff;
    extern __shared__ __attribute__((aligned(16))) char smem[];
    const InvertBlock *const blk = table + blockIdx.x;  // (field by field: a copy of the record would reserve scratch)
    const int n = blk->n, id = blk->id, t = threadIdx.x, lane = t & 63, wave = t >> 6;
    const long long ldg = blk->ld;
    T *const Gm = reinterpret_cast<T *>(blk->ptr);
    const InvertLds lo = invert_lds(nmax, (int)sizeof(T), RES);
    T *const pval = reinterpret_cast<T *>(smem);
    R *const pmag = reinterpret_cast<R *>(smem + 64);
    int *const pidx = reinterpret_cast<int *>(smem + 96);
    T *const prow = reinterpret_cast<T *>(smem + lo.prow);
    T *const pcol = reinterpret_cast<T *>(smem + lo.pcol);
    int *const piv = reinterpret_cast<int *>(smem + lo.piv);
    int *const perm = reinterpret_cast<int *>(smem + lo.perm);
    T *const A = RES ? reinterpret_cast<T *>(smem + lo.mat) : Gm;
    const long long lda = RES ? (long long)n : ldg;
    int P = 1, lg = 0;
    while (P < n && P < 256) P <<= 1, ++lg;
    const int NG = 256 >> lg, ti = t & (P - 1), tg = t >> lg;

    if constexpr (RES) {
        for (int i = ti; i < n; i += P)
            for (int j = tg; j < n; j += NG) A[i + j * lda] = Gm[i + j * ldg];
        __syncthreads();
    }

    for (int k = 0; k < n; ++k) {
        // ---- search
        R bm = R(-1);
        int bi = kNone;
        for (int i = k + t; i < n; i += 256) {
            const R m = pivot_mag(A[i + k * lda]);
            if (m > bm) bm = m, bi = i;
        }
#pragma unroll
        for (int d = 32; d >= 1; d >>= 1) {
            const R om = __shfl_xor(bm, d, 64);
            const int oi = __shfl_xor(bi, d, 64);
            if (om > bm || (om == bm && oi < bi)) bm = om, bi = oi;
        }
        if (lane == 0) {
            pmag[wave] = bm;
            pidx[wave] = bi;
            if (bi != kNone) pval[wave] = A[bi + k * lda];
        }
        __syncthreads();
        int p = pidx[0], pw = 0;
        R pm = pmag[0];
#pragma unroll
        for (int w = 1; w < 4; ++w) {
            const R om = pmag[w];
            const int oi = pidx[w];
            if (om > pm || (om == pm && oi < p)) pm = om, p = oi, pw = w;
        }
        const T pv = pval[pw];
        if (bad_pivot(pv)) {  // uniform: every thread read the same records
            if (t == 0) info[id] = k + 1;
            return;
        }
        // ---- pivot
        const T r = recip(pv);
        if (t == 0) piv[k] = p;
        for (int j = t; j < n; j += 256) {
            const T a = A[p + j * lda], b = A[k + j * lda];
            const T v = j == k ? r : mul(a, r);
            if (p != k) A[p + j * lda] = j == k ? zero_of(T{}) : b;
            A[k + j * lda] = v;
            prow[j] = j == k ? one_of(T{}) : a;
            if (j == k && p != k) pcol[p] = pivot_div(b, pv);  // row p now holds the old row k, A[k, k] is its entry here
        }
        for (int i = t; i < n; i += 256)
            if (i != k && i != p) {
                pcol[i] = pivot_div(A[i + k * lda], pv);
                A[i + k * lda] = zero_of(T{});
            }
        __syncthreads();
        // ---- update
        for (int i = ti; i < n; i += P) {
            if (i == k) continue;
            const T f = pcol[i];
            T *const Ai = A + i;
            for (int j0 = tg; j0 < n; j0 += NG * U) {
                T v[U];
#pragma unroll
                for (int u = 0; u < U; ++u) {
                    const int j = j0 + u * NG;
                    v[u] = j < n ? Ai[j * lda] : zero_of(T{});
                }
#pragma unroll
                for (int u = 0; u < U; ++u) {
                    const int j = j0 + u * NG;
                    if (j < n) Ai[j * lda] = sub_mul(v[u], f, prow[j]);
                }
            }
        }
        __syncthreads();
    }

    if constexpr (RES) {
        if (t == 0) {
            for (int c = 0; c < n; ++c) perm[c] = c;
            for (int k = n - 1; k >= 0; --k) {
                const int p = piv[k], a = perm[k];
                perm[k] = perm[p];
                perm[p] = a;
            }
        }
        __syncthreads();
        for (int i = ti; i < n; i += P)
            for (int j = tg; j < n; j += NG) Gm[i + j * ldg] = A[i + perm[j] * lda];
    } else {
        for (int k = n - 1; k >= 0; --k) {
            const int p = piv[k];
            if (p == k) continue;
            for (int i = t; i < n; i += 256) {  // (by real components: a 16-byte element swapped whole goes through scratch)
                R *const x = reinterpret_cast<R *>(A + (i + k * lda)), *const y = reinterpret_cast<R *>(A + (i + p * lda));
#pragma unroll
                for (int c = 0; c < (int)(sizeof(T) / sizeof(R)); ++c) {
                    const R a = x[c], b = y[c];
                    x[c] = b;
                    y[c] = a;
                }
            }
            __syncthreads();
        }
    }
    if (t == 0) info[id] = 0;
}

hipError_t launch_invert(int dtype, const void *d_table, long long count, int nmax, bool resident, void *d_info,
                         hipStream_t stream) {
    if (count <= 0) return hipSuccess;
    const dim3 grid((unsigned)count), block(256);
    return with_pair(dtype, dtype, [&](auto t, auto) {  // (the same-type pair of dtype: its T)
        using T = decltype(t);
        const size_t lds = (size_t)invert_lds(nmax, (int)sizeof(T), resident).total;
        if (resident) {
            if (lds > 65536) {
                const hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void *>(&invert_kernel<T, true>),
                                                         hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
                if (e != hipSuccess) return e;
            }
            hipLaunchKernelGGL((invert_kernel<T, true>), grid, block, lds, stream, (const InvertBlock *)d_table, (int *)d_info, nmax);
        } else {
            hipLaunchKernelGGL((invert_kernel<T, false>), grid, block, lds, stream, (const InvertBlock *)d_table, (int *)d_info, nmax);
        }
        return hipGetLastError();
    });
}

}  // namespace bsm
