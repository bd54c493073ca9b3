// bsm_lobpcg.hip -- the kernels of bsm_block_gram, bsm_block_combine and bsm_lobpcg_* (include/bsm_rocm.h): the two tall-skinny
// products of a block method -- the Gram matrix U^H W on the matrix pipe and the combination V C with a complex C -- and the
// residual pass of LOBPCG.  Kept out of the product kernel units like bsm_eig.hip: the build id names the kernels of the
// PRODUCTS.  (No counterpart in the reference: its operators are LinearMaps handed to a Julia eigensolver package.)
//
//   gram_kernel      grid = gram_grid workgroups of 4 waves; workgroup g owns the rows wg_range(n, G, g).  Per chunk of
//                    gram_chunk_rows rows: the p columns of U and the q of W are read ONCE, one REAL per lane, lanes along the
//                    rows (coalesced, any element alignment), into LDS as lds[plane][column][row] -- a complex column as a plane
//                    of real and one of imaginary parts --; a barrier; then the 16 x 16 tiles of the p x q result are dealt to
//                    the waves (tile t to wave t mod 4, at most 5 each) and every tile takes the chunk through
//                    v_mfma_{f64,f32}_16x16x4 with the ROWS as the K dimension: lane l holds A[i = l & 15][k = l >> 4] =
//                    U[row 4 s + k, column 16 pt + i] and B[k][j = l & 15] = W[row 4 s + k, column 16 qt + j].  Complex types
//                    take four real products: Re += Ur^T Wr + Ui^T Wi, Im += Ur^T Wi - Ui^T Wr.  Columns past p / q are
//                    clamped: they feed only rows / columns of D that are not stored.  The accumulator of lane l, register r is
//                    D[row, column l & 15] with row = (l >> 4) + 4 r for f64 and 4 (l >> 4) + r for f32.  A chunk's sum is the
//                    chain of its MFMAs in the working precision; the chunks' sums are added in double in registers, and the
//                    workgroup leaves ONE partial p x q matrix, rounded once to the working precision.
//   gram_sum_kernel  one thread per entry adds the partials over g ascending in double.
//   bcombine_kernel  combine_kernel of bsm_eig.hip for complex columns and a complex C: a tile of rows x p elements through
//                    LDS, all reads of a tile in front of the barrier (Out == V works), a thread owns one row and four output
//                    columns, j ascending with re = fma(vr, cr, re), re = fma(-vi, ci, re), im = fma(vr, ci, im),
//                    im = fma(vi, cr, im) per term: fixed to the bit whatever the geometry.
//   lob_resid_kernel grid (krylov_grid, k): R = AX - theta X on a row range, one partial of ||R_c||^2 per workgroup and column;
//                    lob_resid_sum_kernel: one wave per column adds them in a fixed order and takes the root.
// No floating-point atomic, and no workgroup waits for another.
#include "bsm_lobpcg.h"

#include "../../include/bsm_rocm.h"
#include "bsm_lockstep_device.h"

namespace bsm {
namespace {

// the two accumulator shapes of v_mfma_{f64,f32}_16x16x4 (mfma16 of bsm_device.h, whose 16-byte vector type collides with the
// solver units' own: this unit takes the access of bsm_lockstep_device.h)
typedef double v4f64 __attribute__((ext_vector_type(4)));
typedef float v4f32 __attribute__((ext_vector_type(4)));
__device__ __forceinline__ v4f64 mfma16(double a, double b, v4f64 c) { return __builtin_amdgcn_mfma_f64_16x16x4f64(a, b, c, 0, 0, 0); }
__device__ __forceinline__ v4f32 mfma16(float a, float b, v4f32 c) { return __builtin_amdgcn_mfma_f32_16x16x4f32(a, b, c, 0, 0, 0); }
template <typename R> struct GramT;
template <> struct GramT<float> { using V4 = v4f32; };
template <> struct GramT<double> { using V4 = v4f64; };

constexpr int kGramPad = 4;        // rows of padding of a staged column
constexpr int kGramWaveTiles = 5;  // ceil(3 * 6 / 4): tiles of one wave at p = 48, q = 96

template <typename R, int NC, int KC>
__global__ void __launch_bounds__(kGramThreads)
    gram_kernel(long long n, int p, int q, const R *__restrict__ U, long long ldu, const R *__restrict__ W, long long ldw,
                R *__restrict__ part) {
    using V4 = typename GramT<R>::V4;
    constexpr int LDK = KC + kGramPad;
    constexpr bool F64MAP = sizeof(R) == 8;
    extern __shared__ __attribute__((aligned(16))) char smem[];
    R *const lds = reinterpret_cast<R *>(smem);  // lds[(plane * (p + q) + column) * LDK + row], U's columns first
    const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
    const int ln = lane & 15, lk = lane >> 4;
    const int cols = p + q, npt = (p + 15) >> 4, nqt = (q + 15) >> 4, ntiles = npt * nqt;
    const long long plane = (long long)cols * LDK;
    long long i0, i1;
    wg_range(n, gridDim.x, blockIdx.x, i0, i1);
    // the sum over the chunks: in double.  A chunk's own sum is the chain of KC / 4 MFMAs in the working precision; for the
    // single types a chain over the whole row range (up to 2048 rows) would leave an error of some sqrt(rows) eps in a Gram
    // entry, which is the size of a single-precision tolerance of the eigensolver (docs/experiments_r37.md)
    v4f64 acc[kGramWaveTiles][NC];
#pragma unroll
    for (int m = 0; m < kGramWaveTiles; ++m)
#pragma unroll
        for (int c = 0; c < NC; ++c) acc[m][c] = v4f64{0.0, 0.0, 0.0, 0.0};
    constexpr int CR = KC * NC;  // reals of one column of a chunk
    for (long long r0 = i0; r0 < i1; r0 += KC) {
        const int nrw = (int)(i1 - r0 < KC ? i1 - r0 : KC);
        for (int idx = t; idx < cols * CR; idx += kGramThreads) {
            const int col = idx / CR, e = idx - col * CR;
            const int row = e / NC, pl = e - row * NC;
            const R *src = col < p ? U + (long long)col * ldu * NC : W + (long long)(col - p) * ldw * NC;
            lds[pl * plane + col * LDK + row] = row < nrw ? src[(r0 + row) * NC + pl] : R(0);
        }
        __syncthreads();
#pragma unroll
        for (int m = 0; m < kGramWaveTiles; ++m) {
            const int tl = wave + 4 * m;  // (wave-uniform)
            if (tl < ntiles) {
                const int pt = tl / nqt, qt = tl - pt * nqt;
                const int uc = min(pt * 16 + ln, p - 1), wc = p + min(qt * 16 + ln, q - 1);
                const R *ua = lds + uc * LDK + lk, *wb = lds + wc * LDK + lk;
                V4 ch[NC];
#pragma unroll
                for (int c = 0; c < NC; ++c) ch[c] = V4{R(0), R(0), R(0), R(0)};
#pragma unroll 4
                for (int s = 0; s < KC; s += 4) {
                    const R ur = ua[s], wr = wb[s];
                    ch[0] = mfma16(ur, wr, ch[0]);
                    if constexpr (NC == 2) {
                        const R ui = ua[plane + s], wi = wb[plane + s];
                        ch[0] = mfma16(ui, wi, ch[0]);
                        ch[1] = mfma16(ur, wi, ch[1]);
                        ch[1] = mfma16(-ui, wr, ch[1]);
                    }
                }
#pragma unroll
                for (int c = 0; c < NC; ++c)
#pragma unroll
                    for (int r = 0; r < 4; ++r) acc[m][c][r] += (double)ch[c][r];
            }
        }
        __syncthreads();  // the next chunk overwrites the LDS this one read
    }
    R *const out = part + (long long)blockIdx.x * p * q * NC;
#pragma unroll
    for (int m = 0; m < kGramWaveTiles; ++m) {
        const int tl = wave + 4 * m;
        if (tl < ntiles) {
            const int pt = tl / nqt, qt = tl - pt * nqt;
            const int j = qt * 16 + ln;
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int i = pt * 16 + (F64MAP ? lk + 4 * r : 4 * lk + r);
                if (i < p && j < q) {
#pragma unroll
                    for (int c = 0; c < NC; ++c) out[((long long)j * p + i) * NC + c] = (R)acc[m][c][r];
                }
            }
        }
    }
}

template <typename R, int NC>
__global__ void __launch_bounds__(256) gram_sum_kernel(int G, int p, int q, const R *__restrict__ part, double *__restrict__ Gm, long long ldg) {
    const int idx = blockIdx.x * 256 + threadIdx.x;
    if (idx >= p * q) return;
    const int j = idx / p, i = idx - j * p;
    double s[NC];
#pragma unroll
    for (int c = 0; c < NC; ++c) s[c] = 0.0;
    for (int g = 0; g < G; ++g) {
#pragma unroll
        for (int c = 0; c < NC; ++c) s[c] += (double)part[((long long)g * p * q + idx) * NC + c];
    }
#pragma unroll
    for (int c = 0; c < NC; ++c) Gm[((long long)j * ldg + i) * NC + c] = s[c];
}

constexpr int kBC = 4;  // output columns per thread and pass over the tile

template <typename R>
__global__ void __launch_bounds__(kEigThreads)
    bcombine_kernel(long long n, int p, int q, const R *V, long long ldv, const R *__restrict__ C, long long ldc, R *Out, long long ldo,
                    int rows) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    R *const tile = reinterpret_cast<R *>(smem);  // tile[(j * rows + r) * 2 + part]
    const int t = threadIdx.x;
    const long long ntiles = (n + rows - 1) / rows;
    const int ncg = (q + kBC - 1) / kBC, rr = 2 * rows;
    for (long long tl = blockIdx.x; tl < ntiles; tl += gridDim.x) {
        const long long r0 = tl * rows;
        const int nrw = (int)(n - r0 < rows ? n - r0 : rows);
        // (V carries no restrict: in place it is Out.  A column of the tile is walked as 2 rows reals, one per lane)
        for (int idx = t; idx < p * rr; idx += kEigThreads) {
            const int j = idx / rr, e = idx - j * rr;
            tile[idx] = e < 2 * nrw ? V[((long long)j * ldv + r0) * 2 + e] : R(0);
        }
        __syncthreads();
        const int items = rows * ncg;
        for (int idx = t; idx < items; idx += kEigThreads) {
            // rows is a multiple of 64: a wave's 64 items share their column group
            const int cg = __builtin_amdgcn_readfirstlane(idx / rows);
            const int r = idx - cg * rows, c0 = cg * kBC;
            const R *cc[kBC];
#pragma unroll
            for (int k = 0; k < kBC; ++k) cc[k] = C + (long long)(c0 + k < q ? c0 + k : q - 1) * ldc * 2;
            R re[kBC], im[kBC];
#pragma unroll
            for (int k = 0; k < kBC; ++k) re[k] = im[k] = R(0);
            for (int j = 0; j < p; ++j) {
                const R vr = tile[(j * rows + r) * 2], vi = tile[(j * rows + r) * 2 + 1];
#pragma unroll
                for (int k = 0; k < kBC; ++k) {
                    const R cr = cc[k][2 * j], ci = cc[k][2 * j + 1];
                    re[k] = fma(vr, cr, re[k]);
                    re[k] = fma(-vi, ci, re[k]);
                    im[k] = fma(vr, ci, im[k]);
                    im[k] = fma(vi, cr, im[k]);
                }
            }
            if (r < nrw) {
#pragma unroll
                for (int k = 0; k < kBC; ++k)
                    if (c0 + k < q) {
                        R *o = Out + ((long long)(c0 + k) * ldo + r0 + r) * 2;
                        o[0] = re[k];
                        o[1] = im[k];
                    }
            }
        }
        __syncthreads();  // the next tile overwrites the LDS this one read
    }
}

template <typename R>
__global__ void __launch_bounds__(kThreads) lob_resid_kernel(long long nr, const R *__restrict__ AX, long long ldax, const R *__restrict__ X,
                                                             long long ldx, const R *__restrict__ theta, R *__restrict__ Rm, long long ldr,
                                                             R *__restrict__ part) {
    __shared__ R red[4][1];
    const int G = gridDim.x, g = blockIdx.x, c = blockIdx.y;
    const R th = theta[c];
    const R *q = AX + (long long)c * ldax, *x = X + (long long)c * ldx;
    R *o = Rm + (long long)c * ldr;
    long long i0, i1;
    wg_range(nr, G, g, i0, i1);
    R s[1] = {R(0)};
    for (long long i = i0 + threadIdx.x; i < i1; i += kThreads) {
        const R d = fma(-th, x[i], q[i]);
        o[i] = d;
        s[0] = fma(d, d, s[0]);
    }
    block_sum<R, 1>(s, red);
    if (threadIdx.x == 0) part[(long long)c * G + g] = s[0];
}

template <typename R> __global__ void __launch_bounds__(64) lob_resid_sum_kernel(int G, const R *__restrict__ part, double *__restrict__ res) {
    const int c = blockIdx.x;
    const R a = wave_total(part + (long long)c * G, G, 1, (int)threadIdx.x);
    if (threadIdx.x == 0) res[c] = sqrt((double)a);
}

}  // namespace

hipError_t launch_block_gram(int dtype, long long n, int p, const void *U, long long ldu, int q, const void *W, long long ldw, void *G,
                             long long ldg, void *part, hipStream_t stream) {
    if (!is_vec_type(dtype) || n < 0 || p < 1 || p > kGramMaxP || q < 1 || q > kGramMaxQ || ldg < p) return hipErrorInvalidValue;
    const int grid = gram_grid(dtype, n);
    with_types(dtype, [&](auto r, auto, auto nc) {
        using R = decltype(r);
        constexpr int NC = decltype(nc)::value;
        constexpr int KC = gram_chunk_rows((int)sizeof(R), NC);
        const size_t lds_bytes = (size_t)(p + q) * NC * (KC + kGramPad) * sizeof(R);
        hipLaunchKernelGGL((gram_kernel<R, NC, KC>), dim3((unsigned)grid), dim3(kGramThreads), lds_bytes, stream, n, p, q, (const R *)U, ldu,
                           (const R *)W, ldw, (R *)part);
        hipLaunchKernelGGL((gram_sum_kernel<R, NC>), dim3((unsigned)((p * q + 255) / 256)), dim3(256), 0, stream, grid, p, q, (const R *)part,
                           (double *)G, ldg);
    });
    return hipGetLastError();
}

hipError_t launch_block_combine_complex(int dtype, long long n, int p, int q, const void *V, long long ldv, const void *C, long long ldc,
                                        void *Out, long long ldo, hipStream_t stream) {
    if ((dtype != BSM_C64 && dtype != BSM_C128) || n < 0 || p < 1 || p > kGramMaxP || q < 0 || q > p) return hipErrorInvalidValue;
    if (n == 0 || q == 0) return hipSuccess;
    const int es = elem_bytes(dtype), rows = block_combine_tile_complex(p, es);
    const long long ntiles = (n + rows - 1) / rows;
    const size_t lds_bytes = (size_t)p * rows * es;
    const dim3 grid((unsigned)std::min<long long>(ntiles, 2048)), block(kEigThreads);
    hipError_t e = hipSuccess;
    with_types(dtype, [&](auto r, auto, auto) {
        using R = decltype(r);
        if (lds_bytes > 65536) {
            e = hipFuncSetAttribute(reinterpret_cast<const void *>(&bcombine_kernel<R>), hipFuncAttributeMaxDynamicSharedMemorySize,
                                    (int)lds_bytes);
            if (e != hipSuccess) return;
        }
        hipLaunchKernelGGL(bcombine_kernel<R>, grid, block, lds_bytes, stream, n, p, q, (const R *)V, ldv, (const R *)C, ldc, (R *)Out, ldo,
                           rows);
    });
    return e != hipSuccess ? e : hipGetLastError();
}

hipError_t launch_lob_resid(int dtype, long long n, int k, const void *AX, long long ldax, const void *X, long long ldx, const void *theta,
                            void *Rm, long long ldr, void *part, double *res, hipStream_t stream) {
    if (!is_vec_type(dtype) || n < 0 || k < 1 || k > kCgMaxRhs) return hipErrorInvalidValue;
    const int es = elem_bytes(dtype), G = krylov_grid(n, es);
    with_types(dtype, [&](auto r, auto, auto ncv) {
        using R = decltype(r);
        constexpr int nc = decltype(ncv)::value;
        hipLaunchKernelGGL(lob_resid_kernel<R>, dim3((unsigned)G, (unsigned)k), dim3(kThreads), 0, stream, n * nc, (const R *)AX, ldax * nc,
                           (const R *)X, ldx * nc, (const R *)theta, (R *)Rm, ldr * nc, (R *)part);
        hipLaunchKernelGGL(lob_resid_sum_kernel<R>, dim3((unsigned)k), dim3(64), 0, stream, G, (const R *)part, res);
    });
    return hipGetLastError();
}

}  // namespace bsm
