// bsm_eig.hip -- the kernels of bsm_krylov_combine and bsm_eigsh_* (include/bsm_rocm.h): the in-place compression of a tall
// basis by a small real matrix (the thick restart, and the way Ritz vectors leave the solver), the guarded scale of a new
// Lanczos vector, the gather of diag(H) and beta for the one copy a cycle ends with, and the true-residual pass over several
// columns.  Kept out of the product kernel units like bsm_krylov.hip: the build id names the kernels of the PRODUCTS.
// (No counterpart in the reference: its operators are LinearMaps handed to KrylovKit's eigsolve.)
//
// Everything here walks REAL components: the projected matrix of a Hermitian operator is real symmetric, so S, theta and
// the scale factor are real and a complex column of n entries is a real one of 2 n.  Two instantiations per kernel.
//
//   combine_kernel  a workgroup owns tiles of `rows` rows (combine_tile_reals of bsm_eig.h: rows x m reals fit into 128 KiB of
//                   LDS).  Per tile: the m columns of those rows are read ONCE, column by column, lanes along the rows
//                   (coalesced), into LDS; the carried column's rows into registers; a barrier; then every thread owns one
//                   row and four output columns at a time, walks j = 0 .. m - 1 with one LDS read and four fmas per j -- the
//                   entries of S come through the scalar unit, the column group is uniform in a wave -- and stores.  A row
//                   of the output depends on the same row of V only and all reads of a tile are in front of the barrier, so
//                   Out == V works.  Every access is one real per lane: any element alignment is served by the same code.
//                   The sum over j is sequential, one fma per term: the result is fixed to the bit.
//   resid_kernel    grid (krylov_grid, columns): d = Q - theta X on a row range, one partial of sum d^2 per workgroup and
//                   column; resid_sum_kernel: one wave per column adds the partials in a fixed order and takes the root.
// No floating-point atomic, and no workgroup waits for another.
#include "bsm_eig.h"

#include "../../include/bsm_rocm.h"
#include "bsm_lockstep_device.h"

namespace bsm {
namespace {

constexpr int kCC = 4;  // output columns per thread and pass over the tile

template <typename R>
__global__ void __launch_bounds__(kEigThreads)
    combine_kernel(long long nr, int m, int k, const R *V, long long ldv, const R *__restrict__ S, long long lds, R *Out,
                   long long ldo, int carry, int rows) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    R *const tile = reinterpret_cast<R *>(smem);  // tile[j * rows + r]
    const int t = threadIdx.x;
    const long long ntiles = (nr + rows - 1) / rows;
    const int ncg = (k + kCC - 1) / kCC;
    for (long long tl = blockIdx.x; tl < ntiles; tl += gridDim.x) {
        const long long r0 = tl * rows;
        const int nrw = (int)(nr - r0 < rows ? nr - r0 : rows);
        // (V carries no restrict: in place it is Out.  The walk over (column, row) steps by the workgroup without a division)
        const int total = m * rows, dj = kEigThreads / rows, dr = kEigThreads - dj * rows;
        int j = t / rows, r = t - j * rows;
#pragma unroll 8
        for (int idx = t; idx < total; idx += kEigThreads) {
            tile[idx] = r < nrw ? V[(long long)j * ldv + r0 + r] : R(0);
            j += dj, r += dr;
            if (r >= rows) r -= rows, ++j;
        }
        R cv[kEigMaxTileRows / kEigThreads];
#pragma unroll
        for (int u = 0; u < kEigMaxTileRows / kEigThreads; ++u) {
            const int r = t + u * kEigThreads;
            cv[u] = carry >= 0 && r < nrw ? V[(long long)carry * ldv + r0 + r] : R(0);
        }
        __syncthreads();
        const int items = rows * ncg;
        for (int idx = t; idx < items; idx += kEigThreads) {
            // rows is a multiple of 64: a wave's 64 items share their column group
            const int cg = __builtin_amdgcn_readfirstlane(idx / rows);
            const int r = idx - cg * rows, c0 = cg * kCC;
            const R *sc[kCC];
#pragma unroll
            for (int cc = 0; cc < kCC; ++cc) sc[cc] = S + (long long)(c0 + cc < k ? c0 + cc : k - 1) * lds;
            R acc[kCC];
#pragma unroll
            for (int cc = 0; cc < kCC; ++cc) acc[cc] = R(0);
            for (int j = 0; j < m; ++j) {
                const R v = tile[j * rows + r];
#pragma unroll
                for (int cc = 0; cc < kCC; ++cc) acc[cc] = fma(v, sc[cc][j], acc[cc]);
            }
            if (r < nrw) {
#pragma unroll
                for (int cc = 0; cc < kCC; ++cc)
                    if (c0 + cc < k) Out[(long long)(c0 + cc) * ldo + r0 + r] = acc[cc];
            }
        }
        if (carry >= 0) {
#pragma unroll
            for (int u = 0; u < kEigMaxTileRows / kEigThreads; ++u) {
                const int r = t + u * kEigThreads;
                if (r < nrw) Out[(long long)k * ldo + r0 + r] = cv[u];
            }
        }
        __syncthreads();  // the next tile overwrites the LDS this one read
    }
}

template <typename R> __global__ void __launch_bounds__(kEigThreads) scale_kernel(long long nr, R *__restrict__ w, const R *__restrict__ nrm) {
    const R b = nrm[0];
    const bool ok = b > R(0) && isfinite(b);
    const R inv = ok ? R(1) / b : R(0);
    for (long long i = (long long)blockIdx.x * kEigThreads + threadIdx.x; i < nr; i += (long long)gridDim.x * kEigThreads)
        w[i] = ok ? w[i] * inv : R(0);
}

template <typename R, int NC>
__global__ void __launch_bounds__(64) pack_kernel(int m, const R *__restrict__ H, const R *__restrict__ beta, double *__restrict__ pack) {
    for (int j = threadIdx.x; j < m; j += 64) {
        pack[j] = (double)H[((long long)j + (long long)j * m) * NC];
        pack[m + j] = (double)beta[j];
    }
    if (threadIdx.x == 0) pack[2 * m] = (double)beta[m];  // ||v0||, kept behind the m norms of the cycle
}

template <typename R>
__global__ void __launch_bounds__(kThreads) resid_kernel(long long nr, const R *__restrict__ Q, long long ldq, const R *__restrict__ X,
                                                         long long ldx, const R *__restrict__ theta, R *__restrict__ part) {
    __shared__ R red[4][1];
    const int G = gridDim.x, g = blockIdx.x, c = blockIdx.y;
    const R th = theta[c];
    const R *q = Q + (long long)c * ldq, *x = X + (long long)c * ldx;
    long long i0, i1;
    wg_range(nr, G, g, i0, i1);
    R s[1] = {R(0)};
    for (long long i = i0 + threadIdx.x; i < i1; i += kThreads) {
        const R d = fma(-th, x[i], q[i]);
        s[0] = fma(d, d, s[0]);
    }
    block_sum<R, 1>(s, red);
    if (threadIdx.x == 0) part[(long long)c * G + g] = s[0];
}

template <typename R> __global__ void __launch_bounds__(64) resid_sum_kernel(int G, const R *__restrict__ part, double *__restrict__ res) {
    const int c = blockIdx.x;
    const R a = wave_total(part + (long long)c * G, G, 1, (int)threadIdx.x);
    if (threadIdx.x == 0) res[c] = sqrt((double)a);
}

// f(R{}, NC) for a vector type
template <typename F> void on_real(int dtype, F &&f) {
    with_types(dtype, [&](auto r, auto, auto nc) { f(r, nc); });
}

}  // namespace

hipError_t launch_eig_combine(int dtype, long long n, int m, int k, const void *V, long long ldv, const void *S, long long lds, void *Out,
                              long long ldo, int carry, hipStream_t stream) {
    if (!is_vec_type(dtype) || n < 0 || m < 1 || m > BSM_GMRES_MAX_RESTART || k < 0 || k > m || carry < -1 || carry > m)
        return hipErrorInvalidValue;
    if (n == 0 || (k == 0 && carry < 0)) return hipSuccess;
    const int rs = real_bytes(dtype), nc = elem_bytes(dtype) / rs;
    const int rows = combine_tile_reals(m, rs);
    const long long nr = n * nc, ntiles = (nr + rows - 1) / rows;
    const size_t lds_bytes = (size_t)m * rows * rs;
    const dim3 grid((unsigned)std::min<long long>(ntiles, 2048)), block(kEigThreads);
    hipError_t e = hipSuccess;
    on_real(dtype, [&](auto r, auto) {
        using R = decltype(r);
        if (lds_bytes > 65536) {
            e = hipFuncSetAttribute(reinterpret_cast<const void *>(&combine_kernel<R>), hipFuncAttributeMaxDynamicSharedMemorySize,
                                    (int)lds_bytes);
            if (e != hipSuccess) return;
        }
        hipLaunchKernelGGL(combine_kernel<R>, grid, block, lds_bytes, stream, nr, m, k, (const R *)V, ldv * nc, (const R *)S, lds, (R *)Out,
                           ldo * nc, carry, rows);
    });
    return e != hipSuccess ? e : hipGetLastError();
}

hipError_t launch_eig_scale(int dtype, long long n, void *w, const void *nrm, hipStream_t stream) {
    if (!is_vec_type(dtype) || n < 0) return hipErrorInvalidValue;
    if (n == 0) return hipSuccess;
    const int nc = elem_bytes(dtype) / real_bytes(dtype);
    const long long nr = n * nc;
    const dim3 grid((unsigned)std::min<long long>((nr + kEigThreads * 4 - 1) / (kEigThreads * 4), 1024)), block(kEigThreads);
    on_real(dtype, [&](auto r, auto) {
        using R = decltype(r);
        hipLaunchKernelGGL(scale_kernel<R>, grid, block, 0, stream, nr, (R *)w, (const R *)nrm);
    });
    return hipGetLastError();
}

hipError_t launch_eig_pack(int dtype, int m, const void *H, const void *beta, double *pack, hipStream_t stream) {
    if (!is_vec_type(dtype) || m < 1) return hipErrorInvalidValue;
    on_real(dtype, [&](auto r, auto nc) {
        using R = decltype(r);
        hipLaunchKernelGGL((pack_kernel<R, decltype(nc)::value>), dim3(1), dim3(64), 0, stream, m, (const R *)H, (const R *)beta, pack);
    });
    return hipGetLastError();
}

hipError_t launch_eig_resid(int dtype, long long n, int k, const void *Q, long long ldq, const void *X, long long ldx, const void *theta,
                            void *part, double *res, hipStream_t stream) {
    if (!is_vec_type(dtype) || n < 0 || k < 1 || k > kCgMaxRhs) return hipErrorInvalidValue;
    const int es = elem_bytes(dtype), nc = es / real_bytes(dtype), G = krylov_grid(n, es);
    on_real(dtype, [&](auto r, auto) {
        using R = decltype(r);
        hipLaunchKernelGGL(resid_kernel<R>, dim3((unsigned)G, (unsigned)k), dim3(kThreads), 0, stream, n * nc, (const R *)Q, ldq * nc,
                           (const R *)X, ldx * nc, (const R *)theta, (R *)part);
        hipLaunchKernelGGL(resid_sum_kernel<R>, dim3((unsigned)k), dim3(64), 0, stream, G, (const R *)part, res);
    });
    return hipGetLastError();
}

}  // namespace bsm
