// bsm_svds.hip -- the kernels of bsm_svds_* (include/bsm_rocm.h) that are its own: the gather of a cycle's norms for the one
// copy the cycle ends with, and the two-grid true-residual pass.  A step of the bidiagonalisation itself runs on the product
// kernels, on the Gram-Schmidt pass of bsm_krylov.hip and on the guarded scale and the basis compression of bsm_eig.hip,
// through their launch interfaces.  Kept out of the product kernel units like bsm_eig.hip: the build id names the kernels of
// the PRODUCTS.
// (No counterpart in the reference: its operators are LinearMaps handed to KrylovKit's svdsolve.)
//
// Everything here walks REAL components: the projected matrix is real, so sigma is real and a complex column of n entries is a
// real one of 2 n.  Two instantiations per kernel.
//
//   pack_kernel       one wave: alpha, beta and ||v0|| as doubles, side by side.
//   resid_kernel      grid (Gm + Gn, columns).  Workgroups g < Gm walk a row range of the m-row grid: d = RM - sigma U; the
//                     others one of the n-row grid: d = RN - sigma V.  One partial of sum d^2 per workgroup and column; every
//                     access is one real per lane, so any element alignment and leading dimension is served by the same code.
//   resid_sum_kernel  one wave per column adds the partials of either grid in a fixed order and takes the roots.
// No floating-point atomic, and no workgroup waits for another.
#include "bsm_svds.h"

#include "../../include/bsm_rocm.h"
#include "bsm_lockstep_device.h"

namespace bsm {
namespace {

template <typename R>
__global__ void __launch_bounds__(64) pack_kernel(int m, const R *__restrict__ alpha, const R *__restrict__ beta, double *__restrict__ pack) {
    for (int j = threadIdx.x; j < m; j += 64) {
        pack[j] = (double)alpha[j];
        pack[m + j] = (double)beta[j];
    }
    if (threadIdx.x == 0) pack[2 * m] = (double)beta[m];  // ||v0||, kept behind the m norms of the cycle
}

template <typename R>
__global__ void __launch_bounds__(kThreads)
    resid_kernel(long long mr, long long nr, int Gm, const R *__restrict__ RM, long long ldrm, const R *__restrict__ U, long long ldu,
                 const R *__restrict__ RN, long long ldrn, const R *__restrict__ V, long long ldv, const R *__restrict__ sigma,
                 R *__restrict__ part) {
    __shared__ R red[4][1];
    const int Gall = gridDim.x, c = blockIdx.y;
    const bool left = (int)blockIdx.x < Gm;  // uniform in the workgroup
    const int G = left ? Gm : Gall - Gm, g = left ? (int)blockIdx.x : (int)blockIdx.x - Gm;
    const long long rows = left ? mr : nr;
    const R sg = sigma[c];
    const R *q = left ? RM + (long long)c * ldrm : RN + (long long)c * ldrn;
    const R *x = left ? U + (long long)c * ldu : V + (long long)c * ldv;
    long long i0, i1;
    wg_range(rows, G, g, i0, i1);
    R s[1] = {R(0)};
    for (long long i = i0 + threadIdx.x; i < i1; i += kThreads) {
        const R d = fma(-sg, x[i], q[i]);
        s[0] = fma(d, d, s[0]);
    }
    block_sum<R, 1>(s, red);
    if (threadIdx.x == 0) part[(long long)c * Gall + blockIdx.x] = s[0];
}

template <typename R>
__global__ void __launch_bounds__(64)
    resid_sum_kernel(int Gm, int Gn, const R *__restrict__ part, double *__restrict__ res_av, double *__restrict__ res_ahu) {
    const int c = blockIdx.x;
    const R *p = part + (long long)c * (Gm + Gn);
    const R a = wave_total(p, Gm, 1, (int)threadIdx.x);
    const R b = wave_total(p + Gm, Gn, 1, (int)threadIdx.x);
    if (threadIdx.x == 0) {
        res_av[c] = sqrt((double)a);
        res_ahu[c] = sqrt((double)b);
    }
}

// f(R{}) for a vector type
template <typename F> void on_real(int dtype, F &&f) {
    with_types(dtype, [&](auto r, auto, auto) { f(r); });
}

}  // namespace

hipError_t launch_svds_pack(int dtype, int m, const void *alpha, const void *beta, double *pack, hipStream_t stream) {
    if (!is_vec_type(dtype) || m < 1) return hipErrorInvalidValue;
    on_real(dtype, [&](auto r) {
        using R = decltype(r);
        hipLaunchKernelGGL(pack_kernel<R>, dim3(1), dim3(64), 0, stream, m, (const R *)alpha, (const R *)beta, pack);
    });
    return hipGetLastError();
}

hipError_t launch_svds_resid(int dtype, long long mrows, long long nrows, int k, const void *RM, long long ldrm, const void *U,
                             long long ldu, const void *RN, long long ldrn, const void *V, long long ldv, const void *sigma, void *part,
                             double *res_av, double *res_ahu, hipStream_t stream) {
    if (!is_vec_type(dtype) || mrows < 0 || nrows < 0 || k < 1 || k > kCgMaxRhs) return hipErrorInvalidValue;
    const int es = elem_bytes(dtype), nc = es / real_bytes(dtype), Gm = krylov_grid(mrows, es), Gn = krylov_grid(nrows, es);
    on_real(dtype, [&](auto r) {
        using R = decltype(r);
        hipLaunchKernelGGL(resid_kernel<R>, dim3((unsigned)(Gm + Gn), (unsigned)k), dim3(kThreads), 0, stream, mrows * nc, nrows * nc, Gm,
                           (const R *)RM, ldrm * nc, (const R *)U, ldu * nc, (const R *)RN, ldrn * nc, (const R *)V, ldv * nc,
                           (const R *)sigma, (R *)part);
        hipLaunchKernelGGL(resid_sum_kernel<R>, dim3((unsigned)k), dim3(64), 0, stream, Gm, Gn, (const R *)part, res_av, res_ahu);
    });
    return hipGetLastError();
}

}  // namespace bsm
