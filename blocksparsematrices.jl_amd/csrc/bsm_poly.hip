// bsm_poly.hip -- the kernels of a composed handle's product (bsm_poly_create; include/bsm_rocm.h): the vector work between
// the products with A and D of the s-step polynomial recurrence z = p(A) x on K columns at once.  Kept out of the product
// kernel units like bsm_cg.hip: the build id (Makefile BUILD_ID) names the kernels and schedule of the PRODUCTS.
// (No counterpart in the reference: its operators are LinearMaps handed to a Julia solver package.)
//
// The conventions are those of bsm_cg.hip: 256-thread workgroups on the (krylov_grid(n), K) grid, a workgroup's row range
// walked in tiles of 256 threads x kU unguarded 16-byte groups of workspace columns whose padding is zero and stays zero
// (the helpers: bsm_lockstep_device.h).  There is no reduction, no device state and no decision: the scalars of a step are
// kernel arguments, real ones, so every kernel but the two that touch the caller's matrices walks a column as reals.
//   load_kernel    R = X (element by element under a guard, padding zeroed);  without D also d = b0 R
//   step_kernel    (no D) ONE pass:  acc += d (first step: acc = d);  R -= Q;  d = a d + b R
//   resid_kernel   (with D, in front of T = D R)  acc += d (first step: acc = d);  R -= Q
//   dir_kernel     (with D, behind T = D R)  d = a d + b T (first: d = b T, d is not read)
//   store_kernel   Y = alpha (acc + d) + beta Y on n rows of K columns of the caller's Y under a guard, nothing else
// Every product and sum below is rounded on its own (mul_rn / add_rn: no fused multiply-add), the arithmetic of the numpy
// twin in tests/_poly.py, so a product is bit-identical from run to run wherever the products with A and D are.
// Device values are written with ordinary vector stores only.
#include "bsm_poly.h"

#include "../../include/bsm_rocm.h"
#include "bsm_lockstep_device.h"

namespace bsm {
namespace {

__device__ __forceinline__ float mul_rn(float a, float b) { return __fmul_rn(a, b); }
__device__ __forceinline__ double mul_rn(double a, double b) { return __dmul_rn(a, b); }
__device__ __forceinline__ float add_rn(float a, float b) { return __fadd_rn(a, b); }
__device__ __forceinline__ double add_rn(double a, double b) { return __dadd_rn(a, b); }

// v = a v + b w on the reals of one group, every product rounded before the sum
template <typename R> __device__ __forceinline__ void axpby16(Vec16<R> &v, R a, R b, const Vec16<R> &w) {
#pragma unroll
    for (int k = 0; k < 16 / (int)sizeof(R); ++k) v.r[k] = add_rn(mul_rn(a, v.r[k]), mul_rn(b, w.r[k]));
}
// a x for one element (real: ai, xi unused)
template <typename R, int NC> __device__ __forceinline__ void scale_elem(R ar, R ai, R xr, R xi, R &yr, R &yi) {
    if (NC == 1) {
        yr = mul_rn(ar, xr);
    } else {
        yr = add_rn(mul_rn(ar, xr), -mul_rn(ai, xi));
        yi = add_rn(mul_rn(ar, xi), mul_rn(ai, xr));
    }
}

template <typename R, int NC>
__global__ void __launch_bounds__(kThreads) load_kernel(long long n, long long ng, long long ldx, R b0, const R *__restrict__ X,
                                                        R *__restrict__ Rv, R *__restrict__ d) {
    constexpr int GC = 16 / (int)sizeof(R);
    const int t = threadIdx.x, G = gridDim.x, wg = blockIdx.x, c = blockIdx.y;
    const R *Xc = X + (long long)c * ldx * NC;
    const long long off = (long long)c * ng * GC;
    long long g0, g1;
    wg_range(ng, G, wg, g0, g1);
    for (long long tile = g0; tile < g1; tile += (long long)kThreads * kU) {
#pragma unroll
        for (int i = 0; i < kU; ++i) {
            const long long g = tile + (long long)i * kThreads + t;
            if (g >= g1) continue;
            Vec16<R> v = load16_guarded<R, NC>(Xc, g, n);
            store16(Rv + off + g * GC, v);
            if (d) {
#pragma unroll
                for (int k = 0; k < GC; ++k) v.r[k] = mul_rn(b0, v.r[k]);
                store16(d + off + g * GC, v);
            }
        }
    }
}

template <typename R, bool FIRST>
__global__ void __launch_bounds__(kThreads) step_kernel(long long ng, R a, R b, R *__restrict__ acc, R *__restrict__ Rv,
                                                        const R *__restrict__ Q, R *__restrict__ d) {
    constexpr int GC = 16 / (int)sizeof(R);
    const int t = threadIdx.x, G = gridDim.x, wg = blockIdx.x, c = blockIdx.y;
    const long long off = (long long)c * ng * GC;
    long long g0, g1;
    wg_range(ng, G, wg, g0, g1);
    for (long long tile = g0; tile < g1; tile += (long long)kThreads * kU) {
        Vec16<R> dv[kU], rv[kU], qv[kU], av[kU];
#pragma unroll
        for (int i = 0; i < kU; ++i) {
            const long long g = tile + (long long)i * kThreads + t;
            if (g < g1) {
                dv[i] = load16(d + off + g * GC);
                rv[i] = load16(Rv + off + g * GC);
                qv[i] = load16(Q + off + g * GC);
                if (!FIRST) av[i] = load16(acc + off + g * GC);
            }
        }
#pragma unroll
        for (int i = 0; i < kU; ++i) {
            const long long g = tile + (long long)i * kThreads + t;
            if (g >= g1) continue;
            if (FIRST)
                av[i] = dv[i];
            else
                add16(av[i], dv[i]);
            sub16(rv[i], qv[i]);
            axpby16(dv[i], a, b, rv[i]);
            store16(acc + off + g * GC, av[i]);
            store16(Rv + off + g * GC, rv[i]);
            store16(d + off + g * GC, dv[i]);
        }
    }
}

template <typename R, bool FIRST>
__global__ void __launch_bounds__(kThreads) resid_kernel(long long ng, R *__restrict__ acc, const R *__restrict__ d, R *__restrict__ Rv,
                                                         const R *__restrict__ Q) {
    constexpr int GC = 16 / (int)sizeof(R);
    const int t = threadIdx.x, G = gridDim.x, wg = blockIdx.x, c = blockIdx.y;
    const long long off = (long long)c * ng * GC;
    long long g0, g1;
    wg_range(ng, G, wg, g0, g1);
    for (long long tile = g0; tile < g1; tile += (long long)kThreads * kU) {
        Vec16<R> dv[kU], rv[kU], qv[kU], av[kU];
#pragma unroll
        for (int i = 0; i < kU; ++i) {
            const long long g = tile + (long long)i * kThreads + t;
            if (g < g1) {
                dv[i] = load16(d + off + g * GC);
                rv[i] = load16(Rv + off + g * GC);
                qv[i] = load16(Q + off + g * GC);
                if (!FIRST) av[i] = load16(acc + off + g * GC);
            }
        }
#pragma unroll
        for (int i = 0; i < kU; ++i) {
            const long long g = tile + (long long)i * kThreads + t;
            if (g >= g1) continue;
            if (FIRST)
                av[i] = dv[i];
            else
                add16(av[i], dv[i]);
            sub16(rv[i], qv[i]);
            store16(acc + off + g * GC, av[i]);
            store16(Rv + off + g * GC, rv[i]);
        }
    }
}

template <typename R, bool FIRST>
__global__ void __launch_bounds__(kThreads) dir_kernel(long long ng, R a, R b, const R *__restrict__ T, R *__restrict__ d) {
    constexpr int GC = 16 / (int)sizeof(R);
    const int t = threadIdx.x, G = gridDim.x, wg = blockIdx.x, c = blockIdx.y;
    const long long off = (long long)c * ng * GC;
    long long g0, g1;
    wg_range(ng, G, wg, g0, g1);
    for (long long tile = g0; tile < g1; tile += (long long)kThreads * kU) {
        Vec16<R> dv[kU], tv[kU];
#pragma unroll
        for (int i = 0; i < kU; ++i) {
            const long long g = tile + (long long)i * kThreads + t;
            if (g < g1) {
                tv[i] = load16(T + off + g * GC);
                if (!FIRST) dv[i] = load16(d + off + g * GC);
            }
        }
#pragma unroll
        for (int i = 0; i < kU; ++i) {
            const long long g = tile + (long long)i * kThreads + t;
            if (g >= g1) continue;
            if (FIRST) {
#pragma unroll
                for (int k = 0; k < GC; ++k) dv[i].r[k] = mul_rn(b, tv[i].r[k]);
            } else {
                axpby16(dv[i], a, b, tv[i]);
            }
            store16(d + off + g * GC, dv[i]);
        }
    }
}

template <typename R, int NC, bool STRONG>
__global__ void __launch_bounds__(kThreads) store_kernel(long long n, long long ng, long long ldy, R ar, R ai, R br, R bi,
                                                         const R *__restrict__ acc, const R *__restrict__ d, R *__restrict__ Y) {
    constexpr int GC = 16 / (int)sizeof(R), VE = GC / NC;
    const int t = threadIdx.x, G = gridDim.x, wg = blockIdx.x, c = blockIdx.y;
    R *Yc = Y + (long long)c * ldy * NC;
    const long long off = (long long)c * ng * GC;
    long long g0, g1;
    wg_range(ng, G, wg, g0, g1);
    for (long long g = g0 + t; g < g1; g += kThreads) {
        Vec16<R> s = load16(d + off + g * GC);
        if (acc) {
            Vec16<R> av = load16(acc + off + g * GC);
            add16(av, s);
            s = av;
        }
#pragma unroll
        for (int e = 0; e < VE; ++e) {
            const long long row = g * VE + e;
            if (row >= n) continue;
            R yr = R(0), yi = R(0);
            scale_elem<R, NC>(ar, ai, s.r[e * NC], s.r[e * NC + NC - 1], yr, yi);
            if (!STRONG) {
                R zr = R(0), zi = R(0);
                scale_elem<R, NC>(br, bi, Yc[row * NC], Yc[row * NC + NC - 1], zr, zi);
                yr = add_rn(yr, zr);
                yi = add_rn(yi, zi);
            }
            Yc[row * NC] = yr;
            if (NC == 2) Yc[row * NC + NC - 1] = yi;
        }
    }
}

}  // namespace

hipError_t launch_poly_load(const CgDims &dm, const void *X, long long ldx, void *R_, void *d, double b0, hipStream_t stream) {
    return cg_dispatch(dm, [&](auto rt, auto nc, long long ng, dim3 grid, auto) {
        using R = decltype(rt);
        constexpr int NC = decltype(nc)::value;
        hipLaunchKernelGGL((load_kernel<R, NC>), grid, dim3(kThreads), 0, stream, dm.n, ng, ldx, (R)b0, (const R *)X, (R *)R_, (R *)d);
    });
}

hipError_t launch_poly_step(const CgDims &dm, bool first, double a, double b, void *acc, void *R_, const void *Q, void *d, hipStream_t stream) {
    return cg_dispatch(dm, [&](auto rt, auto, long long ng, dim3 grid, auto) {
        using R = decltype(rt);
        auto launch = [&](auto kernel) {
            hipLaunchKernelGGL(kernel, grid, dim3(kThreads), 0, stream, ng, (R)a, (R)b, (R *)acc, (R *)R_, (const R *)Q, (R *)d);
        };
        if (first)
            launch(step_kernel<R, true>);
        else
            launch(step_kernel<R, false>);
    });
}

hipError_t launch_poly_resid(const CgDims &dm, bool first, void *acc, const void *d, void *R_, const void *Q, hipStream_t stream) {
    return cg_dispatch(dm, [&](auto rt, auto, long long ng, dim3 grid, auto) {
        using R = decltype(rt);
        auto launch = [&](auto kernel) {
            hipLaunchKernelGGL(kernel, grid, dim3(kThreads), 0, stream, ng, (R *)acc, (const R *)d, (R *)R_, (const R *)Q);
        };
        if (first)
            launch(resid_kernel<R, true>);
        else
            launch(resid_kernel<R, false>);
    });
}

hipError_t launch_poly_dir(const CgDims &dm, bool first, double a, double b, const void *T, void *d, hipStream_t stream) {
    return cg_dispatch(dm, [&](auto rt, auto, long long ng, dim3 grid, auto) {
        using R = decltype(rt);
        auto launch = [&](auto kernel) { hipLaunchKernelGGL(kernel, grid, dim3(kThreads), 0, stream, ng, (R)a, (R)b, (const R *)T, (R *)d); };
        if (first)
            launch(dir_kernel<R, true>);
        else
            launch(dir_kernel<R, false>);
    });
}

hipError_t launch_poly_store(const CgDims &dm, const double *alpha, const double *beta, bool strong_zero, const void *acc, const void *d,
                             void *Y, long long ldy, hipStream_t stream) {
    return cg_dispatch(dm, [&](auto rt, auto nc, long long ng, dim3 grid, auto) {
        using R = decltype(rt);
        constexpr int NC = decltype(nc)::value;
        auto launch = [&](auto kernel) {
            hipLaunchKernelGGL(kernel, grid, dim3(kThreads), 0, stream, dm.n, ng, ldy, (R)alpha[0], (R)alpha[1], (R)beta[0], (R)beta[1],
                               (const R *)acc, (const R *)d, (R *)Y);
        };
        if (strong_zero)
            launch(store_kernel<R, NC, true>);
        else
            launch(store_kernel<R, NC, false>);
    });
}

}  // namespace bsm
