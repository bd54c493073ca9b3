// bsm_cg_device.h -- the device-side pieces the lockstep solver units (bsm_cg.hip, bsm_bicgstab.hip, bsm_gmres_multi.hip) share: the 16-byte
// access, the wave / workgroup sums, the fixed-order sum of a column's partials, a workgroup's row range and the dispatch
// of a launch on the vector type.  For the kernel units only; the layout these walk is described in bsm_cg.h.
#pragma once
#include <hip/hip_runtime.h>

#include "bsm_cg.h"

namespace bsm {

constexpr int kThreads = 256;
constexpr int kU = 2;  // 16-byte groups per thread, array and tile

template <typename R> struct alignas(16) Vec16 {
    R r[16 / sizeof(R)];
};
template <typename R> __device__ __forceinline__ Vec16<R> load16(const R *p) { return *reinterpret_cast<const Vec16<R> *>(p); }
template <typename R> __device__ __forceinline__ void store16(R *p, const Vec16<R> &v) { *reinterpret_cast<Vec16<R> *>(p) = v; }

template <typename R> __device__ __forceinline__ R wave_sum(R v) {
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) v += __shfl_xor(v, d, 64);
    return v;
}
// sum of p[0], p[stride], .. (G terms) by one wave in a fixed order: every wave of every workgroup gets the same bits
template <typename R> __device__ __forceinline__ R wave_total(const R *__restrict__ p, int G, int stride, int lane) {
    R a = R(0);
    for (int g = lane; g < G; g += 64) a += p[(long long)g * stride];
    return wave_sum(a);
}
// v[q] = the workgroup's sum of v[q], in every thread
template <typename R, int NV> __device__ __forceinline__ void block_sum(R (&v)[NV], R (*red)[NV]) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
    for (int q = 0; q < NV; ++q) v[q] = wave_sum(v[q]);
    if (lane == 0) {
#pragma unroll
        for (int q = 0; q < NV; ++q) red[wave][q] = v[q];
    }
    __syncthreads();
#pragma unroll
    for (int q = 0; q < NV; ++q) v[q] = (red[0][q] + red[1][q]) + (red[2][q] + red[3][q]);
}
__device__ __forceinline__ void wg_range(long long ng, int G, int wg, long long &g0, long long &g1) {
    const long long per = (ng + G - 1) / G;
    g0 = per * wg;
    g0 = g0 < ng ? g0 : ng;
    g1 = g0 + per < ng ? g0 + per : ng;
}
// whether an element (NC reals) is zero
template <typename R, int NC> __device__ __forceinline__ bool is_zero(const R *a) { return a[0] == R(0) && a[NC - 1] == R(0); }

// f(R{}, NC, 16-byte groups per column, the (row ranges, columns) grid, sgn) for the vector type of d, sgn = +1 / -1 as R
// for the conjugated / unconjugated form
template <typename F> hipError_t cg_dispatch(const CgDims &d, F &&f) {
    if (!is_vec_type(d.dtype) || d.n < 0 || d.nrhs < 1 || d.nrhs > kCgMaxRhs || d.G < 1 || d.G > kKrylovMaxGrid)
        return hipErrorInvalidValue;
    with_types(d.dtype, [&](auto r, auto, auto nc) {
        using R = decltype(r);
        constexpr int NC = decltype(nc)::value;
        const long long ng = d.ld / (16 / (long long)(sizeof(R) * NC));
        f(r, nc, ng, dim3((unsigned)d.G, (unsigned)d.nrhs), (R)(d.conj ? 1 : -1));
    });
    return hipGetLastError();
}

}  // namespace bsm
