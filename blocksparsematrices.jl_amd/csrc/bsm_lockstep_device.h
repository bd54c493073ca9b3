// bsm_lockstep_device.h -- the one home of the device-side pieces the solver kernel units share (bsm_cg.hip, bsm_bicgstab.hip,
// bsm_gmres_multi.hip, bsm_minres.hip; bsm_krylov.hip takes the access and the sums): the 16-byte access with the guarded read of a caller's
// column, the arithmetic on one 16-byte group, the wave / workgroup sums, the fixed-order sum of a column's partials, the
// decision of a column with its first tolerance, the carry-over of a frozen column, a workgroup's row range and the dispatch
// of a launch on the vector type.  Every helper adds to each accumulator exactly the fma sequence written in it -- the
// results of the units are bit-identical from run to run because of that order, so it is part of the interface.
// For the kernel units only; the layout these walk is described in bsm_cg.h.
#pragma once
#include <hip/hip_runtime.h>

#include "bsm_cg.h"
#include "bsm_krylov_device.h"

namespace bsm {

constexpr int kThreads = 256;
constexpr int kU = 2;  // 16-byte groups per thread, array and tile

// ---- the 16-byte access
template <typename R> struct alignas(16) Vec16 {
    R r[16 / sizeof(R)];
};
template <typename R> __device__ __forceinline__ Vec16<R> load16(const R *p) { return *reinterpret_cast<const Vec16<R> *>(p); }
template <typename R> __device__ __forceinline__ void store16(R *p, const Vec16<R> &v) { *reinterpret_cast<Vec16<R> *>(p) = v; }
template <typename R> __device__ __forceinline__ Vec16<R> zero16() {
    Vec16<R> v;
#pragma unroll
    for (int k = 0; k < 16 / (int)sizeof(R); ++k) v.r[k] = R(0);
    return v;
}
// group g of a caller's column (any leading dimension, any element alignment), element by element; rows >= n read as zero
template <typename R, int NC> __device__ __forceinline__ Vec16<R> load16_guarded(const R *col, long long g, long long n) {
    constexpr int VE = 16 / (int)sizeof(R) / NC;
    Vec16<R> v;
#pragma unroll
    for (int e = 0; e < VE; ++e) {
        const long long row = g * VE + e;
#pragma unroll
        for (int k = 0; k < NC; ++k) v.r[e * NC + k] = row < n ? col[row * NC + k] : R(0);
    }
    return v;
}

// ---- arithmetic on one 16-byte group
template <typename R> __device__ __forceinline__ void add16(Vec16<R> &v, const Vec16<R> &w) {
#pragma unroll
    for (int k = 0; k < 16 / (int)sizeof(R); ++k) v.r[k] += w.r[k];
}
template <typename R> __device__ __forceinline__ void sub16(Vec16<R> &v, const Vec16<R> &w) {
#pragma unroll
    for (int k = 0; k < 16 / (int)sizeof(R); ++k) v.r[k] -= w.r[k];
}
template <typename R> __device__ __forceinline__ void scale16(Vec16<R> &v, R sc) {
#pragma unroll
    for (int k = 0; k < 16 / (int)sizeof(R); ++k) v.r[k] *= sc;
}
// y += a x on the elements of the group
template <typename R, int NC> __device__ __forceinline__ void axpy16(R ar, R ai, const Vec16<R> &x, Vec16<R> &y) {
#pragma unroll
    for (int e = 0; e < 16 / (int)sizeof(R) / NC; ++e) gs_madd<R, NC>(ar, ai, x.r[e * NC], x.r[e * NC + NC - 1], y.r[e * NC], y.r[e * NC + NC - 1]);
}
// s += ||v||^2
template <typename R> __device__ __forceinline__ void norm16(const Vec16<R> &v, R &s) {
#pragma unroll
    for (int k = 0; k < 16 / (int)sizeof(R); ++k) s = fma(v.r[k], v.r[k], s);
}
// s[0 .. NC) += conj(u) v
template <typename R, int NC> __device__ __forceinline__ void dot16(const Vec16<R> &u, const Vec16<R> &v, R *s) {
    gs_dot<R, NC, 16 / (int)sizeof(R) / NC>(u.r, v.r, s);
}
// the same with the sign of the method's form on the ui terms: sgn = +1 conj(u) v (CG), -1 u v (COCG)
template <typename R, int NC> __device__ __forceinline__ void dot16(const Vec16<R> &u, const Vec16<R> &v, R sgn, R *s) {
#pragma unroll
    for (int e = 0; e < 16 / (int)sizeof(R) / NC; ++e) {
        if (NC == 1) {
            s[0] = fma(u.r[e], v.r[e], s[0]);
        } else {
            const R ur = u.r[e * NC], ui = u.r[e * NC + NC - 1], vr = v.r[e * NC], vi = v.r[e * NC + NC - 1];
            s[0] = fma(ur, vr, s[0]);
            s[0] = fma(sgn * ui, vi, s[0]);
            s[NC - 1] = fma(ur, vi, s[NC - 1]);
            s[NC - 1] = fma(-sgn * ui, vr, s[NC - 1]);
        }
    }
}
// the form of a complex v with itself, s[0] += a a + sgn b b, s[1] += a b - sgn b a per element (a, b): dot16 on (v, v)
template <typename R> __device__ __forceinline__ void form16(const Vec16<R> &v, R sgn, R *s) { dot16<R, 2>(v, v, sgn, s); }

// ---- sums
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
// s[0 .. NC) = the total of column c's partials p[(c * G + g) * NC ..]
template <typename R, int NC> __device__ __forceinline__ void column_total(const R *__restrict__ p, int c, int G, int lane, R *s) {
#pragma unroll
    for (int k = 0; k < NC; ++k) s[k] = wave_total(p + (long long)c * G * NC + k, G, NC, lane);
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

// ---- a column's scalars
// the status a residual norm gives a column: 2 not finite, 0 within tol, else it runs on
template <typename R> __device__ __forceinline__ int decide(R norm, double tol) { return !isfinite(norm) ? 2 : ((double)norm <= tol ? 0 : kCgRun); }
// the first launch of a solve: bn = ||b_c|| from the column's G shares of ||b||^2 -> tol_c
template <typename R> __device__ __forceinline__ double first_tol(const R *__restrict__ pbb, int G, int lane, double rtol, double atol, R &bn) {
    bn = sqrt(wave_total(pbb, G, 1, lane));
    return fmax(rtol * (double)bn, atol);
}
// a column that does not iterate any more moves to the other slot with `status` (what it froze with before, or 3: it
// broke down in this iteration); the record repeats the status
__device__ __forceinline__ void carry_frozen(const CgSlot &in, CgSlot &out, CgRecord &rec, int c, int status) {
    out.rz[c][0] = in.rz[c][0];
    out.rz[c][1] = in.rz[c][1];
    out.rn[c] = in.rn[c];
    out.status[c] = status;
    out.done[c] = in.done[c];
    rec.status[c] = status;
}

// the row range of workgroup wg: groups [g0, g1) of ng
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
