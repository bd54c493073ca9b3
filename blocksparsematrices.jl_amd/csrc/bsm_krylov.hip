// bsm_krylov.hip -- the kernels of bsm_krylov_orth (include/bsm_rocm.h): one classical Gram-Schmidt pass on vectors of any
// element alignment, for a caller's Krylov method.  (The GMRES solvers run the same pass on their padded workspace:
// bsm_gmres_multi.hip.)  Kept out of the product kernel units like bsm_extract.hip and bsm_invert.hip: the build id (Makefile
// BUILD_ID) names the kernels and schedule of the PRODUCTS.
// (No counterpart in the reference: its operators are LinearMaps handed to a Julia solver package.)
//
// One classical Gram-Schmidt pass  h = V^H w,  w -= V h,  ||w||  is two launches with a kernel boundary between them --
// no workgroup ever waits for another inside a launch, and there is no floating-point atomic anywhere:
//   dot_kernel    workgroup g owns a contiguous range of the rows (the same split in both kernels, krylov_grid of them).
//                 It walks the range in tiles of 256 threads x U 16-byte groups; a tile of w is loaded ONCE and stays in
//                 registers while the k columns of V stream past it, CB columns -- CB * U loads per thread -- in flight.
//                 Per column: the lane's products, 6 xor-shuffles for the wave, lane 0 adds the wave's sum to its LDS slot
//                 (acc[c][wave]); behind the last tile thread c folds the four slots and writes ONE partial per
//                 workgroup and column, part[c * G + g].
//   sweep_kernel  every workgroup first sums the G partials of every column in the same fixed order (S threads per
//                 column, strided, then xor-shuffles: all workgroups get the same h, bit for bit), keeps h in LDS, and
//                 walks its rows again: a tile of w in registers, the columns streamed past it, w -= V h, stored once,
//                 |w|^2 summed on the way -> nrmpart[g].  Workgroup 0 also adds h to hsum.
// Loads and stores are 16 bytes per lane where the pointers allow it -- w and every column of V congruent modulo
// 16, i.e. (ldv * sizeof(T)) % 16 == 0 --: the vector groups start at the first 16-byte boundary of w, the elements in
// front of it and behind the last whole group go element by element through the same code (a group that is not wholly
// inside [0, n) is read and written under a per-element guard).  Otherwise every group is one element (VE = 1).
// Every sum has a fixed order: the results are bit-identical from run to run.  norm_kernel (one wave) adds the
// per-workgroup norm shares in a fixed order too.  The 16-byte access, the wave / workgroup sums and the row ranges are
// those of the lockstep units (bsm_lockstep_device.h), the arithmetic of a group is bsm_krylov_device.h.
#include "bsm_krylov.h"

#include "../../include/bsm_rocm.h"
#include "bsm_lockstep_device.h"

namespace bsm {
namespace {

constexpr int kCB = 4;  // columns in flight

// one group of VE elements (GC = VE * NC components) starting at element e0 of p; A16: groups are 16-byte aligned
template <typename R, int NC, int VE, bool A16>
__device__ __forceinline__ void load_group(const R *__restrict__ p, long long e0, long long n, bool valid, R (&v)[VE * NC]) {
    constexpr int GC = VE * NC;
    if (A16) {
        if (valid && e0 >= 0 && e0 + VE <= n) {
            const Vec16<R> t = load16(p + e0 * NC);
#pragma unroll
            for (int q = 0; q < GC; ++q) v[q] = t.r[q];
            return;
        }
    }
#pragma unroll
    for (int e = 0; e < VE; ++e) {
        const bool in = valid && e0 + e >= 0 && e0 + e < n;
#pragma unroll
        for (int c = 0; c < NC; ++c) v[e * NC + c] = in ? p[(e0 + e) * NC + c] : R(0);
    }
}
template <typename R, int NC, int VE, bool A16>
__device__ __forceinline__ void store_group(R *__restrict__ p, long long e0, long long n, bool valid, const R (&v)[VE * NC]) {
    constexpr int GC = VE * NC;
    if (A16) {
        if (valid && e0 >= 0 && e0 + VE <= n) {
            Vec16<R> t;
#pragma unroll
            for (int q = 0; q < GC; ++q) t.r[q] = v[q];
            store16(p + e0 * NC, t);
            return;
        }
    }
#pragma unroll
    for (int e = 0; e < VE; ++e) {
        if (valid && e0 + e >= 0 && e0 + e < n) {
#pragma unroll
            for (int c = 0; c < NC; ++c) p[(e0 + e) * NC + c] = v[e * NC + c];
        }
    }
}

// (wg_range of the shared header on the ng groups that cover elements lo .. n - 1; lo <= 0: the first group may start in
// front of the vector)
template <typename R, int NC, int VE, bool A16>
__global__ void __launch_bounds__(kThreads) dot_kernel(long long n, int k, const R *__restrict__ V, long long ldv,
                                                       const R *__restrict__ w, R *__restrict__ part, long long lo, long long ng) {
    constexpr int GC = VE * NC;
    __shared__ R acc[BSM_GMRES_MAX_RESTART * 4 * NC];
    const int t = threadIdx.x, lane = t & 63, wave = t >> 6, G = gridDim.x, wg = blockIdx.x;
    for (int i = t; i < k * 4 * NC; i += kThreads) acc[i] = R(0);
    __syncthreads();
    long long g0, g1;
    wg_range(ng, G, wg, g0, g1);
    for (long long tile = g0; tile < g1; tile += (long long)kThreads * kU) {
        R wv[kU][GC];
        long long e0[kU];
        bool ok[kU];
#pragma unroll
        for (int u = 0; u < kU; ++u) {
            const long long g = tile + (long long)u * kThreads + t;
            ok[u] = g < g1;
            e0[u] = lo + g * VE;
            load_group<R, NC, VE, A16>(w, e0[u], n, ok[u], wv[u]);
        }
        for (int c0 = 0; c0 < k; c0 += kCB) {
            R vv[kCB][kU][GC];
#pragma unroll
            for (int cc = 0; cc < kCB; ++cc)
#pragma unroll
                for (int u = 0; u < kU; ++u)
                    load_group<R, NC, VE, A16>(V + (long long)(c0 + cc) * ldv * NC, e0[u], n, ok[u] && c0 + cc < k, vv[cc][u]);
            R s[kCB][NC];
#pragma unroll
            for (int cc = 0; cc < kCB; ++cc) {
#pragma unroll
                for (int c = 0; c < NC; ++c) s[cc][c] = R(0);
#pragma unroll
                for (int u = 0; u < kU; ++u) gs_dot<R, NC, VE>(vv[cc][u], wv[u], s[cc]);
            }
#pragma unroll
            for (int cc = 0; cc < kCB; ++cc)
#pragma unroll
                for (int c = 0; c < NC; ++c) s[cc][c] = wave_sum(s[cc][c]);
            if (lane == 0) {
#pragma unroll
                for (int cc = 0; cc < kCB; ++cc)
                    if (c0 + cc < k) {
#pragma unroll
                        for (int c = 0; c < NC; ++c) acc[((c0 + cc) * 4 + wave) * NC + c] += s[cc][c];
                    }
            }
        }
    }
    __syncthreads();
    for (int i = t; i < k * NC; i += kThreads) {
        const int c = i / NC, q = i % NC;
        const R a = (acc[(c * 4 + 0) * NC + q] + acc[(c * 4 + 1) * NC + q]) + (acc[(c * 4 + 2) * NC + q] + acc[(c * 4 + 3) * NC + q]);
        part[((long long)c * G + wg) * NC + q] = a;
    }
}

template <typename R, int NC, int VE, bool A16>
__global__ void __launch_bounds__(kThreads)
    sweep_kernel(long long n, int k, const R *__restrict__ V, long long ldv, R *__restrict__ w, const R *__restrict__ part,
                 R *__restrict__ hsum, R *__restrict__ nrmpart, long long lo, long long ng) {
    constexpr int GC = VE * NC;
    __shared__ R hs[BSM_GMRES_MAX_RESTART * NC];
    __shared__ R red[4][1];
    const int t = threadIdx.x, G = gridDim.x, wg = blockIdx.x;
    if (k > 0) {
        int c;
        R a[NC];
        if (gs_sum_partials<R, NC>(part, k, G, t, kThreads, c, a)) {
#pragma unroll
            for (int q = 0; q < NC; ++q) {
                hs[c * NC + q] = -a[q];
                if (wg == 0 && hsum) hsum[c * NC + q] += a[q];
            }
        }
    }
    __syncthreads();
    R nn[1] = {R(0)};
    long long g0, g1;
    wg_range(ng, G, wg, g0, g1);
    for (long long tile = g0; tile < g1; tile += (long long)kThreads * kU) {
        R wv[kU][GC];
        long long e0[kU];
        bool ok[kU];
#pragma unroll
        for (int u = 0; u < kU; ++u) {
            const long long g = tile + (long long)u * kThreads + t;
            ok[u] = g < g1;
            e0[u] = lo + g * VE;
            load_group<R, NC, VE, A16>(w, e0[u], n, ok[u], wv[u]);
        }
        for (int c0 = 0; c0 < k; c0 += kCB) {
            R vv[kCB][kU][GC];
#pragma unroll
            for (int cc = 0; cc < kCB; ++cc)
#pragma unroll
                for (int u = 0; u < kU; ++u)
                    load_group<R, NC, VE, A16>(V + (long long)(c0 + cc) * ldv * NC, e0[u], n, ok[u] && c0 + cc < k, vv[cc][u]);
#pragma unroll
            for (int cc = 0; cc < kCB; ++cc) {
                if (c0 + cc < k) {
                    const R hr = hs[(c0 + cc) * NC], hi = hs[(c0 + cc) * NC + NC - 1];
#pragma unroll
                    for (int u = 0; u < kU; ++u) gs_axpy<R, NC, VE>(vv[cc][u], hr, hi, wv[u]);
                }
            }
        }
#pragma unroll
        for (int u = 0; u < kU; ++u) {
            // (a group in front of the vector or behind it holds zeros where it is outside: they add nothing)
#pragma unroll
            for (int q = 0; q < GC; ++q) nn[0] = fma(wv[u][q], wv[u][q], nn[0]);
            store_group<R, NC, VE, A16>(w, e0[u], n, ok[u], wv[u]);
        }
    }
    if (nrmpart) {
        block_sum<R, 1>(nn, red);
        if (t == 0) nrmpart[wg] = nn[0];
    }
}

template <typename R> __global__ void __launch_bounds__(64) norm_kernel(int G, const R *__restrict__ nrmpart, R *__restrict__ nrm) {
    const R a = wave_total(nrmpart, G, 1, (int)threadIdx.x);
    if (threadIdx.x == 0) nrm[0] = sqrt(a);
}

// whether 16-byte groups serve w and the k columns of V, and where the first one starts
struct Split {
    bool a16;
    long long lo, ng;
};
Split split_of(long long n, int es, long long ldv, int k, const void *V, const void *w) {
    const int ve = 16 / es;
    const uintptr_t f = (uintptr_t)w;
    bool ok = f % (uintptr_t)es == 0;
    if (k > 0) ok = ok && ((uintptr_t)V - f) % 16 == 0 && (k == 1 || (ldv * es) % 16 == 0);
    Split s;
    s.a16 = ok;
    if (!ok) {
        s.lo = 0;
        s.ng = n;
        return s;
    }
    const long long head = (long long)(((16 - f % 16) % 16) / (uintptr_t)es);  // elements in front of the first boundary
    s.lo = head > 0 ? head - ve : 0;
    s.ng = (n - s.lo + ve - 1) / ve;
    return s;
}

}  // namespace

hipError_t launch_krylov_dot(int dtype, long long n, int k, const void *V, long long ldv, const void *w, void *part,
                             hipStream_t stream) {
    if (!is_vec_type(dtype) || k < 0 || k > BSM_GMRES_MAX_RESTART || n < 0) return hipErrorInvalidValue;
    if (k == 0) return hipSuccess;
    const int es = elem_bytes(dtype);
    const Split s = split_of(n, es, ldv, k, V, w);
    const dim3 grid((unsigned)krylov_grid(n, es)), block(kThreads);
    with_types(dtype, [&](auto r, auto, auto nc) {
        using R = decltype(r);
        constexpr int NC = decltype(nc)::value, VE = 16 / (int)(sizeof(R) * NC);
        auto launch = [&](auto kernel) {
            hipLaunchKernelGGL(kernel, grid, block, 0, stream, n, k, (const R *)V, ldv, (const R *)w, (R *)part, s.lo, s.ng);
        };
        if (s.a16)
            launch(dot_kernel<R, NC, VE, true>);
        else
            launch(dot_kernel<R, NC, 1, false>);
    });
    return hipGetLastError();
}

hipError_t launch_krylov_update(int dtype, long long n, int k, const void *V, long long ldv, void *w, const void *part, void *hsum,
                                void *nrmpart, hipStream_t stream) {
    if (!is_vec_type(dtype) || k < 0 || k > BSM_GMRES_MAX_RESTART || n < 0) return hipErrorInvalidValue;
    const int es = elem_bytes(dtype);
    const Split s = split_of(n, es, ldv, k, V, w);
    const dim3 grid((unsigned)krylov_grid(n, es)), block(kThreads);
    with_types(dtype, [&](auto r, auto, auto nc) {
        using R = decltype(r);
        constexpr int NC = decltype(nc)::value, VE = 16 / (int)(sizeof(R) * NC);
        auto launch = [&](auto kernel) {
            hipLaunchKernelGGL(kernel, grid, block, 0, stream, n, k, (const R *)V, ldv, (R *)w, (const R *)part, (R *)hsum, (R *)nrmpart, s.lo, s.ng);
        };
        if (s.a16)
            launch(sweep_kernel<R, NC, VE, true>);
        else
            launch(sweep_kernel<R, NC, 1, false>);
    });
    return hipGetLastError();
}

hipError_t launch_krylov_norm(int dtype, int G, const void *nrmpart, void *nrm, hipStream_t stream) {
    if (real_bytes(dtype) == 4)
        hipLaunchKernelGGL(norm_kernel<float>, dim3(1), dim3(64), 0, stream, G, (const float *)nrmpart, (float *)nrm);
    else
        hipLaunchKernelGGL(norm_kernel<double>, dim3(1), dim3(64), 0, stream, G, (const double *)nrmpart, (double *)nrm);
    return hipGetLastError();
}

}  // namespace bsm
