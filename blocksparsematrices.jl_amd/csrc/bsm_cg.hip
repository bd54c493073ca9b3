// bsm_cg.hip -- the kernels of bsm_cg_solve (include/bsm_rocm.h): preconditioned CG / COCG on K right-hand sides in
// lockstep.  Kept out of the product kernel units like bsm_krylov.hip: the build id (Makefile BUILD_ID) names the kernels
// and schedule of the PRODUCTS.
// (No counterpart in the reference: its operators are LinearMaps handed to a Julia solver package.)
//
// Every kernel is a pure stream over n x K elements with a reduction, in the conventions of bsm_krylov.hip: 256-thread
// workgroups, the krylov_grid(n, es) row ranges walked in tiles of 256 threads x kU 16-byte groups, xor-shuffles for the
// wave sum, one LDS slot per wave, one partial per workgroup (the helpers, from the 16-byte access to the decision of a
// column: bsm_lockstep_device.h, shared with bsm_bicgstab.hip and bsm_gmres_multi.hip).  The launch is (krylov_grid, K): a
// workgroup owns one row range of ONE column, so K columns fill the compute units where one column of n = 100 000 gives 98
// workgroups.
//   start_kernel   r = B - q (B element by element under a guard: any ldb, any alignment; q = A x0 or none), the shares of
//                  ||b||^2, ||r||^2 and, without M, of <r, r> in the method's form.
//   copy_kernel    the strided, guarded copy between the caller's X and the workspace X (both directions).
//   dot_kernel     the shares of <u_c, v_c>: conj(u) v for CG, u v for COCG (sgn = +1 / -1 on the ui vi terms).
//   update_kernel  pq = the column's G partials of <p, q> added in a fixed order by every wave for itself; alpha = rz / pq;
//                  x += alpha p, r -= alpha q in one pass; the shares of ||r||^2 (and of <r, r> without M: for CG the same
//                  numbers, computed once).  pq == 0 or rz == 0: brk[c] is set and nothing else is written.
//   dir_kernel     rn = sqrt(sum of the shares), rz' likewise; the decision against tol_c (first launch of a solve: tol_c
//                  from the shares of ||b||^2); running columns get p = z + (rz' / rz) p.  Workgroup 0 of the column writes
//                  the OTHER parity slot of the state and the record the host reads.
// The workspace vectors carry zero padding up to whole 16-byte groups (bsm_cg.h), so no load or store on them is guarded.
// A frozen column's workgroups return before their first vector load.  Every sum has a fixed order: results are
// bit-identical from run to run where the products are.  Device values are written with ordinary vector stores only.
#include "bsm_cg.h"

#include "../../include/bsm_rocm.h"
#include "bsm_lockstep_device.h"

namespace bsm {
namespace {

template <typename R, int NC, bool RR>
__global__ void __launch_bounds__(kThreads)
    start_kernel(long long n, long long ld, long long ng, long long ldb, R sgn, const R *__restrict__ B, const R *__restrict__ q,
                 R *__restrict__ r, R *__restrict__ pbb, R *__restrict__ pnn, R *__restrict__ prz, CgState *__restrict__ st) {
    constexpr int GC = 16 / (int)sizeof(R);
    __shared__ R red[4][4];
    const int t = threadIdx.x, G = gridDim.x, wg = blockIdx.x, c = blockIdx.y;
    const R *Bc = B + (long long)c * ldb * NC;
    const R *qc = q ? q + (long long)c * ld * NC : nullptr;
    R *rc = r + (long long)c * ld * NC;
    R s[4] = {R(0), R(0), R(0), R(0)};  // ||b||^2, ||r||^2, the form's re, im
    long long g0, g1;
    wg_range(ng, G, wg, g0, g1);
    for (long long tile = g0; tile < g1; tile += (long long)kThreads * kU) {
#pragma unroll
        for (int u = 0; u < kU; ++u) {
            const long long g = tile + (long long)u * kThreads + t;
            if (g >= g1) continue;
            Vec16<R> v = load16_guarded<R, NC>(Bc, g, n);
            norm16(v, s[0]);
            if (qc) sub16(v, load16(qc + g * GC));
            norm16(v, s[1]);
            if (NC == 2 && RR) form16(v, sgn, s + 2);
            store16(rc + g * GC, v);
        }
    }
    block_sum<R, 4>(s, red);
    if (t == 0) {
        pbb[(long long)c * G + wg] = s[0];
        pnn[(long long)c * G + wg] = s[1];
        if (RR) {
            // (CG: <r, r> IS ||r||^2 -- the same numbers, so computed once)
            prz[((long long)c * G + wg) * NC] = (NC == 1 || sgn > R(0)) ? s[1] : s[2];
            if (NC == 2) prz[((long long)c * G + wg) * NC + NC - 1] = sgn > R(0) ? R(0) : s[3];
        }
        if (wg == 0) st->brk[c] = 0;
    }
}

template <typename R, int NC, bool TO_WS>
__global__ void __launch_bounds__(kThreads) copy_kernel(long long n, long long ld, long long ng, long long ldx, R *__restrict__ X,
                                                        R *__restrict__ ws) {
    constexpr int GC = 16 / (int)sizeof(R), VE = GC / NC;
    const int t = threadIdx.x, G = gridDim.x, wg = blockIdx.x, c = blockIdx.y;
    R *Xc = X + (long long)c * ldx * NC;
    R *wc = ws + (long long)c * ld * NC;
    long long g0, g1;
    wg_range(ng, G, wg, g0, g1);
    for (long long g = g0 + t; g < g1; g += kThreads) {
        if (TO_WS) {
            store16(wc + g * GC, load16_guarded<R, NC>(Xc, g, n));
            continue;
        }
        const Vec16<R> v = load16(wc + g * GC);
#pragma unroll
        for (int e = 0; e < VE; ++e) {
            const long long row = g * VE + e;
#pragma unroll
            for (int k = 0; k < NC; ++k)
                if (row < n) Xc[row * NC + k] = v.r[e * NC + k];
        }
    }
}

template <typename R, int NC>
__global__ void __launch_bounds__(kThreads) dot_kernel(long long ld, long long ng, R sgn, int par, const R *__restrict__ u,
                                                       const R *__restrict__ v, R *__restrict__ part, const CgState *__restrict__ st) {
    constexpr int GC = 16 / (int)sizeof(R);
    __shared__ R red[4][NC];
    const int t = threadIdx.x, G = gridDim.x, wg = blockIdx.x, c = blockIdx.y;
    if (par >= 0 && st->slot[par].status[c] != kCgRun) return;
    const R *uc = u + (long long)c * ld * NC, *vc = v + (long long)c * ld * NC;
    R s[NC];
#pragma unroll
    for (int k = 0; k < NC; ++k) s[k] = R(0);
    long long g0, g1;
    wg_range(ng, G, wg, g0, g1);
    for (long long tile = g0; tile < g1; tile += (long long)kThreads * kU * 2) {
        Vec16<R> a[kU * 2], b[kU * 2];
#pragma unroll
        for (int i = 0; i < kU * 2; ++i) {
            const long long g = tile + (long long)i * kThreads + t;
            if (g < g1) {
                a[i] = load16(uc + g * GC);
                b[i] = load16(vc + g * GC);
            } else {
                a[i] = b[i] = zero16<R>();
            }
        }
#pragma unroll
        for (int i = 0; i < kU * 2; ++i) dot16<R, NC>(a[i], b[i], sgn, s);
    }
    block_sum<R, NC>(s, red);
    if (t == 0) {
#pragma unroll
        for (int k = 0; k < NC; ++k) part[((long long)c * G + wg) * NC + k] = s[k];
    }
}

template <typename R, int NC, bool RR>
__global__ void __launch_bounds__(kThreads)
    update_kernel(long long ld, long long ng, R sgn, int par, const R *__restrict__ ppq, const R *__restrict__ p, const R *__restrict__ q,
                  R *__restrict__ x, R *__restrict__ r, R *__restrict__ pnn, R *__restrict__ prz, CgState *__restrict__ st) {
    constexpr int GC = 16 / (int)sizeof(R);
    __shared__ R red[4][3];
    const int t = threadIdx.x, lane = t & 63, G = gridDim.x, wg = blockIdx.x, c = blockIdx.y;
    if (st->slot[par].status[c] != kCgRun) return;
    R pq[2] = {R(0), R(0)}, rz[2], al[2] = {R(0), R(0)};
    // (not column_total: behind it the compiler contracts the a c + b e of k_div the other way round in the complex float
    // instantiations -- which product is rounded before the fma -- and alpha of COCG changes in its last bit,
    // docs/experiments_r27.md)
#pragma unroll
    for (int k = 0; k < NC; ++k) pq[k] = wave_total(ppq + (long long)c * G * NC + k, G, NC, lane);
    rz[0] = (R)st->slot[par].rz[c][0];
    rz[1] = (R)st->slot[par].rz[c][1];
    if (is_zero<R, NC>(pq) || is_zero<R, NC>(rz)) {  // breakdown: cg_dir freezes the column; no division is executed
        if (wg == 0 && t == 0) st->brk[c] = 1;
        return;
    }
    k_div<R, NC>(rz, pq, al);
    const R ar = al[0], ai = al[NC - 1];
    const long long off = (long long)c * ld * NC;
    R s[3] = {R(0), R(0), R(0)};  // ||r||^2, the form's re, im
    long long g0, g1;
    wg_range(ng, G, wg, g0, g1);
    for (long long tile = g0; tile < g1; tile += (long long)kThreads * kU) {
        Vec16<R> xv[kU], pv[kU], rv[kU], qv[kU];
#pragma unroll
        for (int u = 0; u < kU; ++u) {
            const long long g = tile + (long long)u * kThreads + t;
            if (g < g1) {
                xv[u] = load16(x + off + g * GC);
                pv[u] = load16(p + off + g * GC);
                rv[u] = load16(r + off + g * GC);
                qv[u] = load16(q + off + g * GC);
            }
        }
#pragma unroll
        for (int u = 0; u < kU; ++u) {
            const long long g = tile + (long long)u * kThreads + t;
            if (g >= g1) continue;
            axpy16<R, NC>(ar, ai, pv[u], xv[u]);
            axpy16<R, NC>(-ar, -ai, qv[u], rv[u]);
            norm16(rv[u], s[0]);
            if (NC == 2 && RR) form16(rv[u], sgn, s + 1);
            store16(x + off + g * GC, xv[u]);
            store16(r + off + g * GC, rv[u]);
        }
    }
    block_sum<R, 3>(s, red);
    if (t == 0) {
        pnn[(long long)c * G + wg] = s[0];
        if (RR) {
            prz[((long long)c * G + wg) * NC] = (NC == 1 || sgn > R(0)) ? s[0] : s[1];
            if (NC == 2) prz[((long long)c * G + wg) * NC + NC - 1] = sgn > R(0) ? R(0) : s[2];
        }
    }
}

template <typename R, int NC>
__global__ void __launch_bounds__(kThreads)
    dir_kernel(long long ld, long long ng, int first, int par, long long it, double rtol, double atol, const R *__restrict__ pbb,
               const R *__restrict__ pnn, const R *__restrict__ prz, const R *__restrict__ z, R *__restrict__ p, CgState *__restrict__ st) {
    constexpr int GC = 16 / (int)sizeof(R);
    const int t = threadIdx.x, lane = t & 63, G = gridDim.x, wg = blockIdx.x, c = blockIdx.y;
    const bool writer = wg == 0 && t == 0;
    const CgSlot &in = st->slot[par];
    CgSlot &out = st->slot[first ? 0 : par ^ 1];
    if (!first) {
        const int so = in.status[c];
        const bool broke = so == kCgRun && st->brk[c] != 0;
        if (so != kCgRun || broke) {  // frozen before this iteration, or by its cg_update: the state moves to the other slot
            if (writer) carry_frozen(in, out, st->rec, c, broke ? 3 : so);
            return;
        }
    }
    const R rn = sqrt(wave_total(pnn + (long long)c * G, G, 1, lane));
    R rzn[2] = {R(0), R(0)}, bn = R(0);
    column_total<R, NC>(prz, c, G, lane, rzn);
    const double tol = first ? first_tol(pbb + (long long)c * G, G, lane, rtol, atol, bn) : st->tol[c];
    const int status = decide(rn, tol);
    if (writer) {
        out.rz[c][0] = (double)rzn[0];
        out.rz[c][1] = (double)rzn[1];
        out.rn[c] = (double)rn;
        out.status[c] = status;
        out.done[c] = (int32_t)it;
        if (first) {
            st->tol[c] = tol;
            st->rec.bnorm[c] = (double)bn;
        }
        st->rec.rn[c] = (double)rn;
        st->rec.status[c] = status;
        st->rec.done[c] = (int32_t)it;
    }
    if (status != kCgRun) return;
    R be[2] = {R(0), R(0)};
    if (!first) {
        const R rzo[2] = {(R)in.rz[c][0], (R)in.rz[c][1]};
        k_div<R, NC>(rzn, rzo, be);  // (rzo != 0: cg_update of this iteration checked it)
    }
    const R br = be[0], bi = be[NC - 1];
    const long long off = (long long)c * ld * NC;
    long long g0, g1;
    wg_range(ng, G, wg, g0, g1);
    for (long long tile = g0; tile < g1; tile += (long long)kThreads * kU) {
        Vec16<R> zv[kU], pv[kU];
#pragma unroll
        for (int u = 0; u < kU; ++u) {
            const long long g = tile + (long long)u * kThreads + t;
            if (g < g1) {
                zv[u] = load16(z + off + g * GC);
                if (!first) pv[u] = load16(p + off + g * GC);
            }
        }
#pragma unroll
        for (int u = 0; u < kU; ++u) {
            const long long g = tile + (long long)u * kThreads + t;
            if (g >= g1) continue;
            if (!first) axpy16<R, NC>(br, bi, pv[u], zv[u]);
            store16(p + off + g * GC, zv[u]);
        }
    }
}

}  // namespace

hipError_t launch_cg_start(const CgDims &d, const void *B, long long ldb, const void *q, void *r, void *pbb, void *pnn, void *prz,
                           CgState *st, hipStream_t stream) {
    return cg_dispatch(d, [&](auto rt, auto nc, long long ng, dim3 grid, auto sgn) {
        using R = decltype(rt);
        constexpr int NC = decltype(nc)::value;
        auto launch = [&](auto kernel) {
            hipLaunchKernelGGL(kernel, grid, dim3(kThreads), 0, stream, d.n, d.ld, ng, ldb, sgn, (const R *)B, (const R *)q, (R *)r,
                               (R *)pbb, (R *)pnn, (R *)prz, st);
        };
        if (prz)
            launch(start_kernel<R, NC, true>);
        else
            launch(start_kernel<R, NC, false>);
    });
}

hipError_t launch_cg_copy(const CgDims &d, bool to_ws, void *X, long long ldx, void *ws, hipStream_t stream) {
    return cg_dispatch(d, [&](auto rt, auto nc, long long ng, dim3 grid, auto) {
        using R = decltype(rt);
        constexpr int NC = decltype(nc)::value;
        if (to_ws)
            hipLaunchKernelGGL((copy_kernel<R, NC, true>), grid, dim3(kThreads), 0, stream, d.n, d.ld, ng, ldx, (R *)X, (R *)ws);
        else
            hipLaunchKernelGGL((copy_kernel<R, NC, false>), grid, dim3(kThreads), 0, stream, d.n, d.ld, ng, ldx, (R *)X, (R *)ws);
    });
}

hipError_t launch_cg_dot(const CgDims &d, int par, const void *u, const void *v, void *part, const CgState *st, hipStream_t stream) {
    return cg_dispatch(d, [&](auto rt, auto nc, long long ng, dim3 grid, auto sgn) {
        using R = decltype(rt);
        constexpr int NC = decltype(nc)::value;
        hipLaunchKernelGGL((dot_kernel<R, NC>), grid, dim3(kThreads), 0, stream, d.ld, ng, sgn, par, (const R *)u, (const R *)v, (R *)part, st);
    });
}

hipError_t launch_cg_update(const CgDims &d, int par, const void *ppq, const void *p, const void *q, void *x, void *r, void *pnn,
                            void *prz, CgState *st, hipStream_t stream) {
    return cg_dispatch(d, [&](auto rt, auto nc, long long ng, dim3 grid, auto sgn) {
        using R = decltype(rt);
        constexpr int NC = decltype(nc)::value;
        auto launch = [&](auto kernel) {
            hipLaunchKernelGGL(kernel, grid, dim3(kThreads), 0, stream, d.ld, ng, sgn, par, (const R *)ppq, (const R *)p, (const R *)q,
                               (R *)x, (R *)r, (R *)pnn, (R *)prz, st);
        };
        if (prz)
            launch(update_kernel<R, NC, true>);
        else
            launch(update_kernel<R, NC, false>);
    });
}

hipError_t launch_cg_dir(const CgDims &d, bool first, int par, long long it, double rtol, double atol, const void *pbb, const void *pnn,
                         const void *prz, const void *z, void *p, CgState *st, hipStream_t stream) {
    return cg_dispatch(d, [&](auto rt, auto nc, long long ng, dim3 grid, auto) {
        using R = decltype(rt);
        constexpr int NC = decltype(nc)::value;
        hipLaunchKernelGGL((dir_kernel<R, NC>), grid, dim3(kThreads), 0, stream, d.ld, ng, first ? 1 : 0, par, it, rtol, atol,
                           (const R *)pbb, (const R *)pnn, (const R *)prz, (const R *)z, (R *)p, st);
    });
}

}  // namespace bsm
