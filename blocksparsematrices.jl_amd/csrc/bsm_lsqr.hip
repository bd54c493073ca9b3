// bsm_lsqr.hip -- the kernels of bsm_lsqr_solve (include/bsm_rocm.h): LSQR on K right-hand sides in lockstep, for
// rectangular, rank-deficient and damped least-squares problems.  Kept out of the product kernel units like bsm_cg.hip: the
// build id (Makefile BUILD_ID) names the kernels and schedule of the PRODUCTS.
// (No counterpart in the reference: its operators are LinearMaps handed to a Julia solver package.)
//
// The conventions are those of bsm_cg.hip: 256-thread workgroups, row ranges walked in tiles of 256 threads x kU 16-byte
// groups, one partial per workgroup and column, every consumer adding a column's partials itself (the helpers:
// bsm_lockstep_device.h).  What is new is that a solve has TWO grids (bsm_lsqr.h): the vectors of B's length are walked by
// (krylov_grid(m), K) launches, those of X's length by (krylov_grid(n), K) launches, and a kernel of the n-grid that needs
// ||u||^2 adds the Gm partials the m-grid left.  The decision is (1, K), one wave per column.  Every scalar of the method is
// real, so the kernels but the start walk a column as reals, 16 bytes at a time.
//   start_kernel   (m) u = B - q (B element by element under a guard), the shares of ||b||^2 and ||u||^2
//   begin_kernel   (n) beta from the shares;  v = p / beta;  the shares of ||v||^2
//   u_kernel       (m) u = q / alpha - (alpha / beta) u;  the shares of ||u||^2
//   v_kernel       (n) beta' from the shares;  at iteration 0 w = v / alpha;  v = p / beta' - (beta' / alpha) v;  the shares of ||v||^2
//   update_kernel  (n) alpha', beta' from the shares and lsqr_step (bsm_lsqr.h) by every workgroup for itself;  x, w in one
//                  pass;  workgroup 0 leaves the step
//   decide_kernel  moves the step into the OTHER parity slot of the state and writes the record the host reads (first launch
//                  of a solve: tol_c, the norms and the decision of iteration 0);  carries frozen columns over
// A frozen column's workgroups return before their first vector load.  Every sum has a fixed order: results are
// bit-identical from run to run where the products are.  Device values are written with ordinary vector stores only.
#include "bsm_lsqr.h"

#include "../../include/bsm_rocm.h"
#include "bsm_lockstep_device.h"

namespace bsm {
namespace {

template <typename R, int NC>
__global__ void __launch_bounds__(kThreads) start_kernel(long long m, long long ng, long long ldb, const R *__restrict__ B,
                                                         const R *__restrict__ q, R *__restrict__ u, R *__restrict__ pbb, R *__restrict__ pu) {
    constexpr int GC = 16 / (int)sizeof(R);
    __shared__ R red[4][2];
    const int t = threadIdx.x, G = gridDim.x, wg = blockIdx.x, c = blockIdx.y;
    const R *Bc = B + (long long)c * ldb * NC;
    const long long off = (long long)c * ng * GC;
    R s[2] = {R(0), R(0)};  // ||b||^2, ||u||^2
    long long g0, g1;
    wg_range(ng, G, wg, g0, g1);
    for (long long tile = g0; tile < g1; tile += (long long)kThreads * kU) {
#pragma unroll
        for (int i = 0; i < kU; ++i) {
            const long long g = tile + (long long)i * kThreads + t;
            if (g >= g1) continue;
            Vec16<R> b = load16_guarded<R, NC>(Bc, g, m);
            norm16(b, s[0]);
            if (q) sub16(b, load16(q + off + g * GC));
            norm16(b, s[1]);
            store16(u + off + g * GC, b);
        }
    }
    block_sum<R, 2>(s, red);
    if (t == 0) {
        pbb[(long long)c * G + wg] = s[0];
        pu[(long long)c * G + wg] = s[1];
    }
}

template <typename R>
__global__ void __launch_bounds__(kThreads) begin_kernel(long long ng, int Gm, const R *__restrict__ pu, const R *__restrict__ p,
                                                         R *__restrict__ v, R *__restrict__ pv) {
    constexpr int GC = 16 / (int)sizeof(R);
    __shared__ R red[4][1];
    const int t = threadIdx.x, lane = t & 63, G = gridDim.x, wg = blockIdx.x, c = blockIdx.y;
    const R uu = wave_total(pu + (long long)c * Gm, Gm, 1, lane);
    const R ib = uu > R(0) && isfinite(uu) ? R(1) / sqrt(uu) : R(1);
    const long long off = (long long)c * ng * GC;
    R s[1] = {R(0)};
    long long g0, g1;
    wg_range(ng, G, wg, g0, g1);
    for (long long tile = g0; tile < g1; tile += (long long)kThreads * kU) {
        Vec16<R> pp[kU];
#pragma unroll
        for (int i = 0; i < kU; ++i) {
            const long long g = tile + (long long)i * kThreads + t;
            if (g < g1) pp[i] = load16(p + off + g * GC);
        }
#pragma unroll
        for (int i = 0; i < kU; ++i) {
            const long long g = tile + (long long)i * kThreads + t;
            if (g >= g1) continue;
            scale16(pp[i], ib);
            norm16(pp[i], s[0]);
            store16(v + off + g * GC, pp[i]);
        }
    }
    block_sum<R, 1>(s, red);
    if (t == 0) pv[(long long)c * G + wg] = s[0];
}

template <typename R>
__global__ void __launch_bounds__(kThreads) u_kernel(long long ng, int par, const R *__restrict__ q, R *__restrict__ u, R *__restrict__ pu,
                                                     const LsState *__restrict__ st) {
    constexpr int GC = 16 / (int)sizeof(R);
    __shared__ R red[4][1];
    const int t = threadIdx.x, G = gridDim.x, wg = blockIdx.x, c = blockIdx.y;
    const LsSlot &in = st->slot[par];
    if (in.status[c] != kCgRun) return;
    // (alpha, beta > 0 and finite on a running column: ls_decide froze every other one)
    const R al = (R)in.alpha[c], ia = R(1) / al, co = al / (R)in.beta[c];
    const long long off = (long long)c * ng * GC;
    R s[1] = {R(0)};
    long long g0, g1;
    wg_range(ng, G, wg, g0, g1);
    for (long long tile = g0; tile < g1; tile += (long long)kThreads * kU) {
        Vec16<R> qv[kU], uv[kU];
#pragma unroll
        for (int i = 0; i < kU; ++i) {
            const long long g = tile + (long long)i * kThreads + t;
            if (g < g1) {
                qv[i] = load16(q + off + g * GC);
                uv[i] = load16(u + off + g * GC);
            }
        }
#pragma unroll
        for (int i = 0; i < kU; ++i) {
            const long long g = tile + (long long)i * kThreads + t;
            if (g >= g1) continue;
#pragma unroll
            for (int k = 0; k < GC; ++k) uv[i].r[k] = ia * qv[i].r[k] - co * uv[i].r[k];
            norm16(uv[i], s[0]);
            store16(u + off + g * GC, uv[i]);
        }
    }
    block_sum<R, 1>(s, red);
    if (t == 0) pu[(long long)c * G + wg] = s[0];
}

template <typename R, bool FIRST>
__global__ void __launch_bounds__(kThreads) v_kernel(long long ng, int par, int Gm, const R *__restrict__ pu, const R *__restrict__ p,
                                                     R *__restrict__ v, R *__restrict__ w, R *__restrict__ pv,
                                                     const LsState *__restrict__ st) {
    constexpr int GC = 16 / (int)sizeof(R);
    __shared__ R red[4][1];
    const int t = threadIdx.x, lane = t & 63, G = gridDim.x, wg = blockIdx.x, c = blockIdx.y;
    const LsSlot &in = st->slot[par];
    if (in.status[c] != kCgRun) return;
    const R bn = sqrt(wave_total(pu + (long long)c * Gm, Gm, 1, lane));
    const R ia = R(1) / (R)in.alpha[c];
    // beta' == 0: the Krylov space ended, v_new = 0 and no division (a beta' that is not finite goes through: ls_decide
    // sees it in the estimates)
    const R ib = bn == R(0) ? R(0) : R(1) / bn, co = bn * ia;
    const long long off = (long long)c * ng * GC;
    R s[1] = {R(0)};
    long long g0, g1;
    wg_range(ng, G, wg, g0, g1);
    for (long long tile = g0; tile < g1; tile += (long long)kThreads * kU) {
        Vec16<R> pp[kU], vv[kU];
#pragma unroll
        for (int i = 0; i < kU; ++i) {
            const long long g = tile + (long long)i * kThreads + t;
            if (g < g1) {
                pp[i] = load16(p + off + g * GC);
                vv[i] = load16(v + off + g * GC);
            }
        }
#pragma unroll
        for (int i = 0; i < kU; ++i) {
            const long long g = tile + (long long)i * kThreads + t;
            if (g >= g1) continue;
            if (FIRST) {
                Vec16<R> wv = vv[i];
                scale16(wv, ia);
                store16(w + off + g * GC, wv);
            }
#pragma unroll
            for (int k = 0; k < GC; ++k) vv[i].r[k] = bn == R(0) ? R(0) : ib * pp[i].r[k] - co * vv[i].r[k];
            norm16(vv[i], s[0]);
            store16(v + off + g * GC, vv[i]);
        }
    }
    block_sum<R, 1>(s, red);
    if (t == 0) pv[(long long)c * G + wg] = s[0];
}

template <typename R>
__global__ void __launch_bounds__(kThreads) update_kernel(long long ng, int par, int Gm, double damp, double ntol, const R *__restrict__ pu,
                                                          const R *__restrict__ pv, const R *__restrict__ v, R *__restrict__ w,
                                                          R *__restrict__ x, LsState *__restrict__ st) {
    constexpr int GC = 16 / (int)sizeof(R);
    const int t = threadIdx.x, lane = t & 63, G = gridDim.x, wg = blockIdx.x, c = blockIdx.y;
    const LsSlot &in = st->slot[par];
    if (in.status[c] != kCgRun) return;
    const R bn = sqrt(wave_total(pu + (long long)c * Gm, Gm, 1, lane));
    const R an = sqrt(wave_total(pv + (long long)c * G, G, 1, lane));
    const LsqrScalars<R> cur{(R)in.alpha[c], (R)in.beta[c], (R)in.phibar[c], (R)in.rhobar[c], (R)in.res2[c], (R)in.anorm[c]};
    LsqrStep<R> step;
    lsqr_step(cur, bn, an, (R)damp, st->tol[c], ntol, step);
    if (wg == 0 && t == 0) {
        LsStepState &o = st->step;
        o.alpha[c] = (double)step.next.alpha, o.beta[c] = (double)step.next.beta;
        o.phibar[c] = (double)step.next.phibar, o.rhobar[c] = (double)step.next.rhobar;
        o.res2[c] = (double)step.next.res2, o.anorm[c] = (double)step.next.anorm;
        o.rnorm[c] = (double)step.rnorm, o.arnorm[c] = (double)step.arnorm;
        o.status[c] = step.status;
    }
    const R cx = step.cx, cw = step.cw, ia = an == R(0) ? R(0) : R(1) / an;
    const long long off = (long long)c * ng * GC;
    long long g0, g1;
    wg_range(ng, G, wg, g0, g1);
    for (long long tile = g0; tile < g1; tile += (long long)kThreads * kU) {
        Vec16<R> vv[kU], wv[kU], xv[kU];
#pragma unroll
        for (int i = 0; i < kU; ++i) {
            const long long g = tile + (long long)i * kThreads + t;
            if (g < g1) {
                vv[i] = load16(v + off + g * GC);
                wv[i] = load16(w + off + g * GC);
                xv[i] = load16(x + off + g * GC);
            }
        }
#pragma unroll
        for (int i = 0; i < kU; ++i) {
            const long long g = tile + (long long)i * kThreads + t;
            if (g >= g1) continue;
#pragma unroll
            for (int k = 0; k < GC; ++k) {
                xv[i].r[k] += cx * wv[i].r[k];
                wv[i].r[k] = ia * vv[i].r[k] - cw * wv[i].r[k];
            }
            store16(x + off + g * GC, xv[i]);
            store16(w + off + g * GC, wv[i]);
        }
    }
}

template <typename R>
__global__ void __launch_bounds__(64) decide_kernel(int Gn, int first, int par, long long it, int Gm, double rtol, double atol, double ntol,
                                                    const R *__restrict__ pbb, const R *__restrict__ pu, const R *__restrict__ pv,
                                                    LsState *__restrict__ st) {
    const int lane = threadIdx.x, c = blockIdx.y;
    const bool writer = lane == 0;
    const LsSlot &in = st->slot[par];
    LsSlot &out = st->slot[first ? 0 : par ^ 1];
    if (first) {
        R bnorm = R(0);
        const double tol = first_tol(pbb + (long long)c * Gm, Gm, lane, rtol, atol, bnorm);
        const R uu = wave_total(pu + (long long)c * Gm, Gm, 1, lane), vv = wave_total(pv + (long long)c * Gn, Gn, 1, lane);
        const R beta = sqrt(uu), alpha = sqrt(vv);
        const R arn = alpha * beta;
        const int status = lsqr_decide(beta, arn, R(0), alpha, beta, tol, ntol);
        if (!writer) return;
        out.alpha[c] = (double)alpha, out.beta[c] = (double)beta, out.phibar[c] = (double)beta, out.rhobar[c] = (double)alpha;
        out.res2[c] = 0, out.anorm[c] = 0, out.rnorm[c] = (double)beta, out.arnorm[c] = (double)arn;
        out.status[c] = status;
        out.done[c] = 0;
        st->tol[c] = tol;
        st->rec.bnorm[c] = (double)bnorm;
        st->rec.rn[c] = (double)beta;
        st->rec.status[c] = status;
        st->rec.done[c] = 0;
        return;
    }
    if (!writer) return;
    const bool ran = in.status[c] == kCgRun;
    const LsStepState &s = st->step;
    // a column frozen before this iteration moves to the other slot as it is; a running one takes what ls_update left
    out.alpha[c] = ran ? s.alpha[c] : in.alpha[c], out.beta[c] = ran ? s.beta[c] : in.beta[c];
    out.phibar[c] = ran ? s.phibar[c] : in.phibar[c], out.rhobar[c] = ran ? s.rhobar[c] : in.rhobar[c];
    out.res2[c] = ran ? s.res2[c] : in.res2[c], out.anorm[c] = ran ? s.anorm[c] : in.anorm[c];
    out.rnorm[c] = ran ? s.rnorm[c] : in.rnorm[c], out.arnorm[c] = ran ? s.arnorm[c] : in.arnorm[c];
    const int status = ran ? s.status[c] : in.status[c];
    out.status[c] = status;
    out.done[c] = ran ? (int32_t)it : in.done[c];
    st->rec.status[c] = status;
    if (ran) {
        st->rec.rn[c] = s.rnorm[c];
        st->rec.done[c] = (int32_t)it;
    }
}

}  // namespace

hipError_t launch_ls_start(const CgDims &dm, const void *B, long long ldb, const void *q, void *u, void *pbb, void *pu, hipStream_t stream) {
    return cg_dispatch(dm, [&](auto rt, auto nc, long long ng, dim3 grid, auto) {
        using R = decltype(rt);
        constexpr int NC = decltype(nc)::value;
        hipLaunchKernelGGL((start_kernel<R, NC>), grid, dim3(kThreads), 0, stream, dm.n, ng, ldb, (const R *)B, (const R *)q, (R *)u, (R *)pbb,
                           (R *)pu);
    });
}

hipError_t launch_ls_begin(const CgDims &dn, int Gm, const void *pu, const void *p, void *v, void *pv, hipStream_t stream) {
    return cg_dispatch(dn, [&](auto rt, auto, long long ng, dim3 grid, auto) {
        using R = decltype(rt);
        hipLaunchKernelGGL((begin_kernel<R>), grid, dim3(kThreads), 0, stream, ng, Gm, (const R *)pu, (const R *)p, (R *)v, (R *)pv);
    });
}

hipError_t launch_ls_u(const CgDims &dm, int par, const void *q, void *u, void *pu, const LsState *st, hipStream_t stream) {
    return cg_dispatch(dm, [&](auto rt, auto, long long ng, dim3 grid, auto) {
        using R = decltype(rt);
        hipLaunchKernelGGL((u_kernel<R>), grid, dim3(kThreads), 0, stream, ng, par, (const R *)q, (R *)u, (R *)pu, st);
    });
}

hipError_t launch_ls_v(const CgDims &dn, bool first, int par, int Gm, const void *pu, const void *p, void *v, void *w, void *pv,
                       const LsState *st, hipStream_t stream) {
    return cg_dispatch(dn, [&](auto rt, auto, long long ng, dim3 grid, auto) {
        using R = decltype(rt);
        auto launch = [&](auto kernel) {
            hipLaunchKernelGGL(kernel, grid, dim3(kThreads), 0, stream, ng, par, Gm, (const R *)pu, (const R *)p, (R *)v, (R *)w, (R *)pv, st);
        };
        if (first)
            launch(v_kernel<R, true>);
        else
            launch(v_kernel<R, false>);
    });
}

hipError_t launch_ls_update(const CgDims &dn, int par, int Gm, double damp, double ntol, const void *pu, const void *pv, const void *v,
                            void *w, void *x, LsState *st, hipStream_t stream) {
    return cg_dispatch(dn, [&](auto rt, auto, long long ng, dim3 grid, auto) {
        using R = decltype(rt);
        hipLaunchKernelGGL((update_kernel<R>), grid, dim3(kThreads), 0, stream, ng, par, Gm, damp, ntol, (const R *)pu, (const R *)pv,
                           (const R *)v, (R *)w, (R *)x, st);
    });
}

hipError_t launch_ls_decide(const CgDims &dn, bool first, int par, long long it, int Gm, double rtol, double atol, double ntol,
                            const void *pbb, const void *pu, const void *pv, LsState *st, hipStream_t stream) {
    return cg_dispatch(dn, [&](auto rt, auto, long long, dim3 grid, auto) {
        using R = decltype(rt);
        hipLaunchKernelGGL((decide_kernel<R>), dim3(1, grid.y), dim3(64), 0, stream, (int)grid.x, first ? 1 : 0, par, it, Gm, rtol, atol, ntol,
                           (const R *)pbb, (const R *)pu, (const R *)pv, st);
    });
}

}  // namespace bsm
