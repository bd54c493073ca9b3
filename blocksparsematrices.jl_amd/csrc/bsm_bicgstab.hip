// bsm_bicgstab.hip -- the kernels of bsm_bicgstab_solve (include/bsm_rocm.h): right-preconditioned BiCGSTAB on K right-hand
// sides in lockstep.  Kept out of the product kernel units like bsm_cg.hip: the build id (Makefile BUILD_ID) names the
// kernels and schedule of the PRODUCTS.
// (No counterpart in the reference: its operators are LinearMaps handed to a Julia solver package.)
//
// Every kernel is a pure stream over n x K elements with a reduction, in the conventions of bsm_cg.hip (whose helpers it
// shares through bsm_lockstep_device.h): 256-thread workgroups, the launch (krylov_grid, K), tiles of 256 threads x kU 16-byte
// groups, one partial per workgroup and column.  The inner product is always conjugated: <u, v> = sum conj(u_i) v_i.
//   start_kernel   r = rhat = B - q (B element by element under a guard: any ldb, any alignment; q = A x0 or none), the
//                  shares of ||b||^2 and ||r||^2 (= rho at the start).
//   dot_kernel     the shares of <u_c, v_c> and, for the second dot of an iteration, of ||u_c||^2 in the same pass:
//                  <rhat, v>, then <t, s> with ||t||^2.
//   half_kernel    alpha = rho / sigma;  x += alpha phat, r -= alpha v in one pass;  the shares of ||s||^2.
//   update_kernel  omega = <t, s> / ||t||^2;  x += omega shat, r -= omega t in one pass;  the shares of ||r||^2 and <rhat, r>.
//   dir_kernel     the decisions of the iteration (first launch of a solve: tol_c from the shares of ||b||^2, p = r); running
//                  columns get p = r + beta (p - omega v).  Workgroup 0 of the column writes the OTHER parity slot of the
//                  state and the record the host reads.
// (The copy between the caller's X and the workspace is launch_cg_copy of bsm_cg.hip.)
// No flag passes between the launches of an iteration: half, update and dir each add the partials they need in the one
// fixed order (bicg_alpha, bicg_omega below) and so take the same branch with the same alpha and omega.  A frozen column's
// workgroups return before their first vector load, and so do those of a column whose iteration has ended in an earlier
// launch of it.  The workspace vectors carry zero padding up to whole 16-byte groups (bsm_cg.h), so no load or store on
// them is guarded.  Every sum has a fixed order.  Device values are written with ordinary vector stores only.
#include "bsm_bicgstab.h"

#include "../../include/bsm_rocm.h"
#include "bsm_lockstep_device.h"

namespace bsm {
namespace {

// First half of an iteration on a column running in slot `in`: rho from the slot, sigma from its partials.  False: the
// breakdown rho == 0 or sigma == 0 (no division is executed); else al = rho / sigma.
template <typename R, int NC>
__device__ __forceinline__ bool bicg_alpha(const R *__restrict__ psig, const CgSlot &in, int c, int G, int lane, R (&rho)[2], R (&al)[2]) {
    R sig[2] = {R(0), R(0)};
    column_total<R, NC>(psig, c, G, lane, sig);
    rho[0] = (R)in.rz[c][0];
    rho[1] = (R)in.rz[c][1];
    al[0] = al[1] = R(0);
    if (is_zero<R, NC>(sig) || is_zero<R, NC>(rho)) return false;
    k_div<R, NC>(rho, sig, al);
    return true;
}
// Second half: sn = ||s|| and, in the fixed order of the checks, the status the column ends the iteration with after the
// half step -- 2 (sn not finite), 0 (sn <= tol), 3 (tt == 0, ts == 0, or their quotient underflowed to 0) -- or kCgRun
// with om = ts / tt != 0.
template <typename R, int NC>
__device__ __forceinline__ int bicg_omega(const R *__restrict__ pss, const R *__restrict__ pts, const R *__restrict__ ptt, double tol,
                                          int c, int G, int lane, R &sn, R (&om)[2]) {
    om[0] = om[1] = R(0);
    sn = sqrt(wave_total(pss + (long long)c * G, G, 1, lane));
    if (!isfinite(sn)) return 2;
    if ((double)sn <= tol) return 0;
    R ts[2] = {R(0), R(0)};
    column_total<R, NC>(pts, c, G, lane, ts);
    const R tt = wave_total(ptt + (long long)c * G, G, 1, lane);
    if (tt == R(0) || is_zero<R, NC>(ts)) return 3;
    om[0] = ts[0] / tt;
    if (NC == 2) om[NC - 1] = ts[NC - 1] / tt;
    if (is_zero<R, NC>(om)) {  // ts / tt underflowed: beta = .. / omega must not be formed
        om[0] = om[1] = R(0);
        return 3;
    }
    return kCgRun;
}

template <typename R, int NC>
__global__ void __launch_bounds__(kThreads)
    start_kernel(long long n, long long ld, long long ng, long long ldb, const R *__restrict__ B, const R *__restrict__ q, R *__restrict__ r,
                 R *__restrict__ rhat, R *__restrict__ pbb, R *__restrict__ pnn) {
    constexpr int GC = 16 / (int)sizeof(R);
    __shared__ R red[4][2];
    const int t = threadIdx.x, G = gridDim.x, wg = blockIdx.x, c = blockIdx.y;
    const R *Bc = B + (long long)c * ldb * NC;
    const long long off = (long long)c * ld * NC;
    R s[2] = {R(0), R(0)};  // ||b||^2, ||r||^2
    long long g0, g1;
    wg_range(ng, G, wg, g0, g1);
    for (long long tile = g0; tile < g1; tile += (long long)kThreads * kU) {
#pragma unroll
        for (int u = 0; u < kU; ++u) {
            const long long g = tile + (long long)u * kThreads + t;
            if (g >= g1) continue;
            Vec16<R> v = load16_guarded<R, NC>(Bc, g, n);
            norm16(v, s[0]);
            if (q) sub16(v, load16(q + off + g * GC));
            norm16(v, s[1]);
            store16(r + off + g * GC, v);
            store16(rhat + off + g * GC, v);
        }
    }
    block_sum<R, 2>(s, red);
    if (t == 0) {
        pbb[(long long)c * G + wg] = s[0];
        pnn[(long long)c * G + wg] = s[1];
    }
}

template <typename R, int NC, bool NRM>
__global__ void __launch_bounds__(kThreads) dot_kernel(long long ld, long long ng, int par, const R *__restrict__ u, const R *__restrict__ v,
                                                       R *__restrict__ part, R *__restrict__ nrm, const CgState *__restrict__ st) {
    constexpr int GC = 16 / (int)sizeof(R);
    __shared__ R red[4][3];
    const int t = threadIdx.x, G = gridDim.x, wg = blockIdx.x, c = blockIdx.y;
    if (st->slot[par].status[c] != kCgRun) return;
    const long long off = (long long)c * ld * NC;
    R s[3] = {R(0), R(0), R(0)};  // the form's re, im; ||u||^2
    long long g0, g1;
    wg_range(ng, G, wg, g0, g1);
    for (long long tile = g0; tile < g1; tile += (long long)kThreads * kU * 2) {
        Vec16<R> a[kU * 2], b[kU * 2];
#pragma unroll
        for (int i = 0; i < kU * 2; ++i) {
            const long long g = tile + (long long)i * kThreads + t;
            if (g < g1) {
                a[i] = load16(u + off + g * GC);
                b[i] = load16(v + off + g * GC);
            } else {
                a[i] = b[i] = zero16<R>();
            }
        }
#pragma unroll
        for (int i = 0; i < kU * 2; ++i) {
            dot16<R, NC>(a[i], b[i], s);
            if (NRM) norm16(a[i], s[2]);
        }
    }
    block_sum<R, 3>(s, red);
    if (t == 0) {
#pragma unroll
        for (int k = 0; k < NC; ++k) part[((long long)c * G + wg) * NC + k] = s[k];
        if (NRM) nrm[(long long)c * G + wg] = s[2];
    }
}

template <typename R, int NC>
__global__ void __launch_bounds__(kThreads)
    half_kernel(long long ld, long long ng, int par, const R *__restrict__ psig, const R *__restrict__ phat, const R *__restrict__ v,
                R *__restrict__ x, R *__restrict__ r, R *__restrict__ pss, const CgState *__restrict__ st) {
    constexpr int GC = 16 / (int)sizeof(R);
    __shared__ R red[4][1];
    const int t = threadIdx.x, lane = t & 63, G = gridDim.x, wg = blockIdx.x, c = blockIdx.y;
    if (st->slot[par].status[c] != kCgRun) return;
    R rho[2], al[2];
    if (!bicg_alpha<R, NC>(psig, st->slot[par], c, G, lane, rho, al)) return;  // breakdown: bicg_dir freezes the column
    const R ar = al[0], ai = al[NC - 1];
    const long long off = (long long)c * ld * NC;
    R s[1] = {R(0)};  // ||s||^2
    long long g0, g1;
    wg_range(ng, G, wg, g0, g1);
    for (long long tile = g0; tile < g1; tile += (long long)kThreads * kU) {
        Vec16<R> xv[kU], pv[kU], rv[kU], vv[kU];
#pragma unroll
        for (int u = 0; u < kU; ++u) {
            const long long g = tile + (long long)u * kThreads + t;
            if (g < g1) {
                xv[u] = load16(x + off + g * GC);
                pv[u] = load16(phat + off + g * GC);
                rv[u] = load16(r + off + g * GC);
                vv[u] = load16(v + off + g * GC);
            }
        }
#pragma unroll
        for (int u = 0; u < kU; ++u) {
            const long long g = tile + (long long)u * kThreads + t;
            if (g >= g1) continue;
            axpy16<R, NC>(ar, ai, pv[u], xv[u]);
            axpy16<R, NC>(-ar, -ai, vv[u], rv[u]);
            norm16(rv[u], s[0]);
            store16(x + off + g * GC, xv[u]);
            store16(r + off + g * GC, rv[u]);
        }
    }
    block_sum<R, 1>(s, red);
    if (t == 0) pss[(long long)c * G + wg] = s[0];
}

// SHAT false: shat is r itself (no preconditioner) -- read once, and no pointer aliases the r that is written
template <typename R, int NC, bool SHAT>
__global__ void __launch_bounds__(kThreads)
    update_kernel(long long ld, long long ng, int par, const R *__restrict__ psig, const R *__restrict__ pss, const R *__restrict__ pts,
                  const R *__restrict__ ptt, const R *__restrict__ shat, const R *__restrict__ tv, const R *__restrict__ rhat,
                  R *__restrict__ x, R *__restrict__ r, R *__restrict__ pnn, R *__restrict__ prho, const CgState *__restrict__ st) {
    constexpr int GC = 16 / (int)sizeof(R);
    __shared__ R red[4][3];
    const int t = threadIdx.x, lane = t & 63, G = gridDim.x, wg = blockIdx.x, c = blockIdx.y;
    if (st->slot[par].status[c] != kCgRun) return;
    R rho[2], al[2], om[2], sn;
    if (!bicg_alpha<R, NC>(psig, st->slot[par], c, G, lane, rho, al)) return;
    if (bicg_omega<R, NC>(pss, pts, ptt, st->tol[c], c, G, lane, sn, om) != kCgRun) return;  // the iteration ended at the half step
    const R wr = om[0], wi = om[NC - 1];
    const long long off = (long long)c * ld * NC;
    R s[3] = {R(0), R(0), R(0)};  // <rhat, r> re, im; ||r||^2
    long long g0, g1;
    wg_range(ng, G, wg, g0, g1);
    for (long long tile = g0; tile < g1; tile += (long long)kThreads * kU) {
        Vec16<R> xv[kU], sv[kU], rv[kU], tw[kU], hv[kU];
#pragma unroll
        for (int u = 0; u < kU; ++u) {
            const long long g = tile + (long long)u * kThreads + t;
            if (g < g1) {
                xv[u] = load16(x + off + g * GC);
                if (SHAT) sv[u] = load16(shat + off + g * GC);
                rv[u] = load16(r + off + g * GC);
                tw[u] = load16(tv + off + g * GC);
                hv[u] = load16(rhat + off + g * GC);
            }
        }
#pragma unroll
        for (int u = 0; u < kU; ++u) {
            const long long g = tile + (long long)u * kThreads + t;
            if (g >= g1) continue;
            axpy16<R, NC>(wr, wi, SHAT ? sv[u] : rv[u], xv[u]);
            axpy16<R, NC>(-wr, -wi, tw[u], rv[u]);
            dot16<R, NC>(hv[u], rv[u], s);
            norm16(rv[u], s[2]);
            store16(x + off + g * GC, xv[u]);
            store16(r + off + g * GC, rv[u]);
        }
    }
    block_sum<R, 3>(s, red);
    if (t == 0) {
#pragma unroll
        for (int k = 0; k < NC; ++k) prho[((long long)c * G + wg) * NC + k] = s[k];
        pnn[(long long)c * G + wg] = s[2];
    }
}

template <typename R, int NC>
__global__ void __launch_bounds__(kThreads)
    dir_kernel(long long ld, long long ng, int first, int par, long long it, double rtol, double atol, const R *__restrict__ pbb,
               const R *__restrict__ psig, const R *__restrict__ pss, const R *__restrict__ pts, const R *__restrict__ ptt,
               const R *__restrict__ pnn, const R *__restrict__ prho, const R *__restrict__ r, const R *__restrict__ v, R *__restrict__ p,
               CgState *__restrict__ st) {
    constexpr int GC = 16 / (int)sizeof(R);
    const int t = threadIdx.x, lane = t & 63, G = gridDim.x, wg = blockIdx.x, c = blockIdx.y;
    const bool writer = wg == 0 && t == 0;
    const CgSlot &in = st->slot[par];
    CgSlot &out = st->slot[first ? 0 : par ^ 1];
    R rho[2] = {R(0), R(0)}, al[2] = {R(0), R(0)}, om[2] = {R(0), R(0)}, sn = R(0);
    int half = kCgRun;  // the status the half step ended the iteration with
    if (!first) {
        const int so = in.status[c];
        const bool broke = so == kCgRun && !bicg_alpha<R, NC>(psig, in, c, G, lane, rho, al);
        if (so != kCgRun || broke) {  // frozen before this iteration, or at its top: the state moves to the other slot
            if (writer) carry_frozen(in, out, st->rec, c, broke ? 3 : so);
            return;
        }
        half = bicg_omega<R, NC>(pss, pts, ptt, st->tol[c], c, G, lane, sn, om);
    }
    R rn = sn, rhn[2] = {R(0), R(0)};
    double tol = 0.0;
    R bn = R(0);
    int status = half;
    if (half == kCgRun) {
        const R nn = wave_total(pnn + (long long)c * G, G, 1, lane);
        rn = sqrt(nn);
        if (first) {
            rhn[0] = nn;  // <rhat, r> with rhat = r
            tol = first_tol(pbb + (long long)c * G, G, lane, rtol, atol, bn);
        } else {
            column_total<R, NC>(prho, c, G, lane, rhn);
            tol = st->tol[c];
        }
        status = decide(rn, tol);
    }
    if (writer) {
        // (a column that ended at the half step never reads rho again)
        out.rz[c][0] = (double)rhn[0];
        out.rz[c][1] = (double)rhn[1];
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
    // beta = (rho' / rho) (alpha / omega)   (rho != 0: checked at the top; omega != 0: ts != 0)
    R be[2] = {R(0), R(0)};
    if (!first) {
        R a[2] = {R(0), R(0)}, b[2] = {R(0), R(0)};
        k_div<R, NC>(rhn, rho, a);
        k_div<R, NC>(al, om, b);
        if (NC == 1) {
            be[0] = a[0] * b[0];
        } else {
            be[0] = a[0] * b[0] - a[NC - 1] * b[NC - 1];
            be[NC - 1] = a[0] * b[NC - 1] + a[NC - 1] * b[0];
        }
    }
    const R br = be[0], bi = be[NC - 1], wr = om[0], wi = om[NC - 1];
    const long long off = (long long)c * ld * NC;
    long long g0, g1;
    wg_range(ng, G, wg, g0, g1);
    for (long long tile = g0; tile < g1; tile += (long long)kThreads * kU) {
        Vec16<R> rv[kU], pv[kU], vv[kU];
#pragma unroll
        for (int u = 0; u < kU; ++u) {
            const long long g = tile + (long long)u * kThreads + t;
            if (g < g1) {
                rv[u] = load16(r + off + g * GC);
                if (!first) {
                    pv[u] = load16(p + off + g * GC);
                    vv[u] = load16(v + off + g * GC);
                }
            }
        }
#pragma unroll
        for (int u = 0; u < kU; ++u) {
            const long long g = tile + (long long)u * kThreads + t;
            if (g >= g1) continue;
            if (!first) {
                axpy16<R, NC>(-wr, -wi, vv[u], pv[u]);
                axpy16<R, NC>(br, bi, pv[u], rv[u]);
            }
            store16(p + off + g * GC, rv[u]);
        }
    }
}

}  // namespace

hipError_t launch_bicg_start(const CgDims &d, const void *B, long long ldb, const void *q, void *r, void *rhat, const BicgPartials &P,
                             hipStream_t stream) {
    return cg_dispatch(d, [&](auto rt, auto nc, long long ng, dim3 grid, auto) {
        using R = decltype(rt);
        constexpr int NC = decltype(nc)::value;
        hipLaunchKernelGGL((start_kernel<R, NC>), grid, dim3(kThreads), 0, stream, d.n, d.ld, ng, ldb, (const R *)B, (const R *)q, (R *)r,
                           (R *)rhat, (R *)P.bb, (R *)P.nn);
    });
}

hipError_t launch_bicg_dot(const CgDims &d, int par, const void *u, const void *v, void *part, void *nrm, const CgState *st,
                           hipStream_t stream) {
    return cg_dispatch(d, [&](auto rt, auto nc, long long ng, dim3 grid, auto) {
        using R = decltype(rt);
        constexpr int NC = decltype(nc)::value;
        auto launch = [&](auto kernel) {
            hipLaunchKernelGGL(kernel, grid, dim3(kThreads), 0, stream, d.ld, ng, par, (const R *)u, (const R *)v, (R *)part, (R *)nrm, st);
        };
        if (nrm)
            launch(dot_kernel<R, NC, true>);
        else
            launch(dot_kernel<R, NC, false>);
    });
}

hipError_t launch_bicg_half(const CgDims &d, int par, const BicgPartials &P, const void *phat, const void *v, void *x, void *r,
                            const CgState *st, hipStream_t stream) {
    return cg_dispatch(d, [&](auto rt, auto nc, long long ng, dim3 grid, auto) {
        using R = decltype(rt);
        constexpr int NC = decltype(nc)::value;
        hipLaunchKernelGGL((half_kernel<R, NC>), grid, dim3(kThreads), 0, stream, d.ld, ng, par, (const R *)P.sig, (const R *)phat,
                           (const R *)v, (R *)x, (R *)r, (R *)P.ss, st);
    });
}

hipError_t launch_bicg_update(const CgDims &d, int par, const BicgPartials &P, const void *shat, const void *t, const void *rhat,
                              void *x, void *r, const CgState *st, hipStream_t stream) {
    return cg_dispatch(d, [&](auto rt, auto nc, long long ng, dim3 grid, auto) {
        using R = decltype(rt);
        constexpr int NC = decltype(nc)::value;
        auto launch = [&](auto kernel) {
            hipLaunchKernelGGL(kernel, grid, dim3(kThreads), 0, stream, d.ld, ng, par, (const R *)P.sig, (const R *)P.ss, (const R *)P.ts,
                               (const R *)P.tt, (const R *)shat, (const R *)t, (const R *)rhat, (R *)x, (R *)r, (R *)P.nn, (R *)P.rho, st);
        };
        if (shat)
            launch(update_kernel<R, NC, true>);
        else
            launch(update_kernel<R, NC, false>);
    });
}

hipError_t launch_bicg_dir(const CgDims &d, bool first, int par, long long it, double rtol, double atol, const BicgPartials &P,
                           const void *r, const void *v, void *p, CgState *st, hipStream_t stream) {
    return cg_dispatch(d, [&](auto rt, auto nc, long long ng, dim3 grid, auto) {
        using R = decltype(rt);
        constexpr int NC = decltype(nc)::value;
        hipLaunchKernelGGL((dir_kernel<R, NC>), grid, dim3(kThreads), 0, stream, d.ld, ng, first ? 1 : 0, par, it, rtol, atol,
                           (const R *)P.bb, (const R *)P.sig, (const R *)P.ss, (const R *)P.ts, (const R *)P.tt, (const R *)P.nn,
                           (const R *)P.rho, (const R *)r, (const R *)v, (R *)p, st);
    });
}

}  // namespace bsm
