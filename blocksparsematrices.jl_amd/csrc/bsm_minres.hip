// bsm_minres.hip -- the kernels of bsm_minres_solve (include/bsm_rocm.h): symmetric-preconditioned MINRES on K right-hand
// sides in lockstep.  Kept out of the product kernel units like bsm_cg.hip: the build id (Makefile BUILD_ID) names the
// kernels and schedule of the PRODUCTS.
// (No counterpart in the reference: its operators are LinearMaps handed to a Julia solver package.)
//
// The conventions are those of bsm_cg.hip: 256-thread workgroups, the krylov_grid(n, es) row ranges walked in tiles of 256
// threads x kU 16-byte groups, one partial per workgroup and column, every consumer adding a column's G partials itself
// (the helpers: bsm_lockstep_device.h).  The launch is (krylov_grid, K); the decision is (1, K), one wave per column.
// Every scalar of the method is real, so the kernels but the start walk a column as reals, 16 bytes at a time.
//   start_kernel    r = v = B - q (B element by element under a guard), v_old = w = w_old = 0, the shares of ||b||^2, ||r||^2
//   dot_kernel      the shares of Re <u_c, v_c>: <z, q> and, with M, <v_new, z_new>
//   lanczos_kernel  delta from the shares of <z, q>;  v_new into the storage of v_old;  without M the shares of ||v_new||^2
//   update_kernel   gamma_new and the rotation from the shares and the `in` slot, by every workgroup for itself;  w_new into
//                   the storage of w_old, x, r in one pass;  the shares of ||r||^2;  workgroup 0 leaves the step
//   decide_kernel   ||r|| against tol_c (first launch of a solve: tol_c from the shares of ||b||^2);  writes the OTHER parity
//                   slot of the state and the record the host reads;  carries frozen columns over
// A frozen column's workgroups return before their first vector load.  Every sum has a fixed order: results are
// bit-identical from run to run where the products are.  Device values are written with ordinary vector stores only.
#include "bsm_minres.h"

#include "../../include/bsm_rocm.h"
#include "bsm_lockstep_device.h"

namespace bsm {
namespace {

template <typename R, int NC>
__global__ void __launch_bounds__(kThreads)
    start_kernel(long long n, long long ng, long long ldb, const R *__restrict__ B, const R *__restrict__ q, R *__restrict__ r,
                 R *__restrict__ v, R *__restrict__ vold, R *__restrict__ w0, R *__restrict__ w1, R *__restrict__ pbb, R *__restrict__ pnn) {
    constexpr int GC = 16 / (int)sizeof(R);
    __shared__ R red[4][2];
    const int t = threadIdx.x, G = gridDim.x, wg = blockIdx.x, c = blockIdx.y;
    const R *Bc = B + (long long)c * ldb * NC;
    const long long off = (long long)c * ng * GC;
    R s[2] = {R(0), R(0)};  // ||b||^2, ||r||^2
    long long g0, g1;
    wg_range(ng, G, wg, g0, g1);
    for (long long tile = g0; tile < g1; tile += (long long)kThreads * kU) {
#pragma unroll
        for (int u = 0; u < kU; ++u) {
            const long long g = tile + (long long)u * kThreads + t;
            if (g >= g1) continue;
            Vec16<R> b = load16_guarded<R, NC>(Bc, g, n);
            norm16(b, s[0]);
            if (q) sub16(b, load16(q + off + g * GC));
            norm16(b, s[1]);
            store16(r + off + g * GC, b);
            store16(v + off + g * GC, b);
            const Vec16<R> z = zero16<R>();
            store16(vold + off + g * GC, z);
            store16(w0 + off + g * GC, z);
            store16(w1 + off + g * GC, z);
        }
    }
    block_sum<R, 2>(s, red);
    if (t == 0) {
        pbb[(long long)c * G + wg] = s[0];
        pnn[(long long)c * G + wg] = s[1];
    }
}

template <typename R>
__global__ void __launch_bounds__(kThreads) dot_kernel(long long ng, int par, const R *__restrict__ u, const R *__restrict__ v,
                                                       R *__restrict__ part, const MrState *__restrict__ st) {
    constexpr int GC = 16 / (int)sizeof(R);
    __shared__ R red[4][1];
    const int t = threadIdx.x, G = gridDim.x, wg = blockIdx.x, c = blockIdx.y;
    if (par >= 0 && st->slot[par].status[c] != kCgRun) return;
    const long long off = (long long)c * ng * GC;
    R s[1] = {R(0)};
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
        for (int i = 0; i < kU * 2; ++i) dot16<R, 1>(a[i], b[i], s);  // Re conj(u) v: the group as reals (NC = 1), whatever the element type
    }
    block_sum<R, 1>(s, red);
    if (t == 0) part[(long long)c * G + wg] = s[0];
}

template <typename R, bool NORM>
__global__ void __launch_bounds__(kThreads)
    lanczos_kernel(long long ng, int par, const R *__restrict__ pzq, const R *__restrict__ q, const R *__restrict__ v, R *__restrict__ vold,
                   R *__restrict__ pvz, const MrState *__restrict__ st) {
    constexpr int GC = 16 / (int)sizeof(R);
    __shared__ R red[4][1];
    const int t = threadIdx.x, lane = t & 63, G = gridDim.x, wg = blockIdx.x, c = blockIdx.y;
    const MrSlot &in = st->slot[par];
    if (in.status[c] != kCgRun) return;
    // (gamma > 0 and finite on a running column: mr_decide froze every other one)
    const R zq = wave_total(pzq + (long long)c * G, G, 1, lane);
    const R gam = (R)in.gamma[c], ig = R(1) / gam;
    const R delta = zq / (gam * gam);
    const R cv = delta * ig, co = gam / (R)in.gamma_old[c];
    const long long off = (long long)c * ng * GC;
    R s[1] = {R(0)};
    long long g0, g1;
    wg_range(ng, G, wg, g0, g1);
    for (long long tile = g0; tile < g1; tile += (long long)kThreads * kU) {
        Vec16<R> qv[kU], vv[kU], ov[kU];
#pragma unroll
        for (int u = 0; u < kU; ++u) {
            const long long g = tile + (long long)u * kThreads + t;
            if (g < g1) {
                qv[u] = load16(q + off + g * GC);
                vv[u] = load16(v + off + g * GC);
                ov[u] = load16(vold + off + g * GC);
            }
        }
#pragma unroll
        for (int u = 0; u < kU; ++u) {
            const long long g = tile + (long long)u * kThreads + t;
            if (g >= g1) continue;
#pragma unroll
            for (int k = 0; k < GC; ++k) ov[u].r[k] = (ig * qv[u].r[k] - cv * vv[u].r[k]) - co * ov[u].r[k];
            if (NORM) norm16(ov[u], s[0]);
            store16(vold + off + g * GC, ov[u]);
        }
    }
    if (NORM) {
        block_sum<R, 1>(s, red);
        if (t == 0) pvz[(long long)c * G + wg] = s[0];
    }
}

template <typename R>
__global__ void __launch_bounds__(kThreads)
    update_kernel(long long ng, int par, const R *__restrict__ pzq, const R *__restrict__ pvz, const R *__restrict__ z, R *__restrict__ wold,
                  const R *__restrict__ w, R *__restrict__ x, R *__restrict__ r, const R *__restrict__ vnew, R *__restrict__ pnn,
                  MrState *__restrict__ st) {
    constexpr int GC = 16 / (int)sizeof(R);
    __shared__ R red[4][1];
    const int t = threadIdx.x, lane = t & 63, G = gridDim.x, wg = blockIdx.x, c = blockIdx.y;
    const MrSlot &in = st->slot[par];
    if (in.status[c] != kCgRun) return;
    const bool writer = wg == 0 && t == 0;
    const R zq = wave_total(pzq + (long long)c * G, G, 1, lane);
    const R vz = wave_total(pvz + (long long)c * G, G, 1, lane);
    const R gam = (R)in.gamma[c], eta = (R)in.eta[c], cs = (R)in.c[c], co = (R)in.c_old[c], sn = (R)in.s[c], so = (R)in.s_old[c];
    // breakdown: mr_decide freezes the column; no root of a negative number, no division by zero is executed
    bool brk = !(vz >= R(0)) || !isfinite(vz);
    R gn = R(0), a1 = R(0), a0 = R(0);
    const R delta = zq / (gam * gam);
    if (!brk) {
        gn = sqrt(vz);
        a0 = cs * delta - co * sn * gam;
        a1 = sqrt(a0 * a0 + gn * gn);
        brk = !(a1 > R(0)) || !isfinite(a1);
    }
    if (brk) {
        if (writer) st->step.brk[c] = 1;
        return;
    }
    const R a2 = sn * delta + co * cs * gam, a3 = so * gam;
    const R ia = R(1) / a1, ig = R(1) / gam;
    const R cn = a0 * ia, s1 = gn * ia;
    const R en = -s1 * eta;
    const R cx = cn * eta, ss = s1 * s1, cr = gn == R(0) ? R(0) : cn * en / gn;
    if (writer) {
        st->step.gamma[c] = (double)gn;
        st->step.eta[c] = (double)en;
        st->step.c[c] = (double)cn;
        st->step.s[c] = (double)s1;
        st->step.brk[c] = 0;
    }
    const long long off = (long long)c * ng * GC;
    R s[1] = {R(0)};
    long long g0, g1;
    wg_range(ng, G, wg, g0, g1);
    for (long long tile = g0; tile < g1; tile += (long long)kThreads * kU) {
        Vec16<R> zv[kU], ov[kU], wv[kU], xv[kU], rv[kU], nv[kU];
#pragma unroll
        for (int u = 0; u < kU; ++u) {
            const long long g = tile + (long long)u * kThreads + t;
            if (g < g1) {
                zv[u] = load16(z + off + g * GC);
                ov[u] = load16(wold + off + g * GC);
                wv[u] = load16(w + off + g * GC);
                xv[u] = load16(x + off + g * GC);
                rv[u] = load16(r + off + g * GC);
                nv[u] = load16(vnew + off + g * GC);
            }
        }
#pragma unroll
        for (int u = 0; u < kU; ++u) {
            const long long g = tile + (long long)u * kThreads + t;
            if (g >= g1) continue;
#pragma unroll
            for (int k = 0; k < GC; ++k) {
                const R wn = ((ig * zv[u].r[k] - a3 * ov[u].r[k]) - a2 * wv[u].r[k]) * ia;
                ov[u].r[k] = wn;
                xv[u].r[k] += cx * wn;
                rv[u].r[k] = ss * rv[u].r[k] + cr * nv[u].r[k];
            }
            norm16(rv[u], s[0]);
            store16(wold + off + g * GC, ov[u]);
            store16(x + off + g * GC, xv[u]);
            store16(r + off + g * GC, rv[u]);
        }
    }
    block_sum<R, 1>(s, red);
    if (t == 0) pnn[(long long)c * G + wg] = s[0];
}

// a column that does not iterate any more moves to the other slot with `status` (carry_frozen on the slots of this unit)
__device__ __forceinline__ void mr_carry(const MrSlot &in, MrSlot &out, CgRecord &rec, int c, int status) {
    out.gamma[c] = in.gamma[c], out.gamma_old[c] = in.gamma_old[c], out.eta[c] = in.eta[c];
    out.c[c] = in.c[c], out.c_old[c] = in.c_old[c], out.s[c] = in.s[c], out.s_old[c] = in.s_old[c];
    out.rn[c] = in.rn[c];
    out.status[c] = status;
    out.done[c] = in.done[c];
    rec.status[c] = status;
}

template <typename R>
__global__ void __launch_bounds__(64) decide_kernel(int G, int first, int par, long long it, double rtol, double atol, const R *__restrict__ pbb,
                                                    const R *__restrict__ pnn, const R *__restrict__ pvz, MrState *__restrict__ st) {
    const int lane = threadIdx.x, c = blockIdx.y;
    const bool writer = lane == 0;
    const MrSlot &in = st->slot[par];
    MrSlot &out = st->slot[first ? 0 : par ^ 1];
    if (!first) {
        const int so = in.status[c];
        const bool broke = so == kCgRun && st->step.brk[c] != 0;
        if (so != kCgRun || broke) {  // frozen before this iteration, or by its mr_update: the state moves to the other slot
            if (writer) mr_carry(in, out, st->rec, c, broke ? 3 : so);
            return;
        }
    }
    const R rn = sqrt(wave_total(pnn + (long long)c * G, G, 1, lane));
    R bn = R(0);
    const double tol = first ? first_tol(pbb + (long long)c * G, G, lane, rtol, atol, bn) : st->tol[c];
    int status = decide(rn, tol);
    double gam, gold, eta, cs, co, sn, so;
    if (first) {
        const R vz = wave_total(pvz + (long long)c * G, G, 1, lane);
        const bool pd = vz > R(0) && isfinite(vz);
        if (status == kCgRun && !pd) status = 3;  // <v, z> <= 0 on a residual above the tolerance: M is not positive definite
        gam = eta = pd ? (double)sqrt(vz) : 0.0;
        gold = 1, cs = co = 1, sn = so = 0;
    } else {
        gam = st->step.gamma[c], gold = in.gamma[c], eta = st->step.eta[c];
        cs = st->step.c[c], co = in.c[c], sn = st->step.s[c], so = in.s[c];
        if (status == kCgRun && gam == 0) status = 3;  // the Krylov space ended above the tolerance
    }
    if (!writer) return;
    out.gamma[c] = gam, out.gamma_old[c] = gold, out.eta[c] = eta;
    out.c[c] = cs, out.c_old[c] = co, out.s[c] = sn, out.s_old[c] = so;
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

}  // namespace

hipError_t launch_mr_start(const CgDims &d, const void *B, long long ldb, const void *q, void *r, void *v, void *vold, void *w0, void *w1,
                           void *pbb, void *pnn, hipStream_t stream) {
    return cg_dispatch(d, [&](auto rt, auto nc, long long ng, dim3 grid, auto) {
        using R = decltype(rt);
        constexpr int NC = decltype(nc)::value;
        hipLaunchKernelGGL((start_kernel<R, NC>), grid, dim3(kThreads), 0, stream, d.n, ng, ldb, (const R *)B, (const R *)q, (R *)r, (R *)v,
                           (R *)vold, (R *)w0, (R *)w1, (R *)pbb, (R *)pnn);
    });
}

hipError_t launch_mr_dot(const CgDims &d, int par, const void *u, const void *v, void *part, const MrState *st, hipStream_t stream) {
    return cg_dispatch(d, [&](auto rt, auto, long long ng, dim3 grid, auto) {
        using R = decltype(rt);
        hipLaunchKernelGGL((dot_kernel<R>), grid, dim3(kThreads), 0, stream, ng, par, (const R *)u, (const R *)v, (R *)part, st);
    });
}

hipError_t launch_mr_lanczos(const CgDims &d, int par, const void *pzq, const void *q, const void *v, void *vold, void *pvz,
                             const MrState *st, hipStream_t stream) {
    return cg_dispatch(d, [&](auto rt, auto, long long ng, dim3 grid, auto) {
        using R = decltype(rt);
        auto launch = [&](auto kernel) {
            hipLaunchKernelGGL(kernel, grid, dim3(kThreads), 0, stream, ng, par, (const R *)pzq, (const R *)q, (const R *)v, (R *)vold,
                               (R *)pvz, st);
        };
        if (pvz)
            launch(lanczos_kernel<R, true>);
        else
            launch(lanczos_kernel<R, false>);
    });
}

hipError_t launch_mr_update(const CgDims &d, int par, const void *pzq, const void *pvz, const void *z, void *wold, const void *w, void *x,
                            void *r, const void *vnew, void *pnn, MrState *st, hipStream_t stream) {
    return cg_dispatch(d, [&](auto rt, auto, long long ng, dim3 grid, auto) {
        using R = decltype(rt);
        hipLaunchKernelGGL((update_kernel<R>), grid, dim3(kThreads), 0, stream, ng, par, (const R *)pzq, (const R *)pvz, (const R *)z,
                           (R *)wold, (const R *)w, (R *)x, (R *)r, (const R *)vnew, (R *)pnn, st);
    });
}

hipError_t launch_mr_decide(const CgDims &d, bool first, int par, long long it, double rtol, double atol, const void *pbb, const void *pnn,
                            const void *pvz, MrState *st, hipStream_t stream) {
    return cg_dispatch(d, [&](auto rt, auto, long long, dim3 grid, auto) {
        using R = decltype(rt);
        hipLaunchKernelGGL((decide_kernel<R>), dim3(1, grid.y), dim3(64), 0, stream, (int)grid.x, first ? 1 : 0, par, it, rtol, atol,
                           (const R *)pbb, (const R *)pnn, (const R *)pvz, st);
    });
}

}  // namespace bsm
