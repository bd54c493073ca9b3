// bsm_gmres_multi.hip -- the kernels of bsm_gmres_multi_solve and bsm_gmres_solve (include/bsm_rocm.h): right-preconditioned
// restarted GMRES on K right-hand sides in lockstep (bsm_gmres_solve: K = 1).  Kept out of the product kernel units like
// bsm_cg.hip: the build id (Makefile BUILD_ID) names the kernels and schedule of the PRODUCTS.
// (No counterpart in the reference: its operators are LinearMaps handed to a Julia solver package.)
//
// The conventions are those of bsm_cg.hip / bsm_bicgstab.hip, whose helpers this unit shares through bsm_lockstep_device.h;
// what it shares with the Gram-Schmidt pass of bsm_krylov.hip (bsm_krylov_orth) is bsm_krylov_device.h (the dot and the update
// of a group, the sum of the partials); the rotations and the division are the plain C++ of bsm_krylov.h:
// 256-thread workgroups, the launch (krylov_grid, K), tiles of 256 threads x kU 16-byte groups, one partial per workgroup,
// basis vector and column, unguarded 16-byte accesses on workspace vectors that carry zero padding (bsm_cg.h).  The
// arithmetic of a pass is that of bsm_krylov.hip with the right-hand side on blockIdx.y:
//   start_kernel    r = B - q (B element by element under a guard: any ldb, any alignment) -> V_0, the shares of ||r||^2
//                   and on the first start of ||b||^2.
//   begin_kernel    beta from the shares, summed by every workgroup for itself; V_0 *= 1 / beta; workgroup 0 of the column
//                   writes g = beta e_1, hsum = 0, tol_c on the first start, the decision and the record.
//   dot_kernel      a tile of W[:, c] stays in registers while V_0[:, c] .. V_{k-1}[:, c] stream past it, kCB of them in
//                   flight; per basis vector the lane's products, 6 xor-shuffles, the wave's sum to its LDS slot; one
//                   partial per workgroup, basis vector and column.
//   update_kernel   every workgroup sums the G partials of every basis vector in the same fixed order, keeps h in LDS,
//                   W -= V h, the shares of ||w||^2; workgroup 0 adds h to hsum.
//   hess_kernel     one wave per column: krylov_hess_column (bsm_krylov.h) on (hsum, ||w||), then the decision --
//                   estimate <= tol: 0, not finite: 2 --, the counts, 1 / ||w|| and the record.
//                   Beside begin_kernel the only writer of a column's state.
//   scale_kernel    V_{j+1} = W * (1 / ||w||).
//   trsolve_kernel  one wave per column, k = k_c from the state;  combine_kernel  U = V[:, 0 : k_c] y (zeros on a column
//                   that owes nothing);  axpy_kernel  X += Z on the columns that owe an update.
// A column that has a status is frozen: the workgroups of every vector kernel return before their first vector load, the
// one-wave kernels carry its state over unchanged.  begin and hess read slot `par` of the state and write slot par ^ 1, so
// no launch reads a scalar that the same launch replaces.  No workgroup waits for another, there is no floating-point
// atomic, and every sum has a fixed order.  Device values are written with ordinary vector stores only.
#include "bsm_gmres_multi.h"

#include "../../include/bsm_rocm.h"
#include "bsm_lockstep_device.h"

namespace bsm {
namespace {

constexpr int kCB = 4;  // basis vectors in flight

template <typename R, int NC>
__global__ void __launch_bounds__(kThreads)
    start_kernel(long long n, long long ld, long long ng, long long ldb, int first, int par, const R *__restrict__ B,
                 const R *__restrict__ q, R *__restrict__ v0, R *__restrict__ pbb, long long pbs, R *__restrict__ pnn,
                 const GmState *__restrict__ st) {
    constexpr int GC = 16 / (int)sizeof(R);
    __shared__ R red[4][2];
    const int t = threadIdx.x, G = gridDim.x, wg = blockIdx.x, c = blockIdx.y;
    if (!first && st->slot[par].status[c] != kCgRun) return;
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
            store16(v0 + off + g * GC, v);
        }
    }
    block_sum<R, 2>(s, red);
    if (t == 0) {
        if (first) pbb[(long long)c * pbs + wg] = s[0];
        pnn[(long long)c * G + wg] = s[1];
    }
}

template <typename R, int NC>
__global__ void __launch_bounds__(kThreads)
    begin_kernel(long long ld, long long ng, int first, int par, int m, double rtol, double atol, const R *__restrict__ pbb, long long pbs,
                 const R *__restrict__ pnn, R *__restrict__ v0, R *__restrict__ gv, R *__restrict__ hsum, GmState *__restrict__ st) {
    constexpr int GC = 16 / (int)sizeof(R);
    const int t = threadIdx.x, lane = t & 63, G = gridDim.x, wg = blockIdx.x, c = blockIdx.y;
    const bool writer = wg == 0 && t == 0;
    const GmSlot &in = st->slot[par];
    GmSlot &out = st->slot[first ? 0 : par ^ 1];
    if (!first && in.status[c] != kCgRun) {  // frozen: the state moves to the other slot, nothing is owed any more
        if (writer) {
            out.rn[c] = in.rn[c];
            out.status[c] = in.status[c];
            out.done[c] = in.done[c];
            out.kc[c] = 0;
            out.owed[c] = 0;
            st->rec.rn[c] = in.rn[c];
            st->rec.status[c] = in.status[c];
            st->rec.done[c] = in.done[c];
        }
        return;
    }
    const R beta = sqrt(wave_total(pnn + (long long)c * G, G, 1, lane));
    R bn = R(0);
    const double tol = first ? first_tol(pbb + (long long)c * pbs, G, lane, rtol, atol, bn) : st->tol[c];
    const int status = decide(beta, tol);
    if (wg == 0) {
        R *gc = gv + (long long)c * (m + 1) * NC, *hc = hsum + (long long)c * m * NC;
        for (int i = t; i < (m + 1) * NC; i += kThreads) gc[i] = i == 0 ? beta : R(0);
        for (int i = t; i < m * NC; i += kThreads) hc[i] = R(0);
    }
    if (writer) {
        const int done = first ? 0 : in.done[c];
        out.rn[c] = (double)beta;
        out.status[c] = status;
        out.done[c] = done;
        out.kc[c] = 0;
        out.owed[c] = 0;
        if (first) {
            st->tol[c] = tol;
            st->bnorm[c] = (double)bn;
            st->rec.bnorm[c] = (double)bn;
        }
        st->rec.rn[c] = (double)beta;
        st->rec.status[c] = status;
        st->rec.done[c] = done;
    }
    if (status != kCgRun) return;
    const R inv = R(1) / beta;  // (beta > tol >= 0)
    const long long off = (long long)c * ld * NC;
    long long g0, g1;
    wg_range(ng, G, wg, g0, g1);
    for (long long g = g0 + t; g < g1; g += kThreads) {
        Vec16<R> v = load16(v0 + off + g * GC);
        scale16(v, inv);
        store16(v0 + off + g * GC, v);
    }
}

template <typename R, int NC>
__global__ void __launch_bounds__(kThreads)
    dot_kernel(long long ld, long long ng, long long vs, int k, int m, int par, const R *__restrict__ V, const R *__restrict__ W,
               R *__restrict__ part, const GmState *__restrict__ st) {
    constexpr int GC = 16 / (int)sizeof(R);
    __shared__ R acc[BSM_GMRES_MAX_RESTART * 4 * NC];
    const int t = threadIdx.x, lane = t & 63, wave = t >> 6, G = gridDim.x, wg = blockIdx.x, c = blockIdx.y;
    if (st->slot[par].status[c] != kCgRun) return;
    for (int i = t; i < k * 4 * NC; i += kThreads) acc[i] = R(0);
    __syncthreads();
    const long long off = (long long)c * ld * NC;
    long long g0, g1;
    wg_range(ng, G, wg, g0, g1);
    for (long long tile = g0; tile < g1; tile += (long long)kThreads * kU) {
        Vec16<R> wv[kU];
        long long go[kU];
        bool ok[kU];
#pragma unroll
        for (int u = 0; u < kU; ++u) {
            const long long g = tile + (long long)u * kThreads + t;
            ok[u] = g < g1;
            go[u] = off + g * GC;
            wv[u] = ok[u] ? load16(W + go[u]) : zero16<R>();
        }
        for (int c0 = 0; c0 < k; c0 += kCB) {
            Vec16<R> vv[kCB][kU];
#pragma unroll
            for (int cc = 0; cc < kCB; ++cc)
#pragma unroll
                for (int u = 0; u < kU; ++u)
                    vv[cc][u] = ok[u] && c0 + cc < k ? load16(V + (long long)(c0 + cc) * vs * NC + go[u]) : zero16<R>();
            R s[kCB][NC];
#pragma unroll
            for (int cc = 0; cc < kCB; ++cc) {
#pragma unroll
                for (int q = 0; q < NC; ++q) s[cc][q] = R(0);
#pragma unroll
                for (int u = 0; u < kU; ++u) dot16<R, NC>(vv[cc][u], wv[u], s[cc]);
            }
#pragma unroll
            for (int cc = 0; cc < kCB; ++cc)
#pragma unroll
                for (int q = 0; q < NC; ++q) s[cc][q] = wave_sum(s[cc][q]);
            if (lane == 0) {
#pragma unroll
                for (int cc = 0; cc < kCB; ++cc)
                    if (c0 + cc < k) {
#pragma unroll
                        for (int q = 0; q < NC; ++q) acc[((c0 + cc) * 4 + wave) * NC + q] += s[cc][q];
                    }
            }
        }
    }
    __syncthreads();
    R *pc = part + (long long)c * m * G * NC;
    for (int i = t; i < k * NC; i += kThreads) {
        const int b = i / NC, q = i % NC;
        const R a = (acc[(b * 4 + 0) * NC + q] + acc[(b * 4 + 1) * NC + q]) + (acc[(b * 4 + 2) * NC + q] + acc[(b * 4 + 3) * NC + q]);
        pc[((long long)b * G + wg) * NC + q] = a;
    }
}

// out[:, c] (+)= V[:, 0 : k] h with h in LDS; UPDATE: W -= V h from the partials, with the norm;  else U = V y
template <typename R, int NC, bool UPDATE>
__global__ void __launch_bounds__(kThreads)
    sweep_kernel(long long ld, long long ng, long long vs, int kk, int m, int par, const R *__restrict__ V, R *__restrict__ W,
                 const R *__restrict__ part, const R *__restrict__ y, R *__restrict__ hsum, R *__restrict__ nrm,
                 const GmState *__restrict__ st) {
    constexpr int GC = 16 / (int)sizeof(R), VE = GC / NC;
    __shared__ R hs[BSM_GMRES_MAX_RESTART * NC];
    __shared__ R red[4][1];
    const int t = threadIdx.x, G = gridDim.x, wg = blockIdx.x, c = blockIdx.y;
    const GmSlot &sl = st->slot[par];
    const long long off = (long long)c * ld * NC;
    long long g0, g1;
    wg_range(ng, G, wg, g0, g1);
    int k = kk;
    if (UPDATE) {
        if (sl.status[c] != kCgRun) return;
        int b;
        R a[NC];
        if (gs_sum_partials<R, NC>(part + (long long)c * m * G * NC, k, G, t, kThreads, b, a)) {
#pragma unroll
            for (int q = 0; q < NC; ++q) {
                hs[b * NC + q] = -a[q];
                if (wg == 0) hsum[((long long)c * m + b) * NC + q] += a[q];
            }
        }
    } else {
        k = sl.owed[c] ? sl.kc[c] : 0;
        if (k == 0) {  // nothing owed: zeros, so that the product opM(M) U reads numbers
            for (long long g = g0 + t; g < g1; g += kThreads) store16(W + off + g * GC, zero16<R>());
            return;
        }
        for (int i = t; i < k * NC; i += kThreads) hs[i] = y[(long long)c * m * NC + i];
    }
    __syncthreads();
    R nn[1] = {R(0)};
    for (long long tile = g0; tile < g1; tile += (long long)kThreads * kU) {
        Vec16<R> wv[kU];
        long long go[kU];
        bool ok[kU];
#pragma unroll
        for (int u = 0; u < kU; ++u) {
            const long long g = tile + (long long)u * kThreads + t;
            ok[u] = g < g1;
            go[u] = off + g * GC;
            wv[u] = UPDATE && ok[u] ? load16(W + go[u]) : zero16<R>();
        }
        for (int c0 = 0; c0 < k; c0 += kCB) {
            Vec16<R> vv[kCB][kU];
#pragma unroll
            for (int cc = 0; cc < kCB; ++cc)
#pragma unroll
                for (int u = 0; u < kU; ++u)
                    vv[cc][u] = ok[u] && c0 + cc < k ? load16(V + (long long)(c0 + cc) * vs * NC + go[u]) : zero16<R>();
#pragma unroll
            for (int cc = 0; cc < kCB; ++cc) {
                if (c0 + cc < k) {
                    const R hr = hs[(c0 + cc) * NC], hi = hs[(c0 + cc) * NC + NC - 1];
#pragma unroll
                    for (int u = 0; u < kU; ++u) gs_axpy<R, NC, VE>(vv[cc][u].r, hr, hi, wv[u].r);
                }
            }
        }
#pragma unroll
        for (int u = 0; u < kU; ++u) {
            if (!ok[u]) continue;
            if (UPDATE) norm16(wv[u], nn[0]);
            store16(W + go[u], wv[u]);
        }
    }
    if (UPDATE) {
        block_sum<R, 1>(nn, red);
        if (t == 0) nrm[(long long)c * G + wg] = nn[0];
    }
}

template <typename R, int NC>
__global__ void __launch_bounds__(64) hess_kernel(int G, int m, int j, int par, const R *__restrict__ nrm, R *__restrict__ hsum_,
                                                  R *__restrict__ Hm_, R *__restrict__ cs_, R *__restrict__ sn_, R *__restrict__ g_,
                                                  R *__restrict__ inv, GmState *__restrict__ st) {
    __shared__ R col[(BSM_GMRES_MAX_RESTART + 1) * NC];
    __shared__ R rot[BSM_GMRES_MAX_RESTART * 3];  // cs, sn of the stored rotations
    __shared__ R gg[2 * NC];
    const int lane = threadIdx.x, c = blockIdx.x;
    const GmSlot &in = st->slot[par];
    GmSlot &out = st->slot[par ^ 1];
    if (in.status[c] != kCgRun) {  // frozen: the state moves to the other slot, the record repeats it
        if (lane == 0) {
            out.rn[c] = in.rn[c];
            out.status[c] = in.status[c];
            out.done[c] = in.done[c];
            out.kc[c] = in.kc[c];
            out.owed[c] = in.owed[c];
            st->rec.rn[c] = in.rn[c];
            st->rec.status[c] = in.status[c];
            st->rec.done[c] = in.done[c];
        }
        return;
    }
    R *hsum = hsum_ + (long long)c * m * NC, *Hm = Hm_ + (long long)c * m * (m + 1) * NC, *cs = cs_ + (long long)c * m;
    R *sn = sn_ + (long long)c * m * NC, *g = g_ + (long long)c * (m + 1) * NC;
    const R hn = sqrt(wave_total(nrm + (long long)c * G, G, 1, lane));
    // the column hsum[0 .. j] (zeroed behind it), the stored rotations and g[j] into LDS
    for (int i = lane; i < (j + 1) * NC; i += 64) {
        col[i] = hsum[i];
        hsum[i] = R(0);
    }
    for (int i = lane; i < j; i += 64) rot[i] = cs[i];
    for (int i = lane; i < j * NC; i += 64) rot[BSM_GMRES_MAX_RESTART + i] = sn[i];
    if (lane < NC) gg[lane] = g[j * NC + lane];
    __syncthreads();
    if (lane == 0) {
        const R est = krylov_hess_column<R, NC>(j, col, hn, rot, rot + BSM_GMRES_MAX_RESTART, gg - (long long)j * NC);
        cs[j] = rot[j];
        for (int q = 0; q < NC; ++q) {
            sn[j * NC + q] = rot[BSM_GMRES_MAX_RESTART + j * NC + q];
            g[j * NC + q] = gg[q];
            g[(j + 1) * NC + q] = gg[NC + q];
        }
        inv[c] = hn == R(0) ? R(0) : R(1) / hn;
        // the decision: the answer of this column uses exactly the iterations up to this one
        const int status = !isfinite(hn) ? 2 : decide(est, st->tol[c]);
        const int done = in.done[c] + 1;
        out.rn[c] = (double)est;
        out.status[c] = status;
        out.done[c] = done;
        out.kc[c] = j + 1;
        out.owed[c] = status == 2 ? 0 : 1;  // (status 2: x keeps its last finished cycle)
        st->rec.rn[c] = (double)est;
        st->rec.status[c] = status;
        st->rec.done[c] = done;
    }
    // column j of the rotated Hessenberg matrix (leading dimension m + 1)
    __syncthreads();
    R *const dst = Hm + (long long)j * (m + 1) * NC;
    for (int i = lane; i < (j + 1) * NC; i += 64) dst[i] = col[i];
}

template <typename R, int NC>
__global__ void __launch_bounds__(kThreads) scale_kernel(long long ld, long long ng, int par, const R *__restrict__ W, R *__restrict__ Vn,
                                                         const R *__restrict__ inv, const GmState *__restrict__ st) {
    constexpr int GC = 16 / (int)sizeof(R);
    const int t = threadIdx.x, G = gridDim.x, wg = blockIdx.x, c = blockIdx.y;
    if (st->slot[par].status[c] != kCgRun) return;
    const R sc = inv[c];
    const long long off = (long long)c * ld * NC;
    long long g0, g1;
    wg_range(ng, G, wg, g0, g1);
    for (long long g = g0 + t; g < g1; g += kThreads) {
        Vec16<R> v = load16(W + off + g * GC);
        scale16(v, sc);
        store16(Vn + off + g * GC, v);
    }
}

// y[0 .. k) = R^-1 g[0 .. k) by one wave on the rotated Hessenberg matrix Hm (leading dimension m + 1): lane 0 divides, the
// column update of every step is spread over the lanes.  ys (BSM_GMRES_MAX_RESTART * NC) and q (2) are LDS.
template <typename R, int NC>
__device__ __forceinline__ void trsolve_wave(int m, int k, const R *__restrict__ Hm, const R *__restrict__ g, R *__restrict__ y, R *ys, R *q,
                                             int lane) {
    const long long ldh = m + 1;
    for (int i = lane; i < k * NC; i += 64) ys[i] = g[i];
    __syncthreads();
    for (int i = k - 1; i >= 0; --i) {
        if (lane == 0) {
            R d[2] = {R(0), R(0)};
            k_div<R, NC>(ys + i * NC, Hm + ((long long)i + i * ldh) * NC, d);
            for (int c = 0; c < NC; ++c) q[c] = ys[i * NC + c] = d[c];
        }
        __syncthreads();
        const R qr = q[0], qi = q[NC - 1];
        for (int r = lane; r < i; r += 64) {
            const R *a = Hm + ((long long)r + i * ldh) * NC;
            if (NC == 1) {
                ys[r] -= a[0] * qr;
            } else {
                ys[r * NC] -= a[0] * qr - a[NC - 1] * qi;
                ys[r * NC + NC - 1] -= a[0] * qi + a[NC - 1] * qr;
            }
        }
        __syncthreads();
    }
    for (int i = lane; i < k * NC; i += 64) y[i] = ys[i];
}

template <typename R, int NC>
__global__ void __launch_bounds__(64) trsolve_kernel(int m, int par, const R *__restrict__ Hm_, const R *__restrict__ g_, R *__restrict__ y_,
                                                     const GmState *__restrict__ st) {
    __shared__ R ys[BSM_GMRES_MAX_RESTART * NC];
    __shared__ R q[2];
    const int lane = threadIdx.x, c = blockIdx.x;
    const GmSlot &sl = st->slot[par];
    const int k = sl.owed[c] ? sl.kc[c] : 0;
    if (k == 0) return;
    trsolve_wave<R, NC>(m, k, Hm_ + (long long)c * m * (m + 1) * NC, g_ + (long long)c * (m + 1) * NC, y_ + (long long)c * m * NC, ys, q,
                        lane);
}

template <typename R, int NC>
__global__ void __launch_bounds__(kThreads) axpy_kernel(long long ld, long long ng, int par, const R *__restrict__ Z, R *__restrict__ X,
                                                        const GmState *__restrict__ st) {
    constexpr int GC = 16 / (int)sizeof(R);
    const int t = threadIdx.x, G = gridDim.x, wg = blockIdx.x, c = blockIdx.y;
    const GmSlot &sl = st->slot[par];
    if (!sl.owed[c] || sl.kc[c] == 0) return;
    const long long off = (long long)c * ld * NC;
    long long g0, g1;
    wg_range(ng, G, wg, g0, g1);
    for (long long g = g0 + t; g < g1; g += kThreads) {
        Vec16<R> x = load16(X + off + g * GC);
        add16(x, load16(Z + off + g * GC));
        store16(X + off + g * GC, x);
    }
}

bool gm_ok(const GmDims &g) { return g.m >= 1 && g.m <= BSM_GMRES_MAX_RESTART && g.kmax >= g.d.nrhs && g.kmax <= kCgMaxRhs; }

// the one-wave kernels: f(R{}, NC) for the vector type of g
template <typename F> hipError_t gm_small(const GmDims &g, F &&f) {
    if (!is_vec_type(g.d.dtype) || !gm_ok(g) || g.d.nrhs < 1) return hipErrorInvalidValue;
    with_types(g.d.dtype, [&](auto r, auto, auto nc) { f(r, nc); });
    return hipGetLastError();
}

}  // namespace

hipError_t launch_gm_start(const GmDims &g, bool first, int par, const void *B, long long ldb, const void *q, void *V0,
                           const GmSmall &s, const GmState *st, hipStream_t stream) {
    if (!gm_ok(g)) return hipErrorInvalidValue;
    return cg_dispatch(g.d, [&](auto rt, auto nc, long long ng, dim3 grid, auto) {
        using R = decltype(rt);
        constexpr int NC = decltype(nc)::value;
        hipLaunchKernelGGL((start_kernel<R, NC>), grid, dim3(kThreads), 0, stream, g.d.n, g.d.ld, ng, ldb, first ? 1 : 0, par,
                           (const R *)B, (const R *)q, (R *)V0, (R *)s.part, (long long)g.m * g.d.G * NC, (R *)s.nrm, st);
    });
}

hipError_t launch_gm_begin(const GmDims &g, bool first, int par, double rtol, double atol, void *V0, const GmSmall &s, GmState *st,
                           hipStream_t stream) {
    if (!gm_ok(g)) return hipErrorInvalidValue;
    return cg_dispatch(g.d, [&](auto rt, auto nc, long long ng, dim3 grid, auto) {
        using R = decltype(rt);
        constexpr int NC = decltype(nc)::value;
        hipLaunchKernelGGL((begin_kernel<R, NC>), grid, dim3(kThreads), 0, stream, g.d.ld, ng, first ? 1 : 0, par, g.m, rtol, atol,
                           (const R *)s.part, (long long)g.m * g.d.G * NC, (const R *)s.nrm, (R *)V0, (R *)s.g, (R *)s.hsum, st);
    });
}

hipError_t launch_gm_dot(const GmDims &g, int par, int k, const void *V, const void *W, const GmSmall &s, const GmState *st,
                         hipStream_t stream) {
    if (!gm_ok(g) || k < 1 || k > g.m) return hipErrorInvalidValue;
    return cg_dispatch(g.d, [&](auto rt, auto nc, long long ng, dim3 grid, auto) {
        using R = decltype(rt);
        constexpr int NC = decltype(nc)::value;
        hipLaunchKernelGGL((dot_kernel<R, NC>), grid, dim3(kThreads), 0, stream, g.d.ld, ng, (long long)g.kmax * g.d.ld, k, g.m, par,
                           (const R *)V, (const R *)W, (R *)s.part, st);
    });
}

hipError_t launch_gm_update(const GmDims &g, int par, int k, const void *V, void *W, const GmSmall &s, const GmState *st,
                            hipStream_t stream) {
    if (!gm_ok(g) || k < 1 || k > g.m) return hipErrorInvalidValue;
    return cg_dispatch(g.d, [&](auto rt, auto nc, long long ng, dim3 grid, auto) {
        using R = decltype(rt);
        constexpr int NC = decltype(nc)::value;
        hipLaunchKernelGGL((sweep_kernel<R, NC, true>), grid, dim3(kThreads), 0, stream, g.d.ld, ng, (long long)g.kmax * g.d.ld, k, g.m,
                           par, (const R *)V, (R *)W, (const R *)s.part, (const R *)nullptr, (R *)s.hsum, (R *)s.nrm, st);
    });
}

hipError_t launch_gm_combine(const GmDims &g, int par, const void *V, void *U, const GmSmall &s, const GmState *st, hipStream_t stream) {
    if (!gm_ok(g)) return hipErrorInvalidValue;
    return cg_dispatch(g.d, [&](auto rt, auto nc, long long ng, dim3 grid, auto) {
        using R = decltype(rt);
        constexpr int NC = decltype(nc)::value;
        hipLaunchKernelGGL((sweep_kernel<R, NC, false>), grid, dim3(kThreads), 0, stream, g.d.ld, ng, (long long)g.kmax * g.d.ld, 0, g.m,
                           par, (const R *)V, (R *)U, (const R *)nullptr, (const R *)s.y, (R *)nullptr, (R *)nullptr, st);
    });
}

hipError_t launch_gm_scale(const GmDims &g, int par, const void *W, void *Vn, const GmSmall &s, const GmState *st, hipStream_t stream) {
    if (!gm_ok(g)) return hipErrorInvalidValue;
    return cg_dispatch(g.d, [&](auto rt, auto nc, long long ng, dim3 grid, auto) {
        using R = decltype(rt);
        constexpr int NC = decltype(nc)::value;
        hipLaunchKernelGGL((scale_kernel<R, NC>), grid, dim3(kThreads), 0, stream, g.d.ld, ng, par, (const R *)W, (R *)Vn,
                           (const R *)s.inv, st);
    });
}

hipError_t launch_gm_axpy(const GmDims &g, int par, const void *Z, void *X, const GmState *st, hipStream_t stream) {
    if (!gm_ok(g)) return hipErrorInvalidValue;
    return cg_dispatch(g.d, [&](auto rt, auto nc, long long ng, dim3 grid, auto) {
        using R = decltype(rt);
        constexpr int NC = decltype(nc)::value;
        hipLaunchKernelGGL((axpy_kernel<R, NC>), grid, dim3(kThreads), 0, stream, g.d.ld, ng, par, (const R *)Z, (R *)X, st);
    });
}

hipError_t launch_gm_hess(const GmDims &g, int par, int j, const GmSmall &s, GmState *st, hipStream_t stream) {
    if (j < 0 || j >= g.m) return hipErrorInvalidValue;
    return gm_small(g, [&](auto r, auto nc) {
        using R = decltype(r);
        hipLaunchKernelGGL((hess_kernel<R, decltype(nc)::value>), dim3((unsigned)g.d.nrhs), dim3(64), 0, stream, g.d.G, g.m, j, par,
                           (const R *)s.nrm, (R *)s.hsum, (R *)s.Hm, (R *)s.cs, (R *)s.sn, (R *)s.g, (R *)s.inv, st);
    });
}

hipError_t launch_gm_trsolve(const GmDims &g, int par, const GmSmall &s, const GmState *st, hipStream_t stream) {
    return gm_small(g, [&](auto r, auto nc) {
        using R = decltype(r);
        hipLaunchKernelGGL((trsolve_kernel<R, decltype(nc)::value>), dim3((unsigned)g.d.nrhs), dim3(64), 0, stream, g.m, par,
                           (const R *)s.Hm, (const R *)s.g, (R *)s.y, st);
    });
}

}  // namespace bsm
