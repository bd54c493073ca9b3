// bsm_eigh.hip -- eigh_kernel (bsm_eigh_blocks) and spectral_kernel (bsm_spectral_blocks; include/bsm_rocm.h): a batch of
// dense Hermitian blocks of different orders, each decomposed -- or put together again as V f(w) V^H -- by one workgroup.
// Kept out of the product kernel units like bsm_invert.hip: the build id (Makefile BUILD_ID) names the kernels and schedule
// of the PRODUCTS, and a setup-time decomposition changes neither.
#include <hip/hip_runtime.h>

#include <type_traits>

#include "bsm_types.h"
#define BSM_EIGH_LAUNCH
#include "bsm_eigh.h"

namespace bsm {

// ========================================================================================
// eigh_kernel: the two-sided round-robin Jacobi method of bsm_eigh.h, one 256-thread workgroup per block.  A step has four
// phases with a __syncthreads() behind each:
//   derive  thread k < m / 2 takes pair k of the step (eigh_pair) and leaves its rotation record (eigh_rotation) in LDS;
//   columns A and V: x = col_p, y = conj(omega) col_q -> (c x - s y, s x + c y).  LANES ALONG THE ROWS, the contiguous direction:
//           a thread keeps row i = t mod P (P = n rounded up to a power of two, at most 256) and walks the pairs t / P,
//           t / P + 256 / P, ...;
//   rows    A only: the same with omega on rows p, q.  Resident blocks: lanes along the COLUMNS, the walk the odd leading
//           dimension of the LDS image is chosen for (eigh_ld);  larger blocks, rotated in device memory: lanes along the PAIRS,
//           whose p and q are runs of consecutive rows, so that a wave reads whole cache lines;
//   fix     the pair threads set a_pp, a_qq, zero a_pq and a_qp, and count their rotations.
// Pairs of a step are disjoint: every entry has one writer per phase and the order of the arithmetic is fixed -- the result is
// bit-identical from run to run.  The rotation count of a sweep is summed per wave by shuffles and across the four waves
// through LDS; every thread reads the same four numbers, so the decision to stop is uniform and EVERY BARRIER IS REACHED BY
// ALL 256 THREADS.  No workgroup waits for another one; no atomics.
// Two regimes, one instantiation each per type (the host splits its launches at the seam):
//   RES   2 n^2 sizeof(T) <= BSM_EIGH_LDS_BYTES: A and V live in LDS with leading dimension eigh_ld(n) for the whole solve;
//   !RES  up to n = 512: A is rotated in place in device memory with plain loads and stores, V in the scratch array of the
//         record (leading dimension n), and copied into the block at the end.
// Elements are NC = 1 or 2 reals: LDS images hold aligned elements (one ds_read / ds_write per element), device memory is
// read by real components, so the caller's blocks need the alignment of a real only.
// ========================================================================================
template <typename R, int NC> struct alignas(sizeof(R) * NC) El {
    R v[NC];
};

template <typename R, int NC> __device__ __forceinline__ El<R, NC> eget(const El<R, NC> *p, long long i) { return p[i]; }
template <typename R, int NC> __device__ __forceinline__ void eput(El<R, NC> *p, long long i, El<R, NC> e) { p[i] = e; }
template <typename R, int NC> __device__ __forceinline__ El<R, NC> gget(const R *p, long long i) {
    El<R, NC> e;
#pragma unroll
    for (int c = 0; c < NC; ++c) e.v[c] = p[i * NC + c];
    return e;
}
template <typename R, int NC> __device__ __forceinline__ void gput(R *p, long long i, El<R, NC> e) {
#pragma unroll
    for (int c = 0; c < NC; ++c) p[i * NC + c] = e.v[c];
}

// the matrix a phase works on: an LDS image of aligned elements or device memory read by components
template <typename R, int NC, bool LDS> struct Mat {
    using P = std::conditional_t<LDS, El<R, NC> *, R *>;
    P p;
    long long ld;
    __device__ __forceinline__ El<R, NC> get(long long i, long long j) const {
        if constexpr (LDS)
            return eget<R, NC>(p, i + j * ld);
        else
            return gget<R, NC>(p, i + j * ld);
    }
    __device__ __forceinline__ void put(long long i, long long j, El<R, NC> e) const {
        if constexpr (LDS)
            eput<R, NC>(p, i + j * ld, e);
        else
            gput<R, NC>(p, i + j * ld, e);
    }
};

template <typename R> struct RotRec {  // the arrays of the rotation records in LDS
    R *c, *s, *wre, *wim, *dpp, *dqq;
    int *kind;
};

template <typename R, int NC, bool RES>
__global__ void __launch_bounds__(256) eigh_kernel(const EighBlock *__restrict__ table, int *__restrict__ info, int nmax, int vectors) {
    using E = El<R, NC>;
    extern __shared__ __attribute__((aligned(16))) char smem[];
    const EighBlock *const blk = table + blockIdx.x;
    const int n = blk->n, id = blk->id, t = threadIdx.x, lane = t & 63, wave = t >> 6;
    const long long ldg = blk->ld;
    R *const Gm = reinterpret_cast<R *>(blk->ptr);
    R *const wout = reinterpret_cast<R *>(blk->w);
    const EighLds lo = eigh_lds(nmax, (int)sizeof(E), (int)sizeof(R), RES);
    const int npmax = (nmax + 1) / 2;
    int *const cnt = reinterpret_cast<int *>(smem);  // [0 .. 3]: the waves' rotation counts; [8]: a non-finite entry was seen
    RotRec<R> rr;
    rr.c = reinterpret_cast<R *>(smem + lo.rot);
    rr.s = rr.c + npmax, rr.wre = rr.s + npmax, rr.wim = rr.wre + npmax, rr.dpp = rr.wim + npmax, rr.dqq = rr.dpp + npmax;
    rr.kind = reinterpret_cast<int *>(rr.dqq + npmax);
    R *const wv = reinterpret_cast<R *>(smem + lo.wv);
    int *const rank = reinterpret_cast<int *>(smem + lo.rank);
    const int ldl = eigh_ld(n);
    Mat<R, NC, RES> A, V;
    if constexpr (RES) {
        A.p = reinterpret_cast<E *>(smem + lo.mat), A.ld = ldl;
        V.p = A.p + (long long)n * ldl, V.ld = ldl;
    } else {
        A.p = Gm, A.ld = ldg;
        V.p = reinterpret_cast<R *>(blk->aux), V.ld = n;
    }
    const Mat<R, NC, false> G{Gm, ldg};
    int P = 1, lg = 0;
    while (P < n && P < 256) P <<= 1, ++lg;
    const int NG = 256 >> lg, ti = t & (P - 1), tg = t >> lg;
    const int m = (n + 1) & ~1, np = m >> 1;
    int PK = 1, lgk = 0;  // the row phase of larger blocks: lanes along the pairs
    while (PK < np && PK < 256) PK <<= 1, ++lgk;
    const int NGK = 256 >> lgk, tk = t & (PK - 1), tj = t >> lgk;

    // ---- a non-finite entry ends the block before anything is written
    if (t == 0) cnt[8] = 0;
    __syncthreads();
    {
        bool bad = false;
        for (int i = ti; i < n; i += P)
            for (int j = tg; j < n; j += NG) {
                const E e = G.get(i, j);
#pragma unroll
                for (int c = 0; c < NC; ++c) bad = bad || !eh_finite(e.v[c]);
            }
        if (bad) cnt[8] = 1;  // (every writer stores the same value)
    }
    __syncthreads();
    if (cnt[8]) {  // uniform: read behind the barrier
        for (int i = t; i < n; i += 256) wout[i] = R(NAN);
        if (t == 0) info[2 * id] = 1, info[2 * id + 1] = 0;
        return;
    }
    // ---- H = (B + B^H) / 2, the pair (i, j), (j, i) by one thread; V = I
    for (int i = ti; i < n; i += P)
        for (int j = tg; j <= i; j += NG) {
            const E x = G.get(i, j), y = G.get(j, i);
            E h, hc;
            h.v[0] = hc.v[0] = (x.v[0] + y.v[0]) / R(2);
            if constexpr (NC == 2) {
                const R im = i == j ? R(0) : (x.v[NC - 1] - y.v[NC - 1]) / R(2);
                h.v[NC - 1] = im;
                hc.v[NC - 1] = i == j ? R(0) : -im;
            }
            A.put(i, j, h);
            A.put(j, i, hc);
        }
    if (vectors)
        for (int i = ti; i < n; i += P)
            for (int j = tg; j < n; j += NG) {
                E e;
#pragma unroll
                for (int c = 0; c < NC; ++c) e.v[c] = R(0);
                if (i == j) e.v[0] = R(1);
                V.put(i, j, e);
            }
    __syncthreads();

    int sweeps = 0, status = 2;
    while (sweeps < BSM_EIGH_MAX_SWEEPS) {  // (uniform: sweeps and the exit below are the same in every thread)
        int rotated = 0;
        for (int st = 0; st < m - 1; ++st) {
            // ---- derive
            int p = 0, q = 0, kind = 0;
            R dpp = R(0), dqq = R(0);
            if (t < np) {
                eigh_pair(m, st, t, p, q);
                if (q < n) {
                    const E apq = A.get(p, q);
                    const EighRot<R> r = eigh_rotation<R, NC>(A.get(p, p).v[0], A.get(q, q).v[0], apq.v[0], NC == 2 ? apq.v[NC - 1] : R(0));
                    kind = r.kind, dpp = r.dpp, dqq = r.dqq;
                    rr.c[t] = r.c, rr.s[t] = r.s, rr.wre[t] = r.wre, rr.wim[t] = r.wim;
                }
                rr.kind[t] = kind;
            }
            __syncthreads();
            // ---- columns
            for (int k = tg; k < np; k += NG) {
                if (rr.kind[k] != 2) continue;
                int kp, kq;
                eigh_pair(m, st, k, kp, kq);
                const R c = rr.c[k], s = rr.s[k], wre = rr.wre[k], wim = rr.wim[k];
                for (int i = ti; i < n; i += P) {
                    E x = A.get(i, kp), y = A.get(i, kq);
                    eigh_apply<R, NC>(c, s, wre, wim, R(-1), x.v, y.v);
                    A.put(i, kp, x);
                    A.put(i, kq, y);
                    if (vectors) {
                        E u = V.get(i, kp), w = V.get(i, kq);
                        eigh_apply<R, NC>(c, s, wre, wim, R(-1), u.v, w.v);
                        V.put(i, kp, u);
                        V.put(i, kq, w);
                    }
                }
            }
            __syncthreads();
            // ---- rows
            if constexpr (RES) {
                for (int k = tg; k < np; k += NG) {
                    if (rr.kind[k] != 2) continue;
                    int kp, kq;
                    eigh_pair(m, st, k, kp, kq);
                    const R c = rr.c[k], s = rr.s[k], wre = rr.wre[k], wim = rr.wim[k];
                    for (int j = ti; j < n; j += P) {
                        E x = A.get(kp, j), y = A.get(kq, j);
                        eigh_apply<R, NC>(c, s, wre, wim, R(1), x.v, y.v);
                        A.put(kp, j, x);
                        A.put(kq, j, y);
                    }
                }
            } else {
                for (int k = tk; k < np; k += PK) {
                    if (rr.kind[k] != 2) continue;
                    int kp, kq;
                    eigh_pair(m, st, k, kp, kq);
                    const R c = rr.c[k], s = rr.s[k], wre = rr.wre[k], wim = rr.wim[k];
                    for (int j = tj; j < n; j += NGK) {
                        E x = A.get(kp, j), y = A.get(kq, j);
                        eigh_apply<R, NC>(c, s, wre, wim, R(1), x.v, y.v);
                        A.put(kp, j, x);
                        A.put(kq, j, y);
                    }
                }
            }
            __syncthreads();
            // ---- fix
            if (kind != 0) {
                E z;
#pragma unroll
                for (int c = 0; c < NC; ++c) z.v[c] = R(0);
                A.put(p, q, z);
                A.put(q, p, z);
                if (kind == 2) {
                    ++rotated;
                    E d = z;
                    d.v[0] = dpp;
                    A.put(p, p, d);
                    d.v[0] = dqq;
                    A.put(q, q, d);
                }
            }
            __syncthreads();
        }
#pragma unroll
        for (int d = 32; d >= 1; d >>= 1) rotated += __shfl_xor(rotated, d, 64);
        if (lane == 0) cnt[wave] = rotated;
        __syncthreads();
        const int total = cnt[0] + cnt[1] + cnt[2] + cnt[3];  // (rewritten behind the barriers of the next sweep's steps)
        if (total == 0) {
            status = 0;
            break;
        }
        ++sweeps;
    }

    // ---- the order: a rank sort of the diagonal, stable
    for (int i = t; i < n; i += 256) wv[i] = A.get(i, i).v[0];
    __syncthreads();
    for (int i = t; i < n; i += 256) {
        const R wi = wv[i];
        int r = 0;
        for (int j = 0; j < n; ++j) {
            const R wj = wv[j];
            r += (wj < wi || (wj == wi && j < i)) ? 1 : 0;
        }
        rank[i] = r;
        wout[r] = wi;
    }
    __syncthreads();  // (larger blocks: A, which the block held, is read no more)
    if (vectors)
        for (int i = ti; i < n; i += P)
            for (int j = tg; j < n; j += NG) G.put(i, rank[j], V.get(i, j));
    if (t == 0) info[2 * id] = status, info[2 * id + 1] = sweeps;
}

// ========================================================================================
// spectral_kernel: out = V diag(f(w)) V^H, one 256-thread workgroup per block.  Every thread finds wmax (the loads are the same
// in all lanes); thread k, k + 256, .. leaves f_k in LDS and remembers the first k at which f is undefined, the smallest such k
// is agreed on through LDS (a min: independent of the order) -- it ends the block, uniformly, before out is written.  Then a
// thread keeps row i = t mod P and U columns j = t / P + u * (256 / P) at a time and sums k ascending with fused multiply-adds:
// t_k = f_k V[i, k], acc += t_k conj(V[j, k]); entries with i >= j are computed and stored with their mirror image.  V comes
// from LDS (STAGED: n^2 sizeof(T) <= BSM_EIGH_LDS_BYTES, leading dimension n: the lanes of a wave read consecutive rows of a
// column, V[j, k] is one address for all of them) or from device memory.
// ========================================================================================
template <typename R, int NC, bool STAGED>
__global__ void __launch_bounds__(256) spectral_kernel(const EighBlock *__restrict__ table, int *__restrict__ info, int nmax, int func,
                                                         double rcond) {
    using E = El<R, NC>;
    constexpr int U = 4;
    extern __shared__ __attribute__((aligned(16))) char smem[];
    const EighBlock *const blk = table + blockIdx.x;
    const int n = blk->n, id = blk->id, t = threadIdx.x, lane = t & 63, wave = t >> 6;
    const R *const wsrc = reinterpret_cast<const R *>(blk->w);
    const Mat<R, NC, false> Vg{reinterpret_cast<R *>(blk->ptr), blk->ld}, Og{reinterpret_cast<R *>(blk->aux), blk->ld2};
    int *const cnt = reinterpret_cast<int *>(smem);
    R *const f = reinterpret_cast<R *>(smem + 64);
    Mat<R, NC, STAGED> V;
    if constexpr (STAGED) {
        V.p = reinterpret_cast<E *>(smem + 64 + ((nmax * (int)sizeof(R) + 15) & ~15)), V.ld = n;
    } else {
        V.p = Vg.p, V.ld = Vg.ld;
    }
    int P = 1, lg = 0;
    while (P < n && P < 256) P <<= 1, ++lg;
    const int NG = 256 >> lg, ti = t & (P - 1), tg = t >> lg;

    R wmax = R(0);
    for (int k = 0; k < n; ++k) {
        const R a = eh_abs(wsrc[k]);
        if (eh_finite(a) && a > wmax) wmax = a;
    }
    const R bound = spectral_bound<R>(rcond, wmax);
    int bad = 0x7fffffff;
    for (int k = t; k < n; k += 256) {
        R fk;
        if (!spectral_f<R>(func, wsrc[k], bound, fk) && k < bad) bad = k;
        f[k] = fk;
    }
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) {
        const int o = __shfl_xor(bad, d, 64);
        bad = o < bad ? o : bad;
    }
    if (lane == 0) cnt[wave] = bad;
    if constexpr (STAGED)
        for (int i = ti; i < n; i += P)
            for (int j = tg; j < n; j += NG) V.put(i, j, Vg.get(i, j));
    __syncthreads();
    int first = cnt[0];
#pragma unroll
    for (int w = 1; w < 4; ++w) first = cnt[w] < first ? cnt[w] : first;
    if (first != 0x7fffffff) {  // uniform
        if (t == 0) info[id] = first + 1;
        return;
    }
    for (int i = ti; i < n; i += P)
        for (int j0 = tg; j0 <= i; j0 += NG * U) {
            R re[U], im[U];
#pragma unroll
            for (int u = 0; u < U; ++u) re[u] = im[u] = R(0);
            for (int k = 0; k < n; ++k) {
                const E vi = V.get(i, k);
                const R fk = f[k];
                const R tr = fk * vi.v[0], tim = NC == 2 ? fk * vi.v[NC - 1] : R(0);
#pragma unroll
                for (int u = 0; u < U; ++u) {
                    const int j = j0 + u * NG;
                    if (j > i) continue;
                    const E vj = V.get(j, k);
                    re[u] = eh_fma(tr, vj.v[0], re[u]);
                    if constexpr (NC == 2) {
                        re[u] = eh_fma(tim, vj.v[NC - 1], re[u]);
                        im[u] = eh_fma(tim, vj.v[0], im[u]);
                        im[u] = eh_fma(-tr, vj.v[NC - 1], im[u]);
                    }
                }
            }
#pragma unroll
            for (int u = 0; u < U; ++u) {
                const int j = j0 + u * NG;
                if (j > i) continue;
                E o, oc;
                o.v[0] = oc.v[0] = re[u];
                if constexpr (NC == 2) {
                    o.v[NC - 1] = i == j ? R(0) : im[u];
                    oc.v[NC - 1] = i == j ? R(0) : -im[u];
                }
                Og.put(i, j, o);
                Og.put(j, i, oc);
            }
        }
    if (t == 0) info[id] = 0;
}

template <typename K> static hipError_t raise_lds(K kernel, size_t lds) {
    if (lds <= 65536) return hipSuccess;
    return hipFuncSetAttribute(reinterpret_cast<const void *>(kernel), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
}

hipError_t launch_eigh(int dtype, const void *d_table, long long count, int nmax, bool resident, int vectors, void *d_info,
                       hipStream_t stream) {
    if (count <= 0) return hipSuccess;
    const dim3 grid((unsigned)count), block(256);
    hipError_t e = hipErrorInvalidValue;
    with_types(dtype, [&](auto r, auto, auto nc) {
        using R = decltype(r);
        constexpr int NC = decltype(nc)::value;
        const size_t lds = (size_t)eigh_lds(nmax, (int)sizeof(R) * NC, (int)sizeof(R), resident).total;
        if (resident) {
            e = raise_lds(&eigh_kernel<R, NC, true>, lds);
            if (e != hipSuccess) return;
            hipLaunchKernelGGL((eigh_kernel<R, NC, true>), grid, block, lds, stream, (const EighBlock *)d_table, (int *)d_info, nmax, vectors);
        } else {
            hipLaunchKernelGGL((eigh_kernel<R, NC, false>), grid, block, lds, stream, (const EighBlock *)d_table, (int *)d_info, nmax, vectors);
        }
        e = hipGetLastError();
    });
    return e;
}

hipError_t launch_spectral(int dtype, const void *d_table, long long count, int nmax, bool staged, int func, double rcond,
                           void *d_info, hipStream_t stream) {
    if (count <= 0) return hipSuccess;
    const dim3 grid((unsigned)count), block(256);
    hipError_t e = hipErrorInvalidValue;
    with_types(dtype, [&](auto r, auto, auto nc) {
        using R = decltype(r);
        constexpr int NC = decltype(nc)::value;
        const size_t lds = (size_t)spectral_lds(nmax, (int)sizeof(R) * NC, (int)sizeof(R), staged);
        if (staged) {
            e = raise_lds(&spectral_kernel<R, NC, true>, lds);
            if (e != hipSuccess) return;
            hipLaunchKernelGGL((spectral_kernel<R, NC, true>), grid, block, lds, stream, (const EighBlock *)d_table, (int *)d_info, nmax, func,
                               rcond);
        } else {
            hipLaunchKernelGGL((spectral_kernel<R, NC, false>), grid, block, lds, stream, (const EighBlock *)d_table, (int *)d_info, nmax, func,
                               rcond);
        }
        e = hipGetLastError();
    });
    return e;
}

}  // namespace bsm
