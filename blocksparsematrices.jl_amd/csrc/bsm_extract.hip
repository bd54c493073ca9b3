// bsm_extract.hip -- extract_kernel (bsm_submatrices / bsm_diag, include/bsm_rocm.h): entries of the operator read out
// of its packed image.  Kept out of the product kernel units (bsm_kernels.hip has their index): the build id (Makefile
// BUILD_ID) names the kernels and schedule of the PRODUCTS, and reading entries changes neither.
#include "bsm_device.h"
#include "bsm_types.h"

namespace bsm {

// ========================================================================================
// A[I_s, J_s] for nsets pairs of index sets in ONE pass over the image.  The row sets are pairwise disjoint and so
// are the column sets, so four int32 maps say everything about a request: the set a row (column) of the stored
// operator belongs to (-1: not requested) and its position inside that set.  A stored entry (r, c) is wanted when
// rset[r] == cset[c] >= 0 and is ADDED into the window of that set (overlapping blocks of a BlockSparseMatrix sum,
// like sparse(A) and mul!'s +=, and the image does not record where they overlap).
// One wave per WaveWork descriptor, the decode of export_coo_kernel (bsm_util.hip), but with the lanes laid along
// the ROWS of a strip as the product kernels read: lane = (strip g of G = 64 / P, row i < P), so a wave-instruction
// loads G * m consecutive 16-byte units.  A lane keeps ONE row for the whole piece and looks it up once per role
// (forward; transposed for the off-diagonal columns of a symmetric operator); a wave none of whose rows is requested
// leaves without touching a value byte.  The columns are looked up 64 at a time, one per lane: a chunk none of whose
// columns lies in a set of the wave's rows is skipped with one ballot, inside a chunk a lane loads its unit only when
// one of the unit's E columns belongs to the set of the lane's row.
// DIAG: the same walk for diag(A) -- no maps, the condition is row == column, the address d + row.
// ========================================================================================
template <typename T, typename S, bool DIAG>
__global__ void __launch_bounds__(64 * kWavesPerWg) extract_kernel(const WaveWork *__restrict__ waves, long long nwaves,
                                                                  const uint4 *__restrict__ values, const int *__restrict__ rows,
                                                                  const int *__restrict__ cols, ExtractMaps mp,
                                                                  const ExtractOut *__restrict__ table, T *__restrict__ d,
                                                                  int nrows_tot, int ncols_tot, int opT, int conj) {
    constexpr int E = TT<S>::E;
    const long long wv = (long long)blockIdx.x * kWavesPerWg + (threadIdx.x >> 6);
    if (wv >= nwaves) return;  // whole waves leave: the shuffles below only ever run with all 64 lanes
    const int lane = threadIdx.x & 63;
    const WaveD wd = load_wave(waves + wv);
    if (wd.work != WORK_PANEL || wd.npieces == 0) return;
    const PieceD pc = wd.first;
    const int m = wd.m, ncols = pc.ncols, nstrips = pc.nstrips;
    const ColMap cm = col_map(wd, pc);
    const Vec16<S> *__restrict__ vb = reinterpret_cast<const Vec16<S> *>(values + (((uint64_t)pc.val_hi << 32) | pc.val_lo));
    int P = 8, lg = 3;
    while (P < m) P <<= 1, ++lg;
    const int G = 64 >> lg;
    const int i = lane & (P - 1), g = lane >> lg;
    const bool rvalid = i < m;
    const int ri = rvalid ? row_index(wd, rows, i) : -1;

    // the lane's row in both roles: (fs, fp) = its set and position as a ROW of the stored operator, (ts, tp) as a
    // COLUMN (the transposed copy of an off-diagonal entry (r, c) of a symmetric operator sits at (c, r))
    int fs = -1, fp = 0, ts = -1, tp = 0;
    int lo_f = 0x7fffffff, hi_f = -1, lo_t = 0x7fffffff, hi_t = -1;
    if constexpr (!DIAG) {
        if (rvalid) {
            fs = mp.rset[ri];
            if (fs >= 0) fp = mp.rpos[ri];
            if ((pc.kind & kKindHasOff) && ri < ncols_tot) {
                ts = mp.cset[ri];
                if (ts >= 0) tp = mp.cpos[ri];
            }
        }
        if (__ballot(fs >= 0 || ts >= 0) == 0ull) return;
        lo_f = fs >= 0 ? fs : 0x7fffffff, hi_f = fs;
        lo_t = ts >= 0 ? ts : 0x7fffffff, hi_t = ts;
    } else {
        lo_f = rvalid ? ri : 0x7fffffff, hi_f = ri;
    }
#pragma unroll
    for (int dd = 32; dd >= 1; dd >>= 1) {
        lo_f = min(lo_f, __shfl_xor(lo_f, dd, 64));
        hi_f = max(hi_f, __shfl_xor(hi_f, dd, 64));
        if constexpr (!DIAG) {
            lo_t = min(lo_t, __shfl_xor(lo_t, dd, 64));
            hi_t = max(hi_t, __shfl_xor(hi_t, dd, 64));
        }
    }

    for (int w0 = 0; w0 < ncols; w0 += 64) {
        // lane = one column of the chunk: its index, its kind, and what the maps say about it
        const int w = w0 + lane;
        bool off = false;
        int ci = -1, cs = -1, us = -1;
        if (w < ncols) {
            const int raw = cm.xbase < 0 ? cols[cm.col_off + w] : 0;
            ci = col_decode(cm, w, raw, off);
            if constexpr (!DIAG) {
                cs = mp.cset[ci];
                if (off && ci < nrows_tot) us = mp.rset[ci];
            }
        }
        bool wanted;
        if constexpr (DIAG)
            wanted = ci >= lo_f && ci <= hi_f;
        else
            wanted = (cs >= lo_f && cs <= hi_f) || (us >= lo_t && us <= hi_t);
        if (__ballot(wanted) == 0ull) continue;
        const bool any_off = __ballot(off) != 0ull;
        const int sbase = w0 / E;
        for (int s0 = 0; s0 < 64 / E && sbase + s0 < nstrips; s0 += G) {
            const int sl = s0 + g;  // the lane's strip inside the chunk (G divides 64 / E: sl * E + e < 64)
            int cie[E];
            unsigned fm = 0, tm = 0;
#pragma unroll
            for (int e = 0; e < E; ++e) {
                const int k = sl * E + e;
                cie[e] = __shfl(ci, k, 64);
                if constexpr (DIAG) {
                    const int o = any_off ? __shfl((int)off, k, 64) : 0;
                    if (rvalid && cie[e] == ri) fm |= 1u << e, tm |= o ? 1u << e : 0u;
                } else {
                    const int c_s = __shfl(cs, k, 64);
                    if (fs >= 0 && c_s == fs) fm |= 1u << e;
                    if (any_off) {
                        const int u_s = __shfl(us, k, 64);
                        if (ts >= 0 && u_s == ts) tm |= 1u << e;
                    }
                }
            }
            if ((fm | tm) == 0u) continue;  // (a matching column is a valid one: its strip exists)
            const Vec16<S> v = load_stream16(vb + ((long long)(sbase + sl) * m + i));
#pragma unroll
            for (int e = 0; e < E; ++e) {
                if (((fm | tm) >> e & 1u) == 0u) continue;
                const T val = cj(widen(T{}, v.v[e]), conj != 0);
                if constexpr (DIAG) {
                    atomic_acc(d + ri, val);
                    if (tm >> e & 1u) atomic_acc(d + ri, val);
                } else {
                    if (fm >> e & 1u) {
                        const ExtractOut o = table[fs];
                        const long long cp = mp.cpos[cie[e]];
                        atomic_acc(reinterpret_cast<T *>(o.ptr) + (opT ? cp + o.ld * fp : fp + o.ld * cp), val);
                    }
                    if (tm >> e & 1u) {
                        const ExtractOut o = table[ts];
                        const long long up = mp.rpos[cie[e]];
                        atomic_acc(reinterpret_cast<T *>(o.ptr) + (opT ? tp + o.ld * up : up + o.ld * tp), val);
                    }
                }
            }
        }
    }
}

// the ni x nj window of every set = 0 (blockIdx.x: set, blockIdx.y: slice of the window); nothing outside a window is
// written, the ld padding included
template <typename T>
__global__ void __launch_bounds__(256) zero_windows_kernel(const ExtractOut *__restrict__ table, const long long *__restrict__ shape,
                                                           long long nsets) {
    for (long long s = blockIdx.x; s < nsets; s += gridDim.x) {
        const ExtractOut o = table[s];
        const long long ni = shape[2 * s], cnt = ni * shape[2 * s + 1];
        T *__restrict__ p = reinterpret_cast<T *>(o.ptr);
        for (long long k = (long long)blockIdx.y * 256 + threadIdx.x; k < cnt; k += (long long)gridDim.y * 256)
            p[k % ni + (k / ni) * o.ld] = zero_of(T{});
    }
}

hipError_t launch_zero_windows(int vt, const void *d_table, const void *d_shape, long long nsets, long long largest,
                               hipStream_t stream) {
    if (nsets <= 0 || largest <= 0) return hipSuccess;
    const long long gy = (largest + 4095) / 4096;  // 16 entries per thread where a window is large
    const dim3 grid((unsigned)(nsets < 65535 ? nsets : 65535), (unsigned)(gy < 1024 ? gy : 1024)), block(256);
    return with_pair(vt, vt, [&](auto t, auto) {  // (the same-type pair of vt: its T)
        using T = decltype(t);
        hipLaunchKernelGGL((zero_windows_kernel<T>), grid, block, 0, stream, (const ExtractOut *)d_table, (const long long *)d_shape, nsets);
        return hipGetLastError();
    });
}

hipError_t launch_extract(int dtype, const void *d_waves, long long nwaves, const void *d_values, const void *d_rows,
                          const void *d_cols, const ExtractMaps *maps, const void *d_table, void *d_diag, long long nrows,
                          long long ncols, bool opT, bool conj, hipStream_t stream) {
    if (nwaves <= 0) return hipSuccess;
    const dim3 grid((unsigned)((nwaves + kWavesPerWg - 1) / kWavesPerWg)), block(64 * kWavesPerWg);
    const ExtractMaps mp = maps ? *maps : ExtractMaps{nullptr, nullptr, nullptr, nullptr};
    return with_pair(dtype, vec_type(dtype), [&](auto t, auto st) {
        using T = decltype(t);
        using S = decltype(st);
        // (complex vectors under a real image are no pair of vec_type: no kernel is made for them)
        if constexpr (std::is_arithmetic<T>::value != std::is_arithmetic<S>::value) return hipErrorInvalidValue;
        else if (maps)
            hipLaunchKernelGGL((extract_kernel<T, S, false>), grid, block, 0, stream, (const WaveWork *)d_waves, nwaves,
                               (const uint4 *)d_values, (const int *)d_rows, (const int *)d_cols, mp, (const ExtractOut *)d_table,
                               (T *)nullptr, (int)nrows, (int)ncols, (int)opT, (int)conj);
        else
            hipLaunchKernelGGL((extract_kernel<T, S, true>), grid, block, 0, stream, (const WaveWork *)d_waves, nwaves,
                               (const uint4 *)d_values, (const int *)d_rows, (const int *)d_cols, mp, (const ExtractOut *)nullptr,
                               (T *)d_diag, (int)nrows, (int)ncols, (int)opT, (int)conj);
        return hipGetLastError();
    });
}

}  // namespace bsm
