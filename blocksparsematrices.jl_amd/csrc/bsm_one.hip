// bsm_one.hip -- the one-column family: panel_kernel (run_panel) and the two passes around it in accumulate mode,
// scale_kernel (`y .*= beta`, also in front of the multi-RHS kernels: launch_scale) and gather_kernel.
//
//   forward    u[i]  = sum_w B[i,w] * x[col(w)]     lane owns a row, 16-byte lane loads,
//                                                    x slice staged through LDS per wave
//   transposed v[w]  = sum_i B[i,w] * x[row(i)]     same bytes, halving butterfly across the
//                                                    P lanes of a strip, then y[col(w)] += v
//
// Both directions are taken from ONE read of the piece (SymmetricBlockMatrix off-diagonal
// blocks: reference src/symmetricblockmatrix.jl:394-418 reads them twice).
// The kernels are HBM-bound (0.25-0.5 FLOP/B): no MFMA, everything is about keeping
// >= 8 KB per wave in flight with perfectly coalesced 16-byte loads.
#include "bsm_device.h"
#include "bsm_families.h"

namespace bsm {

#ifndef BSM_C64_FUSED_WAVES
#define BSM_C64_FUSED_WAVES 5
#endif
#ifndef BSM_C128_FUSED_WAVES
#define BSM_C128_FUSED_WAVES 6
#endif

// ----------------------------------------------------------------------------------------
// one wave streams its pieces; returns the forward partial sum of row (lane % P)
// ----------------------------------------------------------------------------------------
// S: the stored type (= T, or float / c64 under double / c128 vectors).  A strip is 16 bytes of S, i.e. E = 16 /
// sizeof(S) columns, so a mixed image's strip covers E entries of the T-typed x slice (4 fp64 / 2 complex128).
template <typename T, int L, int P, bool FWD, bool TRN, bool NT, typename S = T>
__device__ __forceinline__ T run_panel(const WaveD &wd, const uint4 *__restrict__ values,
                                       const int *__restrict__ rows, const int *__restrict__ cols,
                                       const T *__restrict__ x, T *__restrict__ y, T alpha,
                                       int flags, int lane, T *xs, T *vs, T *win, int win_n,
                                       T *__restrict__ ws) {
    constexpr int E = TT<S>::E;
    constexpr int G = 64 / P;
    constexpr int V = L * E;
    constexpr int NC = G * L * E;                        // columns covered per iteration
    constexpr int XCH = x_chunk_cols<T, TRN>();            // columns staged per x chunk
    // the E x entries of one strip, read from the slice as one LDS access (16 bytes; 32 for a mixed image)
    using XV = typename std::conditional<std::is_same<S, T>::value, Vec16<T>, XVec<T, E>>::type;
    // iterations per transposed emission: the column sums of a whole staged chunk leave the wave
    // together.  Atomics (and the plain stores of the gather mode) sit in the same in-order vmcnt
    // queue as the loads and take 2-3x as long under load (MI355X_MICROARCH.md: ~3000 cycles with
    // every CU issuing): emitted every iteration, each one is waited for by the NEXT iteration's
    // matrix loads; emitted at the chunk end of a small panel, nothing ever waits for them.
    constexpr int BF = XCH / NC;
    static_assert(XCH % NC == 0, "x chunk must hold whole iterations");
    constexpr bool INPLACE = FWD && TRN;  // column sums parked in the x slice, y indices of the chunk kept in `vs`
    int *ix = reinterpret_cast<int *>(vs);
    const bool opT = (flags & FLAG_OPT) != 0;
    const bool cjf = (flags & FLAG_CONJ) != 0;
    const int m = wd.m;
    const int i = lane & (P - 1);
    const int g = lane / P;
    const bool row_ok = i < m;

    T acc[E];
#pragma unroll
    for (int e = 0; e < E; ++e) acc[e] = zero_of(T{});
    T xr = zero_of(T{});
    if (TRN && row_ok) {
        // (issuing this second round trip together with the x gather of the first chunk's columns, so that
        // the rows -> x and columns -> x chains overlap, changed nothing on the tiled BEM fixture and costs
        // the fp64 / fp32 fused instances a register they do not have)
        const int ri = row_index(wd, rows, i);
        xr = x[ri];
    }

    const PieceD pc = wd.first;
    if (wd.npieces > 0) {
        const int xbase = pc.xbase;
        const int col_off = pc.col_off;
        const int nstrips = pc.nstrips;
        const int ncols = pc.ncols;
        // per-column kinds (a symmetric row group holds its diagonal block and its off-diagonal
        // blocks in one panel): forward uses a column unless (op T/C and it is not KIND_OFF),
        // transposed uses it iff (op T/C or KIND_OFF)
        const int kinds = pc.kind;
        const bool has_off = (kinds & kKindHasOff) != 0;
        const bool fwd_en = FWD && (!opT || has_off);
        const bool trn_en = TRN && (opT || has_off);
        const Vec16<S> *__restrict__ vb = reinterpret_cast<const Vec16<S> *>(
            values + (((uint64_t)pc.val_hi << 32) | pc.val_lo));
        // piece column -> x / y index: up to three inline contiguous runs, else the cols pool
        const int s1w = wd.seg1_w, s1x = wd.seg1_x - wd.seg1_w;
        const int s2w = wd.seg2_w, s2x = pc.seg2_x - wd.seg2_w;
        // -> x / y index of piece column w; `off` tells whether the column is KIND_OFF
        auto col_lookup = [&](int w, bool &off) -> int {
            if (xbase < 0) {
                const int raw = cols[col_off + w];
                off = raw >= 0 && (kinds & 3) == KIND_OFF;
                return raw & 0x7fffffff;
            }
            const int sh = w < s1w ? 0 : (w < s2w ? 2 : 4);
            off = ((kinds >> sh) & 3) == KIND_OFF;
            return w + (w < s1w ? xbase : (w < s2w ? s1x : s2x));
        };

        // L independent 16-byte loads per lane: 8 KB of the matrix per wave in flight
        auto load_b = [&](Vec16<S>(&b)[L], int s0) {
#pragma unroll
            for (int l = 0; l < L; ++l) {
                const int s = s0 + l * G + g;
                if (row_ok && s < nstrips) {
                    b[l] = NT ? load_stream16(&vb[(uint32_t)(s * m + i)]) : vb[(uint32_t)(s * m + i)];
                } else {
#pragma unroll
                    for (int e = 0; e < E; ++e) b[l].v[e] = zero_of(S{});
                }
            }
        };
        // x slice of a chunk: gathered ONCE per wave into LDS (contiguous runs or through the merged
        // column list), then read back as 16-byte broadcasts by every iteration of the chunk.  The
        // gather is branch-free and batched -- all column-list loads, then all x loads, then the LDS
        // stores: ONE memory round trip (two through the list) instead of a dependent load / wait /
        // store per 64 columns, which tools/wavetrace.py showed as 0.9 us (median) to 3.4 us (p90) of
        // a 9.7 us C2 launch.  A lane past the last column loads the last column's entry and stores
        // zero (the tail one iteration past the end must read as zero).
        auto stage_x = [&](int c0, auto kx_tag) {
            constexpr int KX = decltype(kx_tag)::value;
            const bool pool = xbase < 0;  // wave-uniform
            int raw[KX];                  // column-list entries (pool) -- the only state kept per column
            T xv[KX];
            if (pool) {
#pragma unroll
                for (int k = 0; k < KX; ++k) raw[k] = cols[col_off + min(c0 + k * 64 + lane, ncols - 1)];
#pragma unroll
                for (int k = 0; k < KX; ++k) xv[k] = x[raw[k] & 0x7fffffff];
            } else {
#pragma unroll
                for (int k = 0; k < KX; ++k) {
                    bool off;
                    raw[k] = 0;
                    xv[k] = x[col_lookup(min(c0 + k * 64 + lane, ncols - 1), off)];
                }
            }
#pragma unroll
            for (int k = 0; k < KX; ++k) {
                const int w = c0 + k * 64 + lane;
                bool off;
                int yi = raw[k] & 0x7fffffff;
                if (pool)
                    off = raw[k] >= 0 && (kinds & 3) == KIND_OFF;
                else
                    yi = col_lookup(min(w, ncols - 1), off);
                xs[k * 64 + lane] = (w < ncols && (!opT || off)) ? xv[k] : zero_of(T{});
                // fused kernels: the transposed emission of this chunk finds its y index here (sign bit: the column
                // takes no part in it) instead of reading the column list a second time, a dependent round trip per
                // 64 columns in front of the atomics
                if (INPLACE) ix[k * 64 + lane] = (w < ncols && (opT || off)) ? yi : -1;
            }
        };

        // the x slice of the chunk that starts at column c0
        auto stage_chunk = [&](int c0) {
            // (a fused wave whose piece has no forward half in this op still needs the chunk's y indices)
            if (!fwd_en && !(INPLACE && trn_en)) return;
            if (BSM_DBG(DBG_NO_XGATHER)) {
#pragma unroll
                for (int k = 0; k < XCH / 64; ++k) {
                    xs[k * 64 + lane] = alpha;
                    if (INPLACE) {
                        const int w = c0 + k * 64 + lane;
                        bool off = false;
                        const int yi = col_lookup(min(w, ncols - 1), off);
                        ix[k * 64 + lane] = (w < ncols && (opT || off)) ? yi : -1;
                    }
                }
                return;
            }
            constexpr int KXM = XCH / 64;
            const int need = min(ncols - c0, XCH) + NC;  // columns the chunk's iterations read
            if (KXM >= 4 && need <= (KXM / 4) * 64)
                stage_x(c0, std::integral_constant<int, (KXM >= 4 ? KXM / 4 : 1)>{});
            else if (KXM >= 2 && need <= (KXM / 2) * 64)
                stage_x(c0, std::integral_constant<int, (KXM >= 2 ? KXM / 2 : 1)>{});
            else
                stage_x(c0, std::integral_constant<int, KXM>{});
        };
        // one iteration on the L loaded strips-per-group starting at strip s0 of the chunk [c0, c0 + XCH)
        auto iteration = [&](Vec16<S>(&b)[L], int s0, int c0, int s_end) {
            if (fwd_en) {
                const int cb = (s0 - c0 / E) * E;  // first column of this iteration inside the chunk
#pragma unroll
                for (int l = 0; l < L; ++l) {
                    const XV xv = *reinterpret_cast<const XV *>(&xs[cb + (l * G + g) * E]);
#pragma unroll
                    for (int e = 0; e < E; ++e) acc[e] = madd(acc[e], widen(T{}, cj(b[l].v[e], cjf)), xv.v[e]);
                }
            }
#ifdef BSM_TRACE
            if (s0 == 0) {
                asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
                BSM_TSTAMP(3);  // first iteration's matrix bytes have arrived
            }
#endif
            if (trn_en) {
                T vals[V];
#pragma unroll
                for (int l = 0; l < L; ++l)
#pragma unroll
                    for (int e = 0; e < E; ++e) vals[l * E + e] = mul(widen(T{}, cj(b[l].v[e], cjf)), xr);
                int pos = 0, dup = 0;
                if (!BSM_DBG(DBG_NO_BUTTERFLY)) Butterfly<T, V, P>::run(vals, i, pos, dup);
                constexpr int CF = (V / P) > 1 ? (V / P) : 1;
                // the column sums of the chunk's iterations are parked in LDS and leave the wave
                // together (64 busy lanes per atomic wave-instruction instead of NC)
                const int slot = (s0 - c0 / E) / (G * L);
                // fused kernels park IN PLACE: slot c of the x slice holds x of chunk column c until the forward half of
                // its iteration has read it (above: the same wave, LDS in program order), then the column's sum
                T *park = INPLACE ? xs : vs;
                if ((i & dup) == 0) {
#pragma unroll
                    for (int j = 0; j < CF; ++j) {
                        const int q = pos + j;  // original value index l*E + e
                        const int l = q / E, e = q % E;
                        park[slot * NC + (l * G + g) * E + e] = vals[j];
                    }
                }
                const bool last_it = (s0 + G * L >= s_end);
                if ((slot == BF - 1 || last_it) && !BSM_DBG(DBG_NO_EMISSION)) {
                    const int sb = s0 - slot * (G * L);  // first strip of the batch
                    const int nbatch = min((slot + 1) * NC, ncols - sb * E);  // columns of the batch
#pragma unroll 1
                    for (int k = 0; k * 64 < nbatch; ++k) {
                        const int c = k * 64 + lane;
                        const int w = sb * E + c;
                        if (c < nbatch) {
                            int yi;
                            if (INPLACE) {
                                yi = ix[c];
                                if (yi < 0) continue;  // a diagonal column in op N: forward only
                            } else {
                                bool off;
                                yi = col_lookup(w, off);
                                if (!(opT || off)) continue;
                            }
                            if (flags & FLAG_GATHER) {  // one plain, coalesced store per column sum
                                ws[col_off + w] = park[c];
                                continue;
                            }
                            const T val = mul(alpha, park[c]);
                            const unsigned wi = (unsigned)(yi - wd.win_base);
                            if (wi < (unsigned)win_n) {
                                if (!BSM_DBG(DBG_NO_WINDOW_ADD)) lds_acc(&win[wi], val);  // leaves the CU once, with the window
                            } else if (flags & FLAG_RMW) {
                                y[yi] = add(y[yi], val);
                            } else if (!BSM_DBG(DBG_NO_GLOBAL_ATOMICS)) {
                                atomic_acc(&y[yi], val);
                            }
                        }
                    }
                }
            }
        };

        for (int c0 = 0; c0 < ncols; c0 += XCH) {
            stage_chunk(c0);
#ifdef BSM_TRACE
            if (c0 == 0) BSM_TSTAMP(2);  // x slice staged (loads issued and stored to LDS)
#endif
            const int s_end = min(nstrips, (c0 + XCH) / E);
            for (int s0 = c0 / E; s0 < s_end; s0 += G * L) {
                // (Software-pipelined variants -- two register buffers of L / 2 loads with the next
                // iteration's loads issued before the butterfly / emission of the current one and the
                // first ones before the x gather; every next iteration's loads already in flight; only a
                // chunk's first loads issued inside the x gather -- were measured on forward AND fused
                // kernels and lost every time (tiled BEM fixture, fused: ComplexF64 153 -> 160 us, fp64
                // 82 -> 117 us with 36 B of scratch): the memory system serves requests first come, first
                // served, occupancy provides the parallelism of a long launch, and the extra iterations
                // cost issue slots.)  Round 5, once more for the forward-only kernels with BRANCH-FREE loads (strip and
                // row clamped, so that hipcc counts the loads in flight exactly -- docs/experiments_r05.md): 108 VGPRs = 4
                // waves instead of 6; C2 9.5 -> 12.1 us, C4 slice 301 -> 358, 1 GB VBCRS 166-175 -> 173-191: a wave of one
                // iteration issues a second, redundant batch, and the waves lost cost more than the overlap gains.
                Vec16<S> b[L];
                // a wave about to request matrix bytes is served before its SIMD's other waves (which are in
                // their butterfly / FMA phases): +0.3-2 % on every operator, nothing it costs
                __builtin_amdgcn_s_setprio(3);
                load_b(b, s0);
                __builtin_amdgcn_s_setprio(0);
                iteration(b, s0, c0, s_end);
            }
        }
    }
    T a = acc[0];
    if (FWD) {
#pragma unroll
        for (int e = 1; e < E; ++e) a = add(a, acc[e]);
#pragma unroll
        for (int d = P; d < 64; d <<= 1) a = add(a, shx(a, d));
    }
    return a;
}

template <typename T, bool FWD, bool TRN> constexpr int kMixedWaves = (FWD && TRN && std::is_same<T, double>::value) ? 7 : 6;
// complex vectors under a real image (kCvec): resident waves per SIMD the instances are compiled for
#ifndef BSM_CVEC_WAVES
#define BSM_CVEC_WAVES 6
#endif

// Occupancy is what the small-panel (BEM-shaped) products live on: a small panel is a chain of
// dependent memory round trips, hidden only by other resident waves.
//   fp64 forward-only: capped at 80 VGPRs (>= 6 waves per SIMD = 1536 resident workgroups: every
//     workgroup of a C2-sized launch is resident at once); compiles to 78 (a cap of 72 = 7 waves
//     compiles to 70 without scratch and measures the same: C2, 1 GB VBCRS, BEM forward).
//   fp64 fused: capped at 64 VGPRs = 8 waves per SIMD, no scratch; with 20 KB of LDS per workgroup
//     exactly 8 workgroups fit a CU (+11-13 % on 3-28-row fp64 panels over 6 waves).
//   complex128: capped at 80 (the fused instance compiles to 71: 7 waves).
//   fp32 / complex64: capped at 96 = 5 waves (fp32 fused compiles to 80: 6), no scratch anywhere.
//   mixed precision (S = float / c64 stored under double / complex128 vectors, L = 4: bsm_plan.cpp): capped at 80
//     = 6 waves, the fp64 fused instance at 72 = 7 (a cap of 64 left 8 B of scratch; complex128 needs 72 + 8 B under
//     72).  No scratch anywhere.
template <typename T, int L, bool FWD, bool TRN, bool NT, typename S = T>
__global__ void __launch_bounds__(64 * kWavesPerWg) __attribute__((amdgpu_waves_per_eu(
    kCvec<T, S> ? BSM_CVEC_WAVES :
    !std::is_same<S, T>::value ? kMixedWaves<T, FWD, TRN> :
    (FWD && TRN && (std::is_same<T, double>::value || std::is_same<T, float>::value)) ? 8 :
    (FWD && TRN && std::is_same<T, c128>::value) ? (L == 4 ? 8 : BSM_C128_FUSED_WAVES) :
    (FWD && TRN && std::is_same<T, c64>::value) ? (L == 4 ? 8 : BSM_C64_FUSED_WAVES) :
    (((!TRN && std::is_same<T, double>::value) || std::is_same<T, c128>::value) ? 6 : 5))))
    // <= 96 SGPRs: a CU admits 7 workgroups of 256 threads (the ComplexF64 fused instance compiled to 106 =
    // 6 workgroups; tiled BEM fixture 147.7 -> 143.9 us with the cap, nothing else changes)
    __attribute__((amdgpu_num_sgpr(96)))
    panel_kernel(const WaveWork *__restrict__ waves, const uint4 *__restrict__ values, const int *__restrict__ rows,
                 const int *__restrict__ cols, const T *__restrict__ x, T *__restrict__ y, T alpha,
                 T beta, int flags, unsigned wg_base, T *__restrict__ ws, long long ws_fbase) {
    constexpr int XS = x_chunk_cols<T, TRN>();         // staged x slice per wave
    constexpr int VS = XS;                             // transposed column sums of one staged chunk
    __shared__ __attribute__((aligned(16))) T xs[kWavesPerWg][FWD ? XS : 1];
    __shared__ __attribute__((aligned(16))) T vs[kWavesPerWg][TRN ? VS : 1];
    // (the cross-wave combine slab of split groups aliases xs: a wave's x slice is dead by then)
    // y window of workgroups that pack neighbouring small row groups of a symmetric operator
    constexpr bool WIN = FWD && TRN;
    __shared__ T win[WIN ? window_entries((int)sizeof(T)) : 1];

    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int lane = threadIdx.x & 63;
    BSM_TSTAMP(0);  // wave started
    const WaveD wd = load_wave(waves + ((size_t)(blockIdx.x + wg_base) * kWavesPerWg + wave));
    const int work = wd.work;
    const int m = wd.m;
#ifdef BSM_TRACE
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
    BSM_TSTAMP(1);  // descriptor arrived
    if (lane == 0) {
        t_trace[threadIdx.x >> 6][6] =
            (unsigned long long)(wd.work == WORK_PANEL && wd.npieces ? (long long)wd.first.nstrips * wd.m * 16 : 0);
        t_trace[threadIdx.x >> 6][7] = wall_clock64();
        // where the wave runs (tools/placement_census.py): slot 9 = HW_ID (wave 3:0, SIMD 5:4, CU 11:8, SH 12, SE 15:13),
        // slot 10 = XCC_ID (XCD 3:0); plain register reads
        t_trace[threadIdx.x >> 6][9] = (unsigned long long)__builtin_amdgcn_s_getreg(BSM_GETREG_HW_ID);
        t_trace[threadIdx.x >> 6][10] = (unsigned long long)__builtin_amdgcn_s_getreg(BSM_GETREG_XCC_ID);
    }
#endif
    // workgroup-uniform (all 4 descriptors carry the same window; coloured launches keep plain RMW)
    int win_n = (WIN && !(flags & FLAG_RMW)) ? wd.win_n : 0;
    // complex vectors under a real image: the analysis cut the window at window_entries(sizeof(S)) entries, twice what
    // the 4 KB of `win` hold in T -- the window is clamped, and the y entries beyond it take the path of every entry
    // outside a window (global atomics)
    if constexpr (kCvec<T, S>) win_n = min(win_n, window_entries((int)sizeof(T)));
    if (WIN && win_n > 0) {
        for (int e = threadIdx.x; e < win_n; e += 64 * kWavesPerWg) win[e] = zero_of(T{});
        __syncthreads();
    }

    T u = zero_of(T{});
    if (work == WORK_PANEL) {
        if (m <= 8)
            u = run_panel<T, L, 8, FWD, TRN, NT, S>(wd, values, rows, cols, x, y, alpha, flags, lane, xs[wave], vs[wave], win, win_n, ws);
        else if (m <= 16)
            u = run_panel<T, L, 16, FWD, TRN, NT, S>(wd, values, rows, cols, x, y, alpha, flags, lane, xs[wave], vs[wave], win, win_n, ws);
        else if (m <= 32)
            u = run_panel<T, L, 32, FWD, TRN, NT, S>(wd, values, rows, cols, x, y, alpha, flags, lane, xs[wave], vs[wave], win, win_n, ws);
        else
            u = run_panel<T, L, 64, FWD, TRN, NT, S>(wd, values, rows, cols, x, y, alpha, flags, lane, xs[wave], vs[wave], win, win_n, ws);
    }
    BSM_TSTAMP(4);  // the wave's piece is streamed
    const bool direct = (flags & FLAG_DIRECT) != 0;
    const bool sz = (flags & FLAG_STRONG_ZERO) != 0;
    if (FWD) {
        if (wd.wg_sync) {  // workgroup-uniform: only groups split over several waves meet in LDS
            xs[wave][lane] = u;
            __syncthreads();
        }
        if (work == WORK_PANEL && wd.lead && !BSM_DBG(DBG_NO_FWD_OUT)) {
            for (int k = 1; k < wd.grp; ++k) u = add(u, xs[wave + k][lane]);
            if (flags & FLAG_GATHER) {
                // forward partial sums of this workgroup item: slots ws_fbase + win_base + row
                const bool fwd_on = !(flags & FLAG_OPT) || (wd.first.kind & kKindGroupHasOff);
                if (lane < m && fwd_on) ws[ws_fbase + wd.win_base + lane] = u;
            } else if (lane < m) {
                const int yi = row_index(wd, rows, lane);
                const T val = mul(alpha, u);
                const unsigned wi = (unsigned)(yi - wd.win_base);
                if (direct) {
                    y[yi] = sz ? val : madd(val, beta, y[yi]);
                } else if (wi < (unsigned)win_n) {
                    lds_acc(&win[wi], val);
                } else if (flags & FLAG_RMW) {
                    y[yi] = add(y[yi], val);
                } else {
                    atomic_acc(&y[yi], val);
                }
            }
        }
    }
    if (WIN && win_n > 0) {
        // every wave has parked its sums: the window leaves the CU once, 64 contiguous entries
        // per atomic wave-instruction
        __syncthreads();
        for (int e = threadIdx.x; e < win_n; e += 64 * kWavesPerWg) {
            const T v = win[e];
            if (!is_zero(v)) atomic_acc(&y[wd.win_base + e], v);
        }
    }
    if (work == WORK_SCALE && direct) {
        const int cnt = wd.first.ncols;
        for (int r = lane; r < cnt; r += 64)
            y[wd.rbase + r] = sz ? zero_of(T{}) : mul(beta, y[wd.rbase + r]);
    }
#ifdef BSM_TRACE
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    BSM_TSTAMP(5);  // everything stored
    if (lane == 0) t_trace[threadIdx.x >> 6][8] = wall_clock64();
    if (g_trace && lane < 16)
        g_trace[((size_t)blockIdx.x * kWavesPerWg + (threadIdx.x >> 6)) * 16 + lane] = t_trace[threadIdx.x >> 6][lane];
#endif
}

// y[lo .. hi) = beta * y  (or 0 for the strong zero) -- `y .*= beta`,
// reference src/blockmatrix.jl:231, src/symmetricblockmatrix.jl:392, src/vbcrs.jl:273,313.
// A streaming pass: one 16-byte unit per lane and step (the element-per-thread form took 5.6 us for the 1.6 MB
// of a C3-sized y under rocprofv3 -- 0.3 TB/s -- and is a launch of its own in front of every accumulate-mode
// product), the unaligned head and tail of the range element by element.
template <typename T>
__global__ void __launch_bounds__(256) scale_kernel(T *__restrict__ y, long long ldy, long long lo,
                                                    long long hi, T beta, int strong_zero) {
    constexpr int E = TT<T>::E;
    T *__restrict__ yc = y + (long long)blockIdx.y * ldy + lo;  // one grid row per right-hand side
    const long long n = hi - lo;
    const long long tid = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    const long long stride = (long long)gridDim.x * blockDim.x;
    // elements in front of the first 16-byte boundary
    const unsigned gap = (unsigned)((16 - ((uintptr_t)yc & 15)) & 15);
    if (gap % sizeof(T)) {  // (a complex vector on an 8-byte boundary only: no element count reaches a 16-byte one)
        for (long long i = tid; i < n; i += stride) yc[i] = strong_zero ? zero_of(T{}) : mul(beta, yc[i]);
        return;
    }
    long long head = (long long)(gap / sizeof(T));
    if (head > n) head = n;
    const long long nvec = (n - head) / E;
    Vec16<T> *__restrict__ yv = reinterpret_cast<Vec16<T> *>(yc + head);
    for (long long u = tid; u < nvec; u += stride) {
        Vec16<T> v;
        if (strong_zero) {
#pragma unroll
            for (int e = 0; e < E; ++e) v.v[e] = zero_of(T{});
        } else {
            v = yv[u];
#pragma unroll
            for (int e = 0; e < E; ++e) v.v[e] = mul(beta, v.v[e]);
        }
        yv[u] = v;
    }
    const long long tail0 = head + nvec * E;
    if (tid < head) yc[tid] = strong_zero ? zero_of(T{}) : mul(beta, yc[tid]);
    if (tid < n - tail0) yc[tail0 + tid] = strong_zero ? zero_of(T{}) : mul(beta, yc[tail0 + tid]);
}
// grid of the pass over n elements: one 16-byte unit per thread, at most 2048 workgroups
template <typename T> static unsigned scale_blocks(long long n) {
    long long nblk = (n / TT<T>::E + 255) / 256 + 1;
    return (unsigned)(nblk > 2048 ? 2048 : nblk);
}

// second launch of the gather mode: y[j] = beta*y[j] + alpha * (sum of the workspace slots that
// contribute to j, in their fixed ascending order).  Outside the owned range only rows that
// receive contributions are touched (and not scaled), like the atomic path.
template <typename T>
__global__ void __launch_bounds__(256)
    gather_kernel(T *__restrict__ y, long long ylen, long long own_lo, long long own_hi,
                  const long long *__restrict__ ptr, const int *__restrict__ idx, const T *__restrict__ ws,
                  T alpha, T beta, int strong_zero) {
    const long long j = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (j >= ylen) return;
    // ELL per 64-row tile: line l holds the l-th contribution of each row of the tile (-1: none)
    const long long t = j >> 6;
    const int lane = (int)(j & 63);
    const long long a = ptr[t], b = ptr[t + 1];
    T s = zero_of(T{});
    bool any = false;
    for (long long l = a; l < b; ++l) {
        const int slot = idx[l * 64 + lane];
        if (slot >= 0) {
            s = add(s, ws[slot]);
            any = true;
        }
    }
    const T val = mul(alpha, s);
    if (j >= own_lo && j < own_hi)
        y[j] = strong_zero ? val : madd(val, beta, y[j]);
    else if (any)
        y[j] = add(y[j], val);
}

// one right-hand side (S: the stored type of the image)
template <typename T, int L, typename S>
static hipError_t launch_typed(const Product &p) {
    const DeviceImage &img = p.img;
    const bool opT = p.opT;
    const int strong_zero = p.strong_zero;
    hipStream_t stream = p.stream;
    const T *xd = (const T *)p.x;
    T *yd = (T *)p.y;
    const T alpha = load_scalar<T>(p.alpha, 1.0), beta = load_scalar<T>(p.beta, 0.0);
    int flags = base_flags(opT, p.conj, strong_zero);
    const uint4 *values = (const uint4 *)img.d_values;
    const int *rows = (const int *)img.d_rows;
    const int *cols = (const int *)img.d_cols;
    const bool nt = stream_policy(img);
    T *ws = nullptr;  // gather mode: the workspace
    // one launch of panel_kernel<T, L, FWD, TRN, NT, S> with NT taken from the run-time policy `nt`
    auto panel = [&](auto fwd, auto trn, const WaveWork *waves, dim3 grid, unsigned wg_base) {
        constexpr bool FWD = decltype(fwd)::value, TRN = decltype(trn)::value;
        const dim3 block(64 * kWavesPerWg);
        if (nt)
            hipLaunchKernelGGL((panel_kernel<T, L, FWD, TRN, true, S>), grid, block, 0, stream, waves, values, rows, cols, xd,
                               yd, alpha, beta, flags, wg_base, ws, img.ws_fbase);
        else
            hipLaunchKernelGGL((panel_kernel<T, L, FWD, TRN, false, S>), grid, block, 0, stream, waves, values, rows, cols, xd,
                               yd, alpha, beta, flags, wg_base, ws, img.ws_fbase);
    };
    if (!opT && img.exclusive_fwd) {
        // one launch: every y row has exactly one producer; beta is fused into its store and
        // the rows no block covers are scaled by WORK_SCALE waves of the same grid.
        flags |= FLAG_DIRECT;
        if (img.nwg_total > 0)
            panel(std::true_type{}, std::false_type{}, (const WaveWork *)img.d_waves, dim3((unsigned)img.nwg_total), 0u);
        return hipGetLastError();
    }
    // accumulate mode: y .*= beta over the owned range, then hardware atomics (gather mode: the sums go to the
    // workspace, and a second launch adds them up in a fixed order)
    const YRange r = y_range(img, opT, p.zrange);
    // (complex vectors under a real image: the complex workspace, twice the bytes, allocated at the first such product)
    void *wsp = kCvec<T, S> ? img.d_wsc : img.d_ws;
    const bool gather = p.use_gather && wsp != nullptr;
    if (gather) {
        ws = (T *)wsp;
        flags |= FLAG_GATHER;
    }
    if (!gather && r.hi > r.lo && (strong_zero || !is_one(beta)))
        launch_scale(p.vt, yd, 0LL, r.lo, r.hi, &beta, strong_zero, 1u, stream);
    if (!img.color_wg_ptr.empty()) flags |= FLAG_RMW;
    for_each_launch(img, false, [&](const WaveWork *waves, dim3 grid, unsigned wg_base) {
        with_halves(opT, img.has_off, [&](auto fwd, auto trn) { panel(fwd, trn, waves, grid, wg_base); });
    });
    const long long ylen = opT ? img.ncols : img.nrows;
    if (gather && ylen > 0) {
        const int k = opT ? 1 : 0;
        const long long nblk = (ylen + 255) / 256;
        hipLaunchKernelGGL((gather_kernel<T>), dim3((unsigned)nblk), dim3(256), 0, stream, yd, ylen, r.lo, r.hi,
                           (const long long *)img.d_inv_ptr[k], (const int *)img.d_inv_idx[k], (const T *)ws,
                           alpha, beta, strong_zero);
    }
    return hipGetLastError();
}

// the instance of a ONE batch: L loads per lane in flight, 8 where the plan says so (bsm_plan.cpp: one_column), else the
// pair's own -- 4 for mixed storage and complex vectors under a real image
hipError_t launch_one(const Product &p, const Batch &b) {
    return with_pair(p.img.dtype, p.vt, [&](auto t, auto s) {
        using T = decltype(t);
        using S = decltype(s);
        constexpr bool SAME = std::is_same<S, T>::value;
        constexpr int LF = !SAME ? 4 : std::is_same<T, float>::value ? BSM_F32_L : std::is_same<T, double>::value ? BSM_F64_L
                         : std::is_same<T, c64>::value ? BSM_C64_L : BSM_C128_L;
        if constexpr (SAME && LF != 8)
            if (b.L == 8) return launch_typed<T, 8, S>(p);
        return launch_typed<T, LF, S>(p);
    });
}

void launch_scale(int vt, void *y, long long ldy, long long lo, long long hi, const void *beta, int strong_zero, unsigned ncols,
                  hipStream_t stream) {
    (void)with_pair(vt, vt, [&](auto t, auto) {  // (the same-type pair of vt: its T)
        using T = decltype(t);
        hipLaunchKernelGGL((scale_kernel<T>), dim3(scale_blocks<T>(hi - lo), ncols), dim3(256), 0, stream, (T *)y, ldy, lo, hi,
                           *(const T *)beta, strong_zero);
        return hipSuccess;
    });
}

#ifdef BSM_TRACE
hipError_t set_trace_one(void *buf) { return set_trace_here(buf); }
#endif

}  // namespace bsm
