// bsm_il.hip -- the interleaved multi-RHS pass: il_pack_kernel, panel_kernel_il (il_panel), il_finish_kernel.
#include "bsm_device.h"
#include "bsm_families.h"

namespace bsm {

// ----------------------------------------------------------------------------------------
// INTERLEAVED multi-RHS pass (round 5): 8 ComplexF64 right-hand sides with X and the accumulated Y held ROW-major
// ("K-interleaved") in two work arrays of the handle:
//     Xr[i][c], W[i][c],  c = 2 k + (0: Re, 1: Im),  16 doubles = ONE 128-byte line per vector index
// Xr = alpha * X is written by il_pack_kernel in front of the pass, Y = beta * Y + W is read back (and W zeroed behind)
// by il_finish_kernel.  What it changes against panel_kernel_multi's matrix-pipe path (counters of round 4: 9.7 M atomic
// line requests and 11.6 M read requests per BEM launch, the vector L1 stalled on pending requests 87 % of the time):
//   * the x operand of an MFMA (component on lane % 16) is ONE coalesced 128-byte line per column / row index, loaded
//     straight from Xr into the operand register -- no K-fold gather of column-major X, no x slice in LDS (32 KB per
//     workgroup: 3 workgroups per CU), no dependent "column list -> x gather -> LDS" round trips per 64 columns;
//   * both halves are computed with the COMPONENT on the lane (A = the matrix tile, B = the x lines), so a sum leaves as
//     16 consecutive doubles of one line of W: 4 lines per atomic wave-instruction whatever the column list looks like
//     (column-major Y: one line per (index, k) -- 16-32 per instruction for the scattered lists of a BEM panel);
//   * the whole column list of a panel (<= 256 columns per refill) is staged once, so a wave's start is descriptor ->
//     {row list -> x rows, column list, first tile}: three round trips for the whole panel.
// One step = one row block (16 rows) of one column tile (16 columns), operands one step ahead, as in the path above.
// ----------------------------------------------------------------------------------------
// resident workgroups per CU the interleaved kernels are compiled for (their natural register need, fused instances --
// panels of at most 32 rows, two row blocks, one step ahead: Float32 / ComplexF32 84-92 VGPRs, Float64 110, ComplexF64 144;
// tall panels, four row blocks of the next 16 columns in flight: Float32 128, ComplexF32 145, Float64 184, ComplexF64 231)
#ifndef BSM_IL_C128_WGS
#define BSM_IL_C128_WGS 3
#endif
// mixed storage (ILMixed<S>: values stored as S = float / c64, arithmetic in double): the accumulators, x operands and
// row operands of the Float64 / ComplexF64 instances beside half their tile registers -- compiled for the same number
// of resident workgroups as those (docs/experiments_r09.md has the register table)
template <typename S> struct ILMixed {};
template <typename T, int MRMAX> constexpr int il_wgs() {
    if constexpr (std::is_same<T, ILMixed<float>>::value) return il_wgs<double, MRMAX>();
    if constexpr (std::is_same<T, ILMixed<c64>>::value) return il_wgs<c128, MRMAX>();
    constexpr bool f64 = std::is_same<T, double>::value;
    if (MRMAX > 2) return sizeof(T) == 4 ? 4 : (sizeof(T) == 16 || f64 ? 2 : 3);
    return sizeof(T) == 16 ? BSM_IL_C128_WGS : (f64 ? 4 : 5);
}
constexpr int kIlCols = 256;            // columns of a panel staged per refill of the index list
constexpr int IL_NOFWD = 1 << 30;       // staged column entry: takes no part in the forward half
constexpr int IL_NOTRN = (int)(1u << 31);  // ... in the transposed half
constexpr int IL_MASK = (1 << 30) - 1;

// The loop is written BRANCH-FREE on purpose.  hipcc places its own s_waitcnt in front of the first use of every loaded
// register, and wherever control flow (a lane-masked `if` around a load or an atomic, a scratch reload, paths with different
// numbers of memory operations) keeps it from counting the operations in flight exactly it waits for ALL of them:
// the first version of this kernel -- loads and atomics under `if (row < m && w < ncols)` -- compiled to a
// `s_waitcnt vmcnt(0)` in front of every step's MFMAs, i.e. the operands requested one step ahead were drained at once
// and every step cost a full memory round trip (tools/il_trace.py: 3.5 us per step, 35 us per 19 KB panel).  Here every
// load and every atomic of the loop is issued unconditionally, with indices clamped into the panel (rows >= m read row
// m - 1, columns >= ncols the last column) and the VALUES masked instead: rows beyond m meet x rows that are zero and
// their forward sums are never delivered, columns beyond the panel get a zero x operand and deliver +0.0.  One body per
// number of row blocks (NRB), so that a step is the same instruction sequence every time.
// atomic add of the lanes with `ok`, WITHOUT control flow: the other lanes are switched off for the one instruction
// (EXEC), not branched around -- a lane-masked `if` around an atomic becomes a branch, and hipcc then no longer knows how
// many operations are in flight behind it (above).  Masked lanes must not be routed to a dummy target instead: lanes of
// one instruction that add to the SAME address are serialised on the memory side (measured with +0.0 deliveries to a
// clamped index: the atomics of the BEM pass went from 30 to 390 us).  hipcc does not count the instruction either; it is
// always issued IN FRONT of the step's loads, so every wait it computes for those is still sufficient.
__device__ __forceinline__ void il_atomic_add(double *p, double v, bool ok) {
    unsigned long long save;
    const int flag = ok ? 1 : 0;
    asm volatile(
        "s_mov_b64 %0, exec\n\t"
        "v_cmpx_ne_u32_e32 0, %1\n\t"
        "global_atomic_add_f64 %2, %3, off\n\t"
        "s_mov_b64 exec, %0"
        : "=&s"(save)
        : "v"(flag), "v"(p), "v"(v)
        : "vcc", "memory");
}
__device__ __forceinline__ void il_atomic_add(float *p, float v, bool ok) {
    unsigned long long save;
    const int flag = ok ? 1 : 0;
    asm volatile(
        "s_mov_b64 %0, exec\n\t"
        "v_cmpx_ne_u32_e32 0, %1\n\t"
        "global_atomic_add_f32 %2, %3, off\n\t"
        "s_mov_b64 exec, %0"
        : "=&s"(save)
        : "v"(flag), "v"(p), "v"(v)
        : "vcc", "memory");
}

// The four element types of the interleaved pass: 16 real COMPONENTS per vector index -- 8 complex right-hand sides
// (component 2 k + Re / Im) or 16 real ones -- of type R, one N = 16 of v_mfma_{f64,f32}_16x16x4.  A 16-byte load holds E
// columns of one row; a step (16 rows x 16 columns) is NLD = 4 / E loads per lane (lane = row ln, strip 4 j + lk).
// S: the type the image stores, TL: the element type of the LDS tile of the transposed half.  ILMixed<float> /
// ILMixed<c64> (mixed storage): the loads hold S, E = 4 / 2 columns per load; a value is widened to double (exact) where
// it enters the f64 MFMA of the forward half and where it is stored into the tile (TL = double / c128: the conversion
// then is off the LDS read -> MFMA chain of the transposed half; against a tile kept in S, C3 x 8 192 -> 185 us, tiled
// BEM complex x 4 279 -> 270, x 16 +-0 / +1.4 %, docs/experiments_r09.md), and everything behind that -- accumulators,
// Xr, W, the atomics, the accumulator-row map -- is the Float64 / ComplexF64 instance's.
template <typename T> struct ILT;
template <> struct ILT<c128> { using R = double; using V4 = v4f64; using S = c128; using TL = c128; static constexpr bool CPLX = true; static constexpr int KK = 8; };
template <> struct ILT<double> { using R = double; using V4 = v4f64; using S = double; using TL = double; static constexpr bool CPLX = false; static constexpr int KK = 16; };
template <> struct ILT<c64> { using R = float; using V4 = v4f32; using S = c64; using TL = c64; static constexpr bool CPLX = true; static constexpr int KK = 8; };
template <> struct ILT<float> { using R = float; using V4 = v4f32; using S = float; using TL = float; static constexpr bool CPLX = false; static constexpr int KK = 16; };
template <> struct ILT<ILMixed<c64>> { using R = double; using V4 = v4f64; using S = c64; using TL = c128; static constexpr bool CPLX = true; static constexpr int KK = 8; };
template <> struct ILT<ILMixed<float>> { using R = double; using V4 = v4f64; using S = float; using TL = double; static constexpr bool CPLX = false; static constexpr int KK = 16; };
__device__ __forceinline__ double il_re(const c128 &a) { return a.re; }
__device__ __forceinline__ double il_im(const c128 &a) { return a.im; }
__device__ __forceinline__ float il_re(const c64 &a) { return a.re; }
__device__ __forceinline__ float il_im(const c64 &a) { return a.im; }
__device__ __forceinline__ double il_re(double a) { return a; }
__device__ __forceinline__ double il_im(double) { return 0.0; }
__device__ __forceinline__ float il_re(float a) { return a; }
__device__ __forceinline__ float il_im(float) { return 0.f; }

// CS = components stored per vector index: 16, or 8 for real types with at most 8 right-hand sides (half a tile of the
// MFMA stays empty -- lanes ln >= 8 carry a zero x operand and deliver nothing -- but a vector index is 64 bytes of Xr and
// of W instead of 128: what bounds this pass over short panels is its vector-side traffic, not the matrix pipe)
// DEEP (instances for tall panels, MRMAX = 4): the tiles of ALL NRB row blocks of the next 16 columns are requested
// while the current ones are consumed (each buffer re-requested in place right behind its last use) instead of one step
// ahead -- with one 16 x 16 tile per wave in flight a pass over 64-row panels is bound by tile latency x resident waves
// (fp64: 12 waves per CU x 2 KB per 1.8 us = 3.5 TB/s, matrix pipe half idle).
template <typename T, int NRB, bool FWD, bool TRN, int CS, bool DEEP>
__device__ __forceinline__ void il_panel(const WaveD &wd, const uint4 *__restrict__ values, const int *__restrict__ rows,
                                         const int *__restrict__ cols, const typename ILT<T>::R *__restrict__ xr,
                                         typename ILT<T>::R *__restrict__ wacc, int flags, int lane, typename ILT<T>::TL *tile,
                                         int *cix) {
    using R = typename ILT<T>::R;
    using V4 = typename ILT<T>::V4;
    using S = typename ILT<T>::S;  // the stored type (= T unless mixed storage)
    using TL = typename ILT<T>::TL;
    constexpr bool CPLX = ILT<T>::CPLX;
    constexpr bool F64MAP = sizeof(R) == 8;  // accumulator rows: lk + 4 r (f64) / 4 lk + r (f32)
    constexpr int E = TT<S>::E;
    constexpr int NLD = 4 / E;
    const bool opT = (flags & FLAG_OPT) != 0;
    const bool cjf = (flags & FLAG_CONJ) != 0;
    const int m = wd.m;
    const int ln = lane & 15, lk = lane >> 4;
    const int lc = CS == 16 ? ln : min(ln, CS - 1);  // the component this lane addresses
    const bool live = CS == 16 || ln < CS;           // ... and whether it carries one at all
    const PieceD pc = wd.first;
    const int xbase = pc.xbase, col_off = pc.col_off, ncols = pc.ncols, nstrips = pc.nstrips, kinds = pc.kind;
    const bool has_off = (kinds & kKindHasOff) != 0;
    const bool fwd_en = FWD && (!opT || has_off);
    const bool trn_en = TRN && (opT || has_off);
    const Vec16<S> *__restrict__ vb = reinterpret_cast<const Vec16<S> *>(values + (((uint64_t)pc.val_hi << 32) | pc.val_lo));
    const ColMap cm = col_map(wd, pc);
    // complex: the sign of X'' = i X (conj(B): -i X) on this lane: component 2 k takes -Im, component 2 k + 1 takes +Re
    const bool neg2 = ((ln & 1) == 0) != cjf;
    auto second = [&](R v1) {
        const R v2 = dppx<DPP_QUAD_XOR1>(v1);
        return neg2 ? -v2 : v2;
    };
    auto mfma = [&](R a, R b, V4 c) { return mfma16(a, b, c); };
    auto accrow = [&](int r) { return F64MAP ? lk + 4 * r : 4 * lk + r; };  // accumulator register r of this lane -> row of D
    // matrix operand of step (t0, rb): lane = (row rb * 16 + ln, strip t0 / E + 4 j + lk), indices clamped into the panel
    // (the last strip of a panel is zero-padded to E columns)
    auto mat = [&](int t0, int rb, int j) -> Vec16<S> {
        const int sidx = min(t0 / E + 4 * j + lk, nstrips - 1);
        const int row = min(rb * 16 + ln, m - 1);
        if (BSM_DBG(DBG_NO_MATRIX)) return Vec16<S>{};
        return load_stream16(&vb[(uint32_t)(sidx * m + row)]);
    };
    // ---- first batch of requests: the column list of the first block, the row list, the first tile -- all need the
    // descriptor only
    int craw[kIlCols / 64];
    const int nq0 = (min(ncols, kIlCols) + 63) >> 6;  // (wave-uniform)
#pragma unroll
    for (int q = 0; q < kIlCols / 64; ++q) {
        craw[q] = 0;
        if (xbase < 0 && q < nq0) craw[q] = cols[col_off + min(q * 64 + lane, ncols - 1)];
    }
    // rows 4 q + lk (the k index of the transposed half's MFMA q) and, where the accumulator map differs, the rows the
    // forward sums of this lane belong to
    int ri[4 * NRB], ro[F64MAP ? 1 : 4 * NRB];
#pragma unroll
    for (int q = 0; q < 4 * NRB; ++q) {
        ri[q] = wd.rbase + min(4 * q + lk, m - 1);
        if (!F64MAP) ro[q] = wd.rbase + min((q >> 2) * 16 + accrow(q & 3), m - 1);
    }
    if (wd.rbase < 0) {  // (wave-uniform)
#pragma unroll
        for (int q = 0; q < 4 * NRB; ++q) {
            ri[q] = rows[wd.row_off + min(4 * q + lk, m - 1)];
            if (!F64MAP) ro[q] = rows[wd.row_off + min((q >> 2) * 16 + accrow(q & 3), m - 1)];
        }
    }
    constexpr int NBUF = DEEP ? NRB : 1;
    Vec16<S> nb[NBUF][NLD];
#pragma unroll
    for (int rb = 0; rb < NBUF; ++rb)
#pragma unroll
        for (int j = 0; j < NLD; ++j) nb[rb][j] = mat(0, rb, j);
    // x / y index of panel column w with its roles (IL_NOFWD / IL_NOTRN)
    auto entry = [&](int w, int raw) -> int {
        bool off;
        const int xi = col_decode(cm, w, raw, off);
        return xi | ((!opT || off) ? 0 : IL_NOFWD) | ((opT || off) ? 0 : IL_NOTRN);
    };
    // ---- second batch: the x rows of the panel (operand of the transposed half), one line of Xr per row
    R rr[4 * NRB];
#pragma unroll
    for (int q = 0; q < 4 * NRB; ++q) rr[q] = (TRN && !BSM_DBG(DBG_NO_XGATHER)) ? xr[(size_t)ri[q] * CS + lc] : R(0);
    V4 facc[NRB];
#pragma unroll
    for (int rb = 0; rb < NRB; ++rb) facc[rb] = V4{0, 0, 0, 0};
    R pd[4] = {0, 0, 0, 0};
    int pe[4] = {0, 0, 0, 0};
    bool pok[4] = {false, false, false, false};
    auto emit = [&]() {
        if (BSM_DBG(DBG_NO_GLOBAL_ATOMICS)) return;
#pragma unroll
        for (int r = 0; r < 4; ++r) il_atomic_add(&wacc[(size_t)pe[r] * CS + lc], pd[r], pok[r]);
    };
    for (int cb = 0; cb < ncols; cb += kIlCols) {
        const int c_end = min(ncols, cb + kIlCols);
        // (re)fill the staged index list of [cb, c_end)
        const int nq = (c_end - cb + 63) >> 6;
        if (cb > 0) {
#pragma unroll
            for (int q = 0; q < kIlCols / 64; ++q)
                if (xbase < 0 && q < nq) craw[q] = cols[col_off + min(cb + q * 64 + lane, ncols - 1)];
        }
#pragma unroll
        for (int q = 0; q < kIlCols / 64; ++q)
            if (q < nq) cix[q * 64 + lane] = entry(min(cb + q * 64 + lane, ncols - 1), craw[q]);
        // entry of column w of this block (clamped into it)
        auto ent = [&](int w) { return cix[min(w, c_end - 1) - cb]; };
        // x operand of load j, column e of its strip: lane (component ln, column t0 + E (4 j + lk) + e)
        auto xop = [&](int t0, int j, int e) -> R {
            if (!FWD || BSM_DBG(DBG_NO_XGATHER)) return R(0);
            return xr[(size_t)(ent(t0 + E * (4 * j + lk) + e) & IL_MASK) * CS + lc];
        };
        if (cb == 0) {
#ifdef BSM_TRACE
            asm volatile("s_waitcnt vmcnt(0) lgkmcnt(0)" ::: "memory");
            BSM_TSTAMP(2);  // lists, x rows and the first tile are there
#endif
#pragma unroll
            for (int q = 0; q < 4 * NRB; ++q) rr[q] = (trn_en && live && 4 * q + lk < m) ? rr[q] : R(0);
        }
        R xn[4];
#pragma unroll
        for (int j = 0; j < NLD; ++j)
#pragma unroll
            for (int e = 0; e < E; ++e) xn[j * E + e] = xop(cb, j, e);
#ifdef BSM_TRACE
        if (cb == 0) {
            asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
            BSM_TSTAMP(3);  // first x operands arrived
        }
#endif
        for (int t0 = cb; t0 < c_end; t0 += 16) {
            // this tile's x operand (requested one tile ago), masked: columns beyond the block / without a forward role
            R xq[4];
#pragma unroll
            for (int je = 0; je < 4; ++je) {
                const int w = t0 + E * (4 * (je / E) + lk) + (je % E);
                const int en = ent(w);  // (read unconditionally: a short-circuit around an LDS read is a branch)
                const bool ok = fwd_en & live & (w < c_end) & ((en & IL_NOFWD) == 0);
                xq[je] = ok ? xn[je] : R(0);
            }
            // the PREVIOUS tile's sums first (vector-memory operations retire in order: they have the whole step, and the
            // latency of the requests behind them, to complete), then the next tile's operands
            emit();
            // (DEEP: everything this tile needs was requested a tile ago; hipcc does not count the atomics above and
            // drains what is in flight at the first use behind them -- so the new requests go out behind that use)
            if (!DEEP) {
#pragma unroll
                for (int j = 0; j < NLD; ++j)
#pragma unroll
                    for (int e = 0; e < E; ++e) xn[j * E + e] = xop(t0 + 16, j, e);
            }
            V4 dt = {0, 0, 0, 0};
#pragma unroll
            for (int rb = 0; rb < NRB; ++rb) {
                Vec16<S> b[NLD];
#pragma unroll
                for (int j = 0; j < NLD; ++j) b[j] = nb[DEEP ? rb : 0][j];
                // the next step's tile: the next row block of these columns, or the first one of the next 16 columns
                if (!DEEP) {
#pragma unroll
                    for (int j = 0; j < NLD; ++j) nb[0][j] = (rb + 1 < NRB) ? mat(t0, rb + 1, j) : mat(t0 + 16, 0, j);
                }
                if (FWD && !BSM_DBG(DBG_NO_FWD_HALF)) {
#pragma unroll
                    for (int j = 0; j < NLD; ++j)
#pragma unroll
                        for (int e = 0; e < E; ++e) {
                            const R x1 = xq[j * E + e];
                            facc[rb] = mfma(il_re(b[j].v[e]), x1, facc[rb]);
                            if (CPLX) facc[rb] = mfma(il_im(b[j].v[e]), second(x1), facc[rb]);
                        }
                }
                if (TRN && !BSM_DBG(DBG_NO_TRN_HALF)) {
#pragma unroll
                    for (int j = 0; j < NLD; ++j)
#pragma unroll
                        for (int e = 0; e < E; ++e) {
                            if constexpr (std::is_same<TL, S>::value)
                                tile[(E * (4 * j + lk) + e) * 17 + ln] = b[j].v[e];
                            else
                                tile[(E * (4 * j + lk) + e) * 17 + ln] = widen(TL{}, b[j].v[e]);
                        }
                }
                if (DEEP) {  // this row block's tile of the next 16 columns, into the registers just consumed
                    if (rb == 0) {
#pragma unroll
                        for (int j = 0; j < NLD; ++j)
#pragma unroll
                            for (int e = 0; e < E; ++e) xn[j * E + e] = xop(t0 + 16, j, e);
                    }
#pragma unroll
                    for (int j = 0; j < NLD; ++j) nb[rb][j] = mat(t0 + 16, rb, j);
                }
                if (TRN && !BSM_DBG(DBG_NO_TRN_HALF)) {
#pragma unroll
                    for (int q = 0; q < 4; ++q) {
                        const TL u = tile[ln * 17 + 4 * q + lk];
                        const R r1 = rr[rb * 4 + q];
                        dt = mfma(il_re(u), r1, dt);
                        if (CPLX) dt = mfma(il_im(u), second(r1), dt);
                    }
                }
            }
            // lane (component ln, lk), register r: the sums of column t0 + accrow(r): parked until the next step
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int w = t0 + accrow(r);
                const int en = ent(w);
                pe[r] = en & IL_MASK;
                pd[r] = dt[r];
                pok[r] = trn_en & live & (w < c_end) & ((en & IL_NOTRN) == 0);
            }
        }
    }
#ifdef BSM_TRACE
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    BSM_TSTAMP(4);  // every tile done
#endif
    emit();
    if (fwd_en && !BSM_DBG(DBG_NO_FWD_OUT)) {
        // lane (component ln, lk), register r of row block rb: row rb * 16 + accrow(r) -- every wave adds its own partial sums
#pragma unroll
        for (int rb = 0; rb < NRB; ++rb)
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int row = rb * 16 + accrow(r);
                const int yi = F64MAP ? ri[4 * rb + r] : ro[4 * rb + r];  // (f64 map: row = 4 q + lk for q = 4 rb + r)
                il_atomic_add(&wacc[(size_t)yi * CS + lc], facc[rb][r], live & (row < m));
            }
    }
}

// (one wave per workgroup -- the waves of this pass share nothing, and a workgroup's slot is only recycled when its
// SLOWEST wave is done: tools/il_trace.py showed 66 % of the wave slots occupied -- was measured at +-0 and removed)
template <typename T, int MRMAX, bool FWD, bool TRN, int CS>
__global__ void __launch_bounds__(64 * kWavesPerWg, (il_wgs<T, MRMAX>()))
    panel_kernel_il(const WaveWork *__restrict__ waves, const uint4 *__restrict__ values, const int *__restrict__ rows,
                    const int *__restrict__ cols, const typename ILT<T>::R *__restrict__ xr, typename ILT<T>::R *__restrict__ wacc,
                    int flags, unsigned wg_base, unsigned xcd_run) {
    constexpr int WPW = kWavesPerWg;
    constexpr bool DEEP = MRMAX > 2;  // tall panels: all row blocks of the next 16 columns in flight (il_panel)
    __shared__ typename ILT<T>::TL tl[WPW][TRN ? 16 * 17 : 1];
    __shared__ int cixs[WPW][kIlCols];
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int lane = threadIdx.x & 63;
    BSM_TSTAMP(0);  // wave started
    // XCD-aware order (xcd_run > 0): workgroups are dealt to the 8 XCDs round robin, so with the plain order eight
    // NEIGHBOURING panels -- which read mostly the same lines of Xr -- land in eight different L2s.  Here every XCD takes
    // RUNS of xcd_run consecutive workgroups of the list (8 * xcd_run workgroups = one run per XCD), so neighbours share
    // an L2 while the list is still consumed front to back on all XCDs (its heavy items come first: a contiguous eighth
    // per XCD, the first form of this, left XCD 0 with all of them -- C5 slice x 8 967 -> 1252 us).
    unsigned bid = blockIdx.x;
    if (xcd_run) {  // (the launcher pads the grid to a multiple of 8 * xcd_run; surplus blocks leave at once)
        const unsigned span = 8u * xcd_run, in = bid % span;
        bid = bid - in + (in & 7u) * xcd_run + (in >> 3);
    }
    if (bid >= wg_base) return;  // wg_base: number of workgroups of the record list (re-used argument)
    const WaveD wd = load_wave(waves + ((size_t)bid * WPW + wave));
    if (wd.work != WORK_PANEL || wd.npieces <= 0 || wd.first.ncols <= 0 || wd.m <= 0) return;
#ifdef BSM_TRACE
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
    BSM_TSTAMP(1);  // descriptor arrived
    if (lane == 0) {
        t_trace[threadIdx.x >> 6][6] = (unsigned long long)((long long)wd.first.ncols * 65536 + wd.m);
        t_trace[threadIdx.x >> 6][7] = wall_clock64();
    }
#endif
    const int nrb = (wd.m + 15) >> 4;  // (wave-uniform)
    if (nrb == 1)
        il_panel<T, 1, FWD, TRN, CS, DEEP>(wd, values, rows, cols, xr, wacc, flags, lane, tl[wave], cixs[wave]);
    else if (nrb == 2 || MRMAX <= 2)
        il_panel<T, 2, FWD, TRN, CS, DEEP>(wd, values, rows, cols, xr, wacc, flags, lane, tl[wave], cixs[wave]);
    else if (nrb == 3)
        il_panel<T, (MRMAX > 2 ? 3 : 2), FWD, TRN, CS, DEEP>(wd, values, rows, cols, xr, wacc, flags, lane, tl[wave], cixs[wave]);
    else
        il_panel<T, (MRMAX > 2 ? 4 : 2), FWD, TRN, CS, DEEP>(wd, values, rows, cols, xr, wacc, flags, lane, tl[wave], cixs[wave]);
#ifdef BSM_TRACE
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    BSM_TSTAMP(5);  // everything stored
    if (lane == 0) t_trace[threadIdx.x >> 6][8] = wall_clock64();
    if (g_trace && lane < 16)
        g_trace[((size_t)blockIdx.x * WPW + (threadIdx.x >> 6)) * 16 + lane] = t_trace[threadIdx.x >> 6][lane];
#endif
}

// Xr[i][k] = alpha * X[i + kc(k) * ldx], k < KK (k >= kact: the last active column again, as the padded passes read it):
// 256 rows per workgroup, read down the columns of X, written along the lines of Xr (LDS transposition, row stride KK + 1)
template <typename T, int KK>
__global__ void __launch_bounds__(256) il_pack_kernel(const T *__restrict__ x, long long ldx, long long n, T alpha, int kact,
                                                      T *__restrict__ xr) {
    __shared__ T s[256 * (KK + 1)];
    const long long r0 = (long long)blockIdx.x * 256;
    const int t = threadIdx.x;
    if (r0 + t < n) {
#pragma unroll
        for (int k = 0; k < KK; ++k) s[t * (KK + 1) + k] = mul(alpha, x[r0 + t + (long long)(k < kact ? k : kact - 1) * ldx]);
    }
    __syncthreads();
    const long long cnt = (n - r0 < 256 ? n - r0 : 256) * KK;
#pragma unroll
    for (int j = 0; j < KK; ++j) {
        const int idx = j * 256 + t;
        if (idx < cnt) xr[r0 * KK + idx] = s[(idx / KK) * (KK + 1) + (idx % KK)];
    }
}
// Y[i + k * ldy] = (strong zero ? 0 : beta * Y) + W[i][k] for i in [lo, hi), k < kact;  W[i][:] = 0 behind the read
template <typename T, int KK>
__global__ void __launch_bounds__(256) il_finish_kernel(T *__restrict__ y, long long ldy, long long lo, long long hi, T beta,
                                                        int strong_zero, int kact, T *__restrict__ wacc) {
    __shared__ T s[256 * (KK + 1)];
    const long long r0 = lo + (long long)blockIdx.x * 256;
    const int t = threadIdx.x;
    const long long cnt = (hi - r0 < 256 ? hi - r0 : 256) * KK;
#pragma unroll
    for (int j = 0; j < KK; ++j) {
        const int idx = j * 256 + t;
        if (idx < cnt) {
            s[(idx / KK) * (KK + 1) + (idx % KK)] = wacc[r0 * KK + idx];
            wacc[r0 * KK + idx] = zero_of(T{});
        }
    }
    __syncthreads();
    if (r0 + t < hi) {
        for (int k = 0; k < kact; ++k) {
            T *yp = &y[r0 + t + (long long)k * ldy];
            const T v = s[t * (KK + 1) + k];
            *yp = strong_zero ? v : madd(v, beta, *yp);
        }
    }
}

// ---- the interleaved pass (panel_kernel_il) -- b: its batch (bsm_plan.h: columns, row-block instance, XCD run) -------
// KT: the element type of the image the pass runs on -- T, or the real type of T for complex vectors under a real image:
// then the KK complex columns packed into Xr are 2 KK real components of the real pass (alpha applied in the pack, beta
// in the finish), and W comes back as KK complex sums; or the single-precision type a mixed-storage image stores under
// T = double / c128 (the ILMixed instances: pack, finish and the work arrays are those of T)
template <typename T, int KK, typename KT = T>
static hipError_t launch_il(const Product &p, const Batch &b) {
    const DeviceImage &img = p.img;
    const bool opT = p.opT;
    const int strong_zero = p.strong_zero;
    hipStream_t stream = p.stream;
    const T *xd = (const T *)p.x;
    T *yd = (T *)p.y;
    const long long ldx = p.ldx, ldy = p.ldy;
    const T alpha = load_scalar<T>(p.alpha, 1.0), beta = load_scalar<T>(p.beta, 0.0);
    ILWork &il = *p.il;  // (IL batches are planned only with the arrays at hand)
    using R = typename ILT<T>::R;
    constexpr bool MIXED = (std::is_same<T, double>::value && std::is_same<KT, float>::value) ||
                           (std::is_same<T, c128>::value && std::is_same<KT, c64>::value);
    static_assert(std::is_same<KT, T>::value || std::is_same<KT, R>::value || MIXED,
                  "the image holds T, its real type or (mixed storage) its single-precision type");
    using KI = typename std::conditional<MIXED, ILMixed<KT>, KT>::type;  // the kernel instance
    constexpr int CS = ILT<T>::CPLX ? 2 * KK : KK;  // components per vector index (8 or 16)
    const long long xlen = opT ? img.nrows : img.ncols, ylen = opT ? img.ncols : img.nrows;
    if (xlen > il.rows || ylen > il.rows) return hipErrorInvalidValue;
    const int flags = base_flags(opT, p.conj, 0);  // (beta meets y in the finish pass)
    hipError_t e = hipSuccess;
    if (!il.w_clean) e = hipMemsetAsync(il.w, 0, (size_t)il.rows * 128, stream);
    il.w_clean = false;  // (until the finish pass has been enqueued)
    if (e != hipSuccess) return e;
    if (xlen > 0)
        hipLaunchKernelGGL((il_pack_kernel<T, KK>), dim3((unsigned)((xlen + 255) / 256)), dim3(256), 0, stream, xd, ldx, xlen, alpha,
                           b.kact, (T *)il.xr);
    const uint4 *values = (const uint4 *)img.d_values;
    const int *rows = (const int *)img.d_rows, *cols = (const int *)img.d_cols;
    const R *xr = (const R *)il.xr;
    R *w = (R *)il.w;
    // (never coloured -- bsm_plan.cpp: one launch over every workgroup)
    for_each_launch(img, true, [&](const WaveWork *waves, dim3 plain, unsigned) {
        const unsigned nblk = plain.x, xcd_run = (unsigned)b.xcd_run, span = 8u * xcd_run;
        const dim3 grid(xcd_run ? (nblk + span - 1) / span * span : nblk), block(64 * kWavesPerWg);
        with_halves(opT, img.has_off, [&](auto fwd, auto trn) {
            constexpr bool FWD = decltype(fwd)::value, TRN = decltype(trn)::value;
            if (b.nrb == 2)
                hipLaunchKernelGGL((panel_kernel_il<KI, 2, FWD, TRN, CS>), grid, block, 0, stream, waves, values, rows, cols, xr, w,
                                   flags, nblk, xcd_run);
            else
                hipLaunchKernelGGL((panel_kernel_il<KI, 4, FWD, TRN, CS>), grid, block, 0, stream, waves, values, rows, cols, xr, w,
                                   flags, nblk, xcd_run);
        });
    });
    // Y = beta * Y + W over the rows this handle scales (all of them for op T / C), Y += W elsewhere; W = 0 behind
    const YRange r = y_range(img, opT, p.zrange);
    const T one = make_scalar<T>(1.0);
    auto finish = [&](long long lo, long long hi, T bt, int sz) {
        if (hi > lo)
            hipLaunchKernelGGL((il_finish_kernel<T, KK>), dim3((unsigned)((hi - lo + 255) / 256)), dim3(256), 0, stream, yd, ldy, lo, hi, bt,
                               sz, b.kact, (T *)il.w);
    };
    finish(0, r.lo, one, 0);
    finish(r.lo, r.hi, beta, strong_zero);
    finish(r.hi, ylen, one, 0);
    e = hipGetLastError();
    if (e == hipSuccess) il.w_clean = true;
    return e;
}

// the instance of an IL batch: all KK columns of the vector type per index, or half of them (8 components per index)
hipError_t launch_interleaved(const Product &p, const Batch &b) {
    return with_pair(p.img.dtype, p.vt, [&](auto t, auto s) {
        using T = decltype(t);
        constexpr int KK = ILT<T>::KK;
        return b.width == KK / 2 ? launch_il<T, KK / 2, decltype(s)>(p, b) : launch_il<T, KK, decltype(s)>(p, b);
    });
}

#ifdef BSM_TRACE
hipError_t set_trace_il(void *buf) { return set_trace_here(buf); }
#endif

}  // namespace bsm
