// bsm_multi.hip -- the multi-RHS family, K = 4 / 8 / 16 columns per pass over the matrix: panel_kernel_multi and the three
// paths an instance <T, L, TRN, K> can take, one device function each (overloads of panel_multi on PathTag):
//   MultiShape    which path an instance takes, its LDS arrays, its resident-workgroup bound
//   PanelSetup    what every path sets up for a wave's piece (flags, kact, piece fields, the column decode)
//   panel_multi   Register: tile in registers;  TilePipe: tiles prefetched into LDS (kTilePipe);  MatrixPipe: the three
//                 loops on v_mfma_*_16x16x4 (kMfmaAny) with their forward epilogue
#include "bsm_device.h"
#include "bsm_families.h"

namespace bsm {

// multi-RHS register path: y indices of a chunk kept in LDS (0: read from the column list in every iteration)
#ifndef BSM_MULTI_IX
#define BSM_MULTI_IX 1
#endif

// ========================================================================================
// multi right-hand-side variant: Y = alpha*op(A)*X + beta*Y for K columns per pass.  A is
// streamed ONCE for the K columns (LinearMaps loops the columns through _unsafe_mul!, i.e. K
// full sweeps of A).  Same work distribution and layout as panel_kernel; every lane keeps K
// accumulators, the staged x slice is [column][k] in LDS.
// ========================================================================================
template <typename T, int K> constexpr int x_chunk_cols_multi_vec() {
    return (x_chunk_cols<T>() / K) > 64 * TT<T>::E ? (x_chunk_cols<T>() / K) : 64 * TT<T>::E;
}
// the tile-pipelined kernels (below) stage shorter slices: their LDS goes to the two matrix tiles.  A chunk
// must hold whole iterations of every strip height (8 * L strips of E columns) and the 64 * K combine slab.
template <typename T> constexpr bool kRealType = false;
template <> constexpr bool kRealType<float> = true;
template <> constexpr bool kRealType<double> = true;
// which multi-RHS kernels run the tile pipeline: the transposed / fused 8- and 4-column ones in real arithmetic
// with 4 loads per lane (the complex 8-column ones are at the register limit as they are: c64 fused 242 -> 256
// VGPRs + scratch with it; the ComplexF64 4-column one gains nothing over its register path: 487 vs 490 us)
template <typename T, int L, bool TRN, int K> constexpr bool kTilePipe = TRN && L == 4 && kRealType<T> && K >= 4 && K <= 8;
template <typename T, int L> constexpr int x_chunk_cols_pipe() {
    return 8 * L * TT<T>::E > 64 ? 8 * L * TT<T>::E : 64;
}

// XOR swizzle of the LDS matrix tile (16-byte units; strip sI of an iteration, row r of the strip -> unit
// sI * P + (r ^ tile_swz(sI))): a global -> LDS load writes 64 consecutive units per wave-instruction, so the
// image cannot be padded; instead every lane FETCHES row (lane ^ swz) of its strip.  The masks make both ways
// the tile is read -- by row (lane = row, one strip per load) and by column (lane = strip, L rows per lane) --
// free of bank conflicts under ds_read_b128's four 16-lane groups {0-3,12-15,20-27}, {4-11,16-19,28-31}, ...
// (found by exhaustive search over the linear maps strip bits -> row bits; value b = mask of strip bit b).
template <int P, int L> struct TileSwz;
template <> struct TileSwz<8, 4> { static constexpr int col[6] = {0, 1, 0, 2, 4, 0}; };
template <> struct TileSwz<16, 4> { static constexpr int col[6] = {1, 2, 0, 8, 0, 0}; };
template <> struct TileSwz<32, 4> { static constexpr int col[6] = {1, 2, 0, 0, 0, 0}; };
template <> struct TileSwz<64, 4> { static constexpr int col[6] = {1, 2, 0, 0, 0, 0}; };
template <int P, int L> __device__ __forceinline__ constexpr int tile_swz(int s) {
    int h = 0;
    for (int b = 0; b < 6; ++b)
        if ((s >> b) & 1) h ^= TileSwz<P, L>::col[b];
    return h;
}

// 16 bytes per lane from global memory straight into LDS (global_load_lds_dwordx4 ... nt): lane l's bytes land
// at lds_dst + 16 * l, lds_dst wave-uniform.  No VGPR destination and hipcc does not count it: the caller waits
// with vm_wait(n) (loads, atomics and these complete in issue order).
__device__ __forceinline__ void glds16_nt(const void *gsrc, unsigned lds_dst) {
    unsigned keep;
    asm volatile("s_mov_b32 %0, m0\n\ts_mov_b32 m0, %2\n\ts_nop 0\n\tglobal_load_lds_dwordx4 %1, off nt\n\ts_mov_b32 m0, %0"
                 : "=&s"(keep)
                 : "v"(gsrc), "s"(lds_dst)
                 : "memory");
}
// s_waitcnt vmcnt(N) only (expcnt / lgkmcnt fields at their maxima), as the builtin: hipcc's own wait insertion
// sees it, so loads it still tracks as pending are retired in its model too and it does not add a vmcnt(0) of its
// own further down (which would drain the prefetched tile)
__device__ __forceinline__ void vm_wait(int younger) {  // wave-uniform: all but the `younger` newest are done
    asm volatile("" ::: "memory");  // (the builtin is IntrNoMem: loads and LDS reads may not cross it either way)
    switch (younger) {
        case 0: __builtin_amdgcn_s_waitcnt(0x0F70); break;
        case 1: __builtin_amdgcn_s_waitcnt(0x0F71); break;
        case 2: __builtin_amdgcn_s_waitcnt(0x0F72); break;
        case 3: __builtin_amdgcn_s_waitcnt(0x0F73); break;
        default: __builtin_amdgcn_s_waitcnt(0x0F74); break;
    }
    asm volatile("" ::: "memory");
}
// a value whose load must be complete -- for hipcc too -- from here on
template <typename T> __device__ __forceinline__ void settle(T &v) {
    static_assert(sizeof(T) == 4 || sizeof(T) == 8, "one or two registers");
    asm volatile("" : "+v"(v));
}

// ----------------------------------------------------------------------------------------
// ComplexF64, 8 right-hand sides: the matrix pipe.  A complex product with 8 columns is a REAL product with 16:
//     Y = B X,  X' = X as 16 real columns (Re, Im interleaved),  X'' = i X likewise   =>   Y (interleaved) = Re(B) X' + Im(B) X''
// -- exactly the N = 16 of v_mfma_f64_16x16x4_f64, and both halves land in ONE accumulator.  (conj(B): X'' negated.)
// The instruction runs at the vector FMA rate (tools/mfma_rate.hip: 47 vs 56 TFLOP/s), so in real arithmetic -- 8
// of the 16 columns idle -- it buys nothing; here it replaces 64 v_fma_f64 wave-instructions per 16 bytes of
// matrix and lane by 4 MFMAs per 64 lanes, and the K accumulators / x rows per lane (241 VGPRs = 2 waves per SIMD,
// BEM x 8 at 6.1 single products) by 8 VGPRs per 16 x 16 output tile.
//   lane = (ln = lane % 16, lk = lane / 16);  A operand: lane holds A[ln][lk], B operand: B[lk][ln],
//   C / D: column ln, rows lk + 4 r (r = 0..3)                      (guide: cdna_hip_programming.md, f64 layout)
// Forward half, per tile of 16 rows x 16 columns (4 loads of 16 bytes per lane: lane = row ln of the row block,
// column 4 j + lk): A = Re / Im of the loaded element, B = X' / X'' of the staged x slice (LDS, [column][k] complex
// = 16 doubles per column; X'' is X' with neighbouring lanes swapped and a sign: one DPP move), accumulator = the row block's
// 16 x 16 sums for the whole panel.
// Transposed half: the tile goes through LDS once ([column][row], stride 17 units) and comes back with lane =
// (column ln, row 4 q + lk) -- as the B operand; A = X' / X'' of the panel's x ROWS (registers, loaded once per
// panel), so the 16 x 16 sums of a column tile come out with the COLUMN on the lane (consecutive lanes = consecutive
// y entries); they are complete after the panel's row blocks and leave as scalar atomics, 4 per lane.
// ----------------------------------------------------------------------------------------
#ifndef BSM_MFMA_C128_WGS  // resident workgroups per CU the ComplexF64 instance is compiled for (3: 168 VGPRs)
#define BSM_MFMA_C128_WGS 3
#endif
template <typename T, int K> constexpr bool kMfmaPath = BSM_MFMA_C128 && std::is_same<T, c128>::value && K == 8;
// ComplexF32 likewise on v_mfma_f32_16x16x4_f32 (C / D: column ln, rows 4 lk + r -- the f32 map, not the f64 one).  A
// 16-byte load holds TWO columns of a row (strip = 2 columns): one load feeds 4 MFMAs (2 columns x Re / Im), the k
// index of an MFMA runs over the 4 strips of the load.  For the transposed sums to leave as contiguous runs (one
// wave-instruction = Re and Im of 16 consecutive y entries for two k) the x rows enter the A operand with their 16
// components in transposed order: lane ln holds component 4 (ln % 4) + ln / 4, so accumulator row 4 lk + r is
// component 4 r + lk = (k = 2 r + lk / 2, Re / Im = lk % 2).
template <typename T, int K> constexpr bool kMfmaPath32 = BSM_MFMA_C64 && std::is_same<T, c64>::value && K == 8;
// Real arithmetic: N = 16 is 16 right-hand sides.  The K = 16 instances (bsm_mul_multi: batches of 16, remainders of 9-15
// padded) run the same loop with ONE MFMA per operand (no X''): Float64 = two columns per 16-byte load and the f64
// accumulator map, Float32 = four columns per load and the f32 map with the components in transposed order.
template <typename T, int K> constexpr bool kMfmaReal = BSM_MFMA_REAL && kRealType<T> && K == 16;
template <typename T, int K> constexpr bool kMfmaAny = kMfmaPath<T, K> || kMfmaPath32<T, K> || kMfmaReal<T, K>;
// columns per staged chunk: the matrix-pipe kernels take 64 (whole 16-column tiles; 64 x K elements is also the combine
// slab of coloured / exclusive launches) -- ComplexF32: 4 KB per wave instead of 8, a fourth workgroup per CU
template <typename T, int K> constexpr int x_chunk_cols_multi() {
    return kMfmaAny<T, K> ? 64 : x_chunk_cols_multi_vec<T, K>();
}

// ----------------------------------------------------------------------------------------
// The shape of an instance <T, L, TRN, K>: the ONE path it takes and what follows from that -- its LDS arrays and the
// resident workgroups its register allocation must leave room for.  The kernel and the path functions read it here.
// ----------------------------------------------------------------------------------------
enum class MultiPath { Register, TilePipe, MatrixPipe };
template <MultiPath PATH> using PathTag = std::integral_constant<MultiPath, PATH>;  // selects the overload of panel_multi
template <typename T, int L, bool TRN, int K> struct MultiShape {
    static constexpr MultiPath path = kTilePipe<T, L, TRN, K> ? MultiPath::TilePipe
                                      : kMfmaAny<T, K>        ? MultiPath::MatrixPipe
                                                              : MultiPath::Register;
    static constexpr bool PIPE = path == MultiPath::TilePipe, MFA = path == MultiPath::MatrixPipe;
    static constexpr int XCH = PIPE ? x_chunk_cols_pipe<T, L>() : x_chunk_cols_multi<T, K>();  // columns per staged chunk
    static constexpr int XS = XCH * K;  // elements of the x slice (forward half); >= 64*K: also holds the combine slab
    // 16-byte units: max over P of (64 / P) * L strips of P + 1 units; the pipelined kernels hold two tiles
    // (matrix-pipe kernels: one 16 x 16 tile of elements, column stride 17)
    static constexpr int TILE = PIPE ? 2 * L * 64 : (MFA ? (16 * 17 * (int)sizeof(T) + 15) / 16 : L * 72);
    // y indices of the staged chunk (transposed half; the tile pipeline keeps them in registers)
    static constexpr int IXM = (TRN && !PIPE && BSM_MULTI_IX) ? XCH : 1;
    // resident workgroups per CU the register allocation must leave room for: 3 for the pipelined fp32 kernels (their
    // LDS admits 3; fused: 189 VGPRs = 2 per CU without the bound, 168 + 16 spilled dwords with it: C3 in fp32 x 8
    // 176 -> 159 us), 4 for the fp32 matrix-pipe ones (4 KB of slice per wave), BSM_MFMA_C128_WGS for the fp64
    // matrix-pipe ones, 2 otherwise (the fp64 ones fit 3 by themselves)
    static constexpr bool F32 = std::is_same<T, float>::value || std::is_same<T, c64>::value;
    static constexpr int WGS = (MFA && F32) ? 4 : (((PIPE && F32) || (MFA && BSM_MFMA_C128_WGS == 3)) ? 3 : 2);
};

// number of the K slots of a (possibly padded) batch that carry columns
template <int K> __device__ __forceinline__ int kact_of(int flags) {
    const int k = (flags >> FLAG_KACT_SHIFT) & 15;
    return k ? k : K;
}

// ----------------------------------------------------------------------------------------
// What every path sets up for a wave's piece before its loop, built once per panel.
// ----------------------------------------------------------------------------------------
template <typename T, int K> struct PanelSetup {
    bool opT, cjf;
    int kact, m;
    bool live;  // the wave has a piece
    int xbase, col_off, nstrips, ncols;
    // per-column kinds (a symmetric row group holds its diagonal block and its off-diagonal
    // blocks in one panel): forward uses a column unless (op T/C and it is not KIND_OFF),
    // transposed uses it iff (op T/C or KIND_OFF)
    int kinds;
    bool fwd_en, trn_en;
    const Vec16<T> *vb;
    const int *cols;
    int s1w, s1x, s2w, s2x;
    // the column of X a (possibly padded) slot reads
    __device__ __forceinline__ int kc(int k) const { return k < kact ? k : kact - 1; }
    // -> x / y index of piece column w; `off` tells whether the column is KIND_OFF  (the family's own text of
    // col_decode, bsm_device.h: hipcc schedules these kernels differently around the shared form)
    __device__ __forceinline__ int col_lookup(int w, bool &off) const {
        if (xbase < 0) {
            const int raw = cols[col_off + w];
            off = raw >= 0 && (kinds & 3) == KIND_OFF;
            return raw & 0x7fffffff;
        }
        const int sh = w < s1w ? 0 : (w < s2w ? 2 : 4);
        off = ((kinds >> sh) & 3) == KIND_OFF;
        return w + (w < s1w ? xbase : (w < s2w ? s1x : s2x));
    }
};
template <typename T, int K>
__device__ __forceinline__ PanelSetup<T, K> panel_setup(const WaveD &wd, int flags) {
    PanelSetup<T, K> ps;
    ps.opT = (flags & FLAG_OPT) != 0;
    ps.cjf = (flags & FLAG_CONJ) != 0;
    ps.kact = kact_of<K>(flags);
    ps.m = wd.m;
    ps.live = wd.npieces > 0;
    ps.fwd_en = ps.trn_en = false;
    return ps;
}
template <bool FWD, bool TRN, typename T, int K>
__device__ __forceinline__ void load_piece(PanelSetup<T, K> &ps, const WaveD &wd, const uint4 *__restrict__ values,
                                           const int *__restrict__ cols) {
    const PieceD pc = wd.first;
    ps.xbase = pc.xbase;
    ps.col_off = pc.col_off;
    ps.nstrips = pc.nstrips;
    ps.ncols = pc.ncols;
    ps.kinds = pc.kind;
    const bool has_off = (pc.kind & kKindHasOff) != 0;
    ps.fwd_en = FWD && (!ps.opT || has_off);
    ps.trn_en = TRN && (ps.opT || has_off);
    ps.vb = reinterpret_cast<const Vec16<T> *>(values + (((uint64_t)pc.val_hi << 32) | pc.val_lo));
    ps.cols = cols;
    ps.s1w = wd.seg1_w, ps.s1x = wd.seg1_x - wd.seg1_w;
    ps.s2w = wd.seg2_w, ps.s2x = pc.seg2_x - wd.seg2_w;
}

// ----------------------------------------------------------------------------------------
// What the register path and the tile pipeline share: K accumulators per lane with the lane on the row (forward half),
// and the column-role layout of the transposed half.
// Transposed half, V[w][k] = sum_i B[i][w] * X[row(i)][k].  With the lane on the row (the layout the
// matrix arrives in) every one of the K right-hand sides would need its own cross-lane reduction per
// iteration (K halving butterflies: the multi-RHS fused products were bound by exactly that: C3 x 8 at
// 2.6 products, the BEM fixture at 6.4).  Instead the loaded tile (L * G strips of P rows, 16 bytes per
// lane and load) goes through LDS once and comes back in a COLUMN-role layout: lane (sp = lane % NS,
// rg = lane / NS) holds strip sp (E columns) for the L rows rg * L .. rg * L + L - 1 -- the same 16
// bytes per lane and load, transposed.  The x entries of those L rows stay in registers for the whole
// piece, the transposed product becomes L * E * K in-lane FMAs like the forward one, and only E * K
// partial sums per lane are reduced over the RG = 64 / NS lanes of a strip.
// ----------------------------------------------------------------------------------------
template <typename T, int L, int K>
__device__ __forceinline__ void load_x_rows(const PanelSetup<T, K> &ps, const WaveD &wd, const int *__restrict__ rows,
                                            const T *__restrict__ x, long long ldx, int rg, T (&xrr)[L][K]) {
#pragma unroll
    for (int j = 0; j < L; ++j) {
        const int r = rg * L + j;
        const bool ok = r < ps.m;
        int ri = 0;
        if (ok) ri = row_index(wd, rows, r);
#pragma unroll
        for (int k = 0; k < K; ++k) xrr[j][k] = ok ? x[ri + ps.kc(k) * ldx] : zero_of(T{});
    }
}
// a lane's 16 bytes (E columns of one row) times the K staged x entries of each of the columns (forward half) ...
template <typename T, int K> __device__ __forceinline__ void fma_row_role(T (&acc)[K], const Vec16<T> &b, const T *xp, bool cjf) {
#pragma unroll
    for (int e = 0; e < TT<T>::E; ++e) {
        const T bv = cj(b.v[e], cjf);
#pragma unroll
        for (int k = 0; k < K; ++k) acc[k] = madd(acc[k], bv, xp[e * K + k]);
    }
}
// ... and times the K x entries of its row, into the lane's E * K column sums (transposed half)
template <typename T, int K, int EK> __device__ __forceinline__ void fma_col_role(T (&tv)[EK], const Vec16<T> &u, const T (&xr)[K], bool cjf) {
#pragma unroll
    for (int e = 0; e < TT<T>::E; ++e) {
        const T bv = cj(u.v[e], cjf);
#pragma unroll
        for (int k = 0; k < K; ++k) tv[e * K + k] = madd(tv[e * K + k], bv, xr[k]);
    }
}
// the forward sums of the 64 / P row groups of a wave, folded onto every lane of a row: what the kernel combines and writes
template <int P, bool FWD, typename T, int K> __device__ __forceinline__ void fold_row_groups(const T (&acc)[K], T (&out)[K]) {
#pragma unroll
    for (int k = 0; k < K; ++k) {
        T a = acc[k];
        if (FWD) {
#pragma unroll
            for (int d = P; d < 64; d <<= 1) a = add(a, shx(a, d));
        }
        out[k] = a;
    }
}

// ----------------------------------------------------------------------------------------
// The register path: an iteration's tile is loaded into registers, used by row, and turned through LDS for the
// transposed half.
// ----------------------------------------------------------------------------------------
template <typename T, int L, int P, bool FWD, bool TRN, int K>
__device__ __forceinline__ bool panel_multi(PathTag<MultiPath::Register>, const WaveD &wd, const uint4 *__restrict__ values,
                                            const int *__restrict__ rows, const int *__restrict__ cols,
                                            const T *__restrict__ x, long long ldx, T *__restrict__ y, long long ldy,
                                            T alpha, int flags, int lane, T *xs, Vec16<T> *tile, int *ixm, T (&out)[K]) {
    PanelSetup<T, K> ps = panel_setup<T, K>(wd, flags);  // (the piece fields follow behind the x rows: load_piece)
    constexpr int E = TT<T>::E, G = 64 / P, NC = G * L * E, XCH = MultiShape<T, L, TRN, K>::XCH;
    constexpr int NS = G * L, RG = 64 / NS;
    constexpr int PM = P + 1;  // strip stride in the LDS tile (16-byte units): conflict-free for both layouts
    static_assert(XCH % NC == 0, "x chunk must hold whole iterations");
    static_assert(NS <= 64, "an iteration's strips must fit the wave");
    const int m = ps.m;
    const int i = lane & (P - 1), g = lane / P;
    const int sp = lane % NS, rg = lane / NS;
    const bool row_ok = i < m;
    T acc[K];
#pragma unroll
    for (int k = 0; k < K; ++k) acc[k] = zero_of(T{});
    T xrr[TRN ? L : 1][K];
    if constexpr (TRN) load_x_rows<T, L, K>(ps, wd, rows, x, ldx, rg, xrr);

    if (ps.live) {
        load_piece<FWD, TRN>(ps, wd, values, cols);
        const int nstrips = ps.nstrips, ncols = ps.ncols;
        // the x slice (forward half) and the y indices (transposed half) of the chunk of columns at c0
        // (the lane that stages a column writes its K entries 64 / 128 bytes apart from its neighbours': 16- / 32-way bank
        // conflicts per store -- an XOR swizzle of the slot (k ^ column index within the bank row) was measured: +-0, the
        // staging is bound by the K x 64 scattered line requests of the gather, not by the LDS)
        auto stage_columns = [&](int c0) {
            if (!(ps.fwd_en || (BSM_MULTI_IX && ps.trn_en))) return;
#pragma unroll
            for (int q = 0; q < XCH / 64; ++q) {
                const int c = q * 64 + lane;
                const int w = c0 + c;
                if (BSM_DBG(DBG_NO_XGATHER)) {  // (timing probe: no column list, no x loads)
                    if (BSM_MULTI_IX && TRN) ixm[c] = w < ncols ? w : -1;
                    if (ps.fwd_en) {
#pragma unroll
                        for (int k = 0; k < K; ++k) xs[c * K + k] = zero_of(T{});
                    }
                } else if (w < ncols + NC) {
                    bool ok = w < ncols, off = false;
                    const int xi = ok ? ps.col_lookup(w, off) : 0;
                    // the chunk's y indices stay in LDS for the emission of its iterations (-1: the column takes no
                    // part): read from the column list there, every iteration waited for a dependent load in front
                    // of its atomics
                    if (BSM_MULTI_IX && TRN) ixm[c] = (ok && (ps.opT || off)) ? xi : -1;
                    ok = ok && (!ps.opT || off);
                    if (ps.fwd_en) {
#pragma unroll
                        for (int k = 0; k < K; ++k) xs[c * K + k] = ok ? x[xi + ps.kc(k) * ldx] : zero_of(T{});
                    }
                }
            }
        };
        for (int c0 = 0; c0 < ncols; c0 += XCH) {
            stage_columns(c0);
            const int s_end = min(nstrips, (c0 + XCH) / E);
            for (int s0 = c0 / E; s0 < s_end; s0 += G * L) {
                // (issuing the next iteration's matrix loads before this iteration's arithmetic -- two register
                // buffers -- was measured here too: C3 x 8 379 -> 462 us, C4 slice x 8 406 -> 570 us)
                Vec16<T> b[L];
#pragma unroll
                for (int l = 0; l < L; ++l) {
                    const int s = s0 + l * G + g;
                    if (row_ok && s < nstrips) {
                        b[l] = load_stream16(&ps.vb[(uint32_t)(s * m + i)]);  // multi-RHS: always with the hint
                    } else {
#pragma unroll
                        for (int e = 0; e < E; ++e) b[l].v[e] = zero_of(T{});
                    }
                }
                if (ps.fwd_en) {
                    const int cb = (s0 - c0 / E) * E;
#pragma unroll
                    for (int l = 0; l < L; ++l) fma_row_role<T, K>(acc, b[l], &xs[(cb + (l * G + g) * E) * K], ps.cjf);
                }
                if (!ps.trn_en) continue;
                // registers (row role) -> LDS -> registers (column role); one wave, LDS runs in order
#pragma unroll
                for (int l = 0; l < L; ++l) tile[(l * G + g) * PM + i] = b[l];
                T tv[E * K];
#pragma unroll
                for (int q = 0; q < E * K; ++q) tv[q] = zero_of(T{});
#pragma unroll
                for (int j = 0; j < L; ++j) fma_col_role<T, K>(tv, tile[sp * PM + rg * L + j], xrr[j], ps.cjf);
                int pos = 0, dup = 0;
                ReduceAbove<T, E * K, NS>::run(tv, lane, pos, dup);
                constexpr int CF = (E * K / RG) > 1 ? (E * K / RG) : 1;
                const int s = s0 + sp;  // the lane's strip of the piece
                if ((lane & dup) != 0 || s >= nstrips) continue;
#pragma unroll
                for (int jj = 0; jj < CF; ++jj) {
                    const int q = pos + jj;
                    const int e = q / K, k = q % K;
                    const int w = s * E + e;
                    if (w < ncols) {
                        bool off = false;
                        int yi;
                        if (BSM_MULTI_IX) {
                            yi = ixm[w - c0];
                            off = yi >= 0;
                        } else {
                            yi = ps.col_lookup(w, off);
                            off = ps.opT || off;
                        }
                        if (off && k < ps.kact) {
                            T *yp = &y[yi + k * ldy];
                            const T val = mul(alpha, tv[jj]);
                            if (flags & FLAG_RMW)
                                *yp = add(*yp, val);
                            else if (!BSM_DBG(DBG_NO_GLOBAL_ATOMICS))
                                atomic_acc(yp, val);
                        }
                    }
                }
            }
        }
    }
    fold_row_groups<P, FWD>(acc, out);
    return false;
}

// ----------------------------------------------------------------------------------------
// The tile pipeline (kTilePipe).
// Fused / transposed multi-RHS products at 2-3 waves per SIMD were bound by the bytes in flight (one
// 4 KB tile per wave, and only while the wave was not computing: C3 x 8 ran at 2.5 TB/s with the VALU
// 39 % and the LDS 43 % busy), and a second register tile costs a resident wave.  The tile goes
// through LDS anyway (transposition above), so it is loaded THERE directly, one iteration ahead, with
// no register landing: two LDS tiles per wave, global_load_lds into the one while the other is read
// by row (forward half) and by column (transposed half).  In-order completion of vector memory
// operations does the bookkeeping: the wait for tile n is `all but tile n+1's loads`, which also
// covers every older atomic -- so iteration n's y contributions are issued AFTER that wait in
// iteration n+1 (held in CF registers meanwhile), and nothing else in the loop may load from global
// memory: a slice's gathered column indices are fetched with its x values and kept (in registers).
// ----------------------------------------------------------------------------------------
template <typename T, int L, int P, bool FWD, bool TRN, int K>
__device__ __forceinline__ bool panel_multi(PathTag<MultiPath::TilePipe>, const WaveD &wd, const uint4 *__restrict__ values,
                                            const int *__restrict__ rows, const int *__restrict__ cols,
                                            const T *__restrict__ x, long long ldx, T *__restrict__ y, long long ldy,
                                            T alpha, int flags, int lane, T *xs, Vec16<T> *tile, int *, T (&out)[K]) {
    PanelSetup<T, K> ps = panel_setup<T, K>(wd, flags);  // (the piece fields follow behind the x rows: load_piece)
    constexpr int E = TT<T>::E, G = 64 / P, NC = G * L * E, XCH = MultiShape<T, L, TRN, K>::XCH;
    constexpr int NS = G * L, RG = 64 / NS, NSI = G * L;
    constexpr int CF = (E * K / RG) > 1 ? (E * K / RG) : 1;
    constexpr int NE = CF > K ? CF / K : 1;  // columns (of E) a lane's CF sums belong to
    static_assert(XCH % NC == 0, "x chunk must hold whole iterations");
    static_assert(NS <= 64, "an iteration's strips must fit the wave");
    const int m = ps.m, kact = ps.kact;
    const int i = lane & (P - 1), g = lane / P;
    const int sp = lane % NS, rg = lane / NS;
    T acc[K];
#pragma unroll
    for (int k = 0; k < K; ++k) acc[k] = zero_of(T{});
    T xrr[TRN ? L : 1][K];
    if constexpr (TRN) load_x_rows<T, L, K>(ps, wd, rows, x, ldx, rg, xrr);
    if (ps.live) {
        load_piece<FWD, TRN>(ps, wd, values, cols);
        const int nstrips = ps.nstrips, ncols = ps.ncols;
        const int nit = (nstrips + NSI - 1) / NSI;
        const unsigned lds0 = __builtin_amdgcn_readfirstlane((unsigned)(size_t)tile);
        const int hg = tile_swz<P, L>(g);
        const int cbase = sp * P + ((rg * L) ^ tile_swz<P, L>(sp));
        auto issue = [&](int it, int buf) {
            const int s0 = it * NSI;
#pragma unroll
            for (int l = 0; l < L; ++l) {
                if (s0 + l * G < nstrips) {  // wave-uniform: the load is issued, and counted
                    const int s = s0 + l * G + g;
                    const int rho = i ^ tile_swz<P, L>(l * G) ^ hg;
                    if (BSM_DBG(DBG_NO_MATRIX)) {
                    } else if (rho < m && s < nstrips)
                        glds16_nt(&ps.vb[(uint32_t)(s * m + rho)], lds0 + (unsigned)((buf * L + l) * 1024));
                    else
                        tile[(buf * L + l) * 64 + lane] = Vec16<T>{};
                } else {
                    tile[(buf * L + l) * 64 + lane] = Vec16<T>{};
                }
            }
        };
        auto loads_of = [&](int it) {
            const int left = nstrips - it * NSI;
            const int nl = (left + G - 1) / G;
            return nl < L ? nl : L;
        };
        int dq_yi[NE];
        T dq_val[CF];
#pragma unroll
        for (int q = 0; q < NE; ++q) dq_yi[q] = -1;
        int pos = 0, dup = 0;
        auto emit = [&]() {
#pragma unroll
            for (int jj = 0; jj < CF; ++jj) {
                const int yi = dq_yi[jj / K];
                const int k = (pos + jj) % K;
                // (atomics in coloured launches too: a read-modify-write's load would be waited for with
                // vmcnt(0) by the compiler, i.e. drain the prefetch every iteration)
                if (yi >= 0 && k < kact) atomic_acc(&y[yi + k * ldy], mul(alpha, dq_val[jj]));
            }
        };
        // a slice of columns: x values (forward half) and the gathered indices.  The indices stay in
        // REGISTERS, lane c of cir[q] holding column q * 64 + c of the slice, and are fetched across lanes
        // (ds_bpermute) when a lane emits: an LDS array of them was the 256 bytes per wave that kept a fourth
        // workgroup of the 4-column fp64 kernel off the CU.
        int cir[XCH / 64];
#pragma unroll
        for (int q = 0; q < XCH / 64; ++q) cir[q] = 0;
        auto stage_slice = [&](int c0) {
#pragma unroll
            for (int q = 0; q < XCH / 64; ++q) {
                const int c = q * 64 + lane;
                const int w = c0 + c;
                if (ps.xbase < 0) {
                    // (waited for HERE: a loaded register whose first use lies in the loop body makes hipcc
                    // wait vmcnt(0) there in every iteration, which drains the prefetched tile)
                    cir[q] = ps.cols[ps.col_off + min(w, ncols - 1)];
                    settle(cir[q]);
                }
                if (w < ncols + NC) {
                    bool ok = w < ncols, off = false;
                    if (ps.fwd_en) {
                        const int xi = ok ? ps.col_lookup(w, off) : 0;
                        ok = ok && (!ps.opT || off);
#pragma unroll
                        for (int k = 0; k < K; ++k) xs[c * K + k] = ok ? x[xi + ps.kc(k) * ldx] : zero_of(T{});
                    }
                }
            }
        };
        // A wave's start is a chain of dependent round trips (descriptor -> row list -> x rows, column list
        // -> x slice -> first tile), and a panel of the BEM fixture is 3-4 iterations long: the first tile's
        // loads go out first (they need the descriptor only), the first slice is staged while the x rows
        // above are still in flight, and only then everything is waited for -- three round trips, not six.
        if (nit > 0) issue(0, 0);
        if (nit > 0) stage_slice(0);
        // the x rows: no load hipcc knows of may be pending inside the loop, or its wait for it (a
        // vmcnt(0) at the first use, executed every iteration) would drain the prefetched tile
        if (TRN) {
#pragma unroll
            for (int j = 0; j < L; ++j)
#pragma unroll
                for (int k = 0; k < K; ++k) settle(xrr[j][k]);
        }
        for (int it = 0; it < nit; ++it) {
            const int buf = it & 1;
            const int s0 = it * NSI;
            const int c0 = (s0 * E) / XCH * XCH;
            if (s0 * E == c0 && it > 0) stage_slice(c0);
            int younger = 0;
            if (it + 1 < nit) {
                issue(it + 1, buf ^ 1);
                younger = BSM_DBG(DBG_NO_MATRIX) ? 0 : loads_of(it + 1);
            }
            vm_wait(younger);
            if (!BSM_DBG(DBG_NO_GLOBAL_ATOMICS)) emit();  // iteration it-1's sums
            if (ps.fwd_en && !BSM_DBG(DBG_NO_FWD_HALF)) {
                const int cb = s0 * E - c0;
#pragma unroll
                for (int l = 0; l < L; ++l)
                    fma_row_role<T, K>(acc, tile[(buf * L + l) * 64 + (lane ^ tile_swz<P, L>(l * G) ^ hg)],
                                       &xs[(cb + (l * G + g) * E) * K], ps.cjf);
            }
            if (!ps.trn_en || BSM_DBG(DBG_NO_TRN_HALF)) continue;
            T tv[E * K];
#pragma unroll
            for (int q = 0; q < E * K; ++q) tv[q] = zero_of(T{});
#pragma unroll
            for (int j = 0; j < L; ++j) fma_col_role<T, K>(tv, tile[buf * L * 64 + (cbase ^ j)], xrr[j], ps.cjf);
            pos = 0, dup = 0;
            ReduceAbove<T, E * K, NS>::run(tv, lane, pos, dup);
            const int s = s0 + sp;
            const bool mine = (lane & dup) == 0 && s < nstrips;
#pragma unroll
            for (int q = 0; q < NE; ++q) {
                const int w = s * E + pos / K + q;
                int raw = 0;
                if (ps.xbase < 0) {  // (every lane takes part in the exchange)
                    const int c = (w - c0) & (XCH - 1);
#pragma unroll
                    for (int h = 0; h < XCH / 64; ++h) {
                        const int v = __shfl(cir[h], c & 63, 64);
                        if ((c >> 6) == h) raw = v;
                    }
                }
                int yi = -1;
                if (mine && w < ncols) {
                    bool off;
                    if (ps.xbase < 0) {
                        off = raw >= 0 && (ps.kinds & 3) == KIND_OFF;
                        yi = raw & 0x7fffffff;
                    } else {
                        yi = ps.col_lookup(w, off);
                    }
                    if (!(ps.opT || off)) yi = -1;
                }
                dq_yi[q] = yi;
            }
#pragma unroll
            for (int jj = 0; jj < CF; ++jj) dq_val[jj] = tv[jj];
        }
        emit();
    }
    fold_row_groups<P, FWD>(acc, out);
    return false;
}

// ----------------------------------------------------------------------------------------
// The matrix pipe (kMfmaAny; layouts in the comment at kMfmaPath above): row blocks of 16, the x rows of the panel as
// operands, one accumulator per row block.  The three element classes -- ComplexF64 (MF), ComplexF32 (MF32), real x 16
// (MFR) -- keep a prologue and a loop each, as they were written: the one loop over an element-type trait that was
// tried costs <c64, 4, false, true, 8> 235 instructions and <c128, 4, true, true, 8> a spilled dword
// (docs/experiments_r28.md).  They share the staging, and the epilogue that hands the forward sums on.
// -> true: the wave has added its forward sums to y itself (accumulate mode); else they are in `out`, lane = row
// ----------------------------------------------------------------------------------------
template <typename T, int L, int P, bool FWD, bool TRN, int K>
__device__ __forceinline__ bool panel_multi(PathTag<MultiPath::MatrixPipe>, const WaveD &wd, const uint4 *__restrict__ values,
                                            const int *__restrict__ rows, const int *__restrict__ cols,
                                            const T *__restrict__ x, long long ldx, T *__restrict__ y, long long ldy,
                                            T alpha, int flags, int lane, T *xs, Vec16<T> *tile, int *ixm, T (&out)[K]) {
    PanelSetup<T, K> ps = panel_setup<T, K>(wd, flags);  // (the piece fields follow behind the x rows: load_piece)
    constexpr int E = TT<T>::E;
    constexpr int G = 64 / P;
    constexpr int NC = G * L * E;
    constexpr int XCH = MultiShape<T, L, TRN, K>::XCH;
    const bool opT = ps.opT, cjf = ps.cjf;
    const int kact = ps.kact;
    auto kc = [&](int k) { return ps.kc(k); };
    const int m = ps.m;
    // matrix-pipe path (above): row blocks of 16, the x rows of the panel as B operands, one accumulator per row block
    constexpr bool MF = kMfmaPath<T, K>;
    constexpr int MR = (P + 15) / 16;
    const int ln = lane & 15, lk = lane >> 4;
    double xr1[(MF && TRN) ? 4 * MR : 1];  // (X'' of a row is X' with neighbouring lanes swapped, and a sign)
    constexpr bool MFR = kMfmaReal<T, K>;
    constexpr bool MFR64 = MFR && sizeof(T) == 8, MFR32 = MFR && sizeof(T) == 4;
    v4f64 facc[(MF || MFR64) ? MR : 1];
    if constexpr (MF) {
#pragma unroll
        for (int rb = 0; rb < MR; ++rb) facc[rb] = v4f64{0.0, 0.0, 0.0, 0.0};
        if (TRN) {
#pragma unroll
            for (int q = 0; q < 4 * MR; ++q) {
                const int r = 4 * q + lk;
                double re = 0.0, im = 0.0;
                if (r < m && !BSM_DBG(DBG_NO_XGATHER)) {
                    const int ri = row_index(wd, rows, r);
                    const double *px = reinterpret_cast<const double *>(&x[ri + kc(ln >> 1) * ldx]);
                    re = px[0];
                    im = px[1];
                }
                // (alpha goes in here: the transposed sums leave the lanes as they come out of the accumulator)
                xr1[q] = (ln & 1) ? alpha.re * im + alpha.im * re : alpha.re * re - alpha.im * im;
            }
        }
    }
    constexpr bool MF32 = kMfmaPath32<T, K>;
    constexpr bool MFA = MF || MF32 || MFR;
    float fr1[(MF32 && TRN) ? 4 * MR : 1], fr2[(MF32 && TRN) ? 4 * MR : 1];
    v4f32 facc32[(MF32 || MFR32) ? MR : 1];
    // real types, K = 16: the panel's x rows (alpha folded in) as A operands of the transposed half; the lane carries
    // component (= right-hand side) compA: ln for the f64 accumulator map, the transposed order for the f32 one
    const int compA = MFR32 ? 4 * (ln & 3) + (ln >> 2) : ln;
    T rr[(MFR && TRN) ? 4 * MR : 1];
    if constexpr (MFR) {
#pragma unroll
        for (int rb = 0; rb < MR; ++rb) {
            if constexpr (MFR64) facc[rb] = v4f64{0.0, 0.0, 0.0, 0.0};
            if constexpr (MFR32) facc32[rb] = v4f32{0.f, 0.f, 0.f, 0.f};
        }
        if (TRN) {
#pragma unroll
            for (int q = 0; q < 4 * MR; ++q) {
                const int r = 4 * q + lk;
                T v = zero_of(T{});
                if (r < m && !BSM_DBG(DBG_NO_XGATHER)) {
                    const int ri = row_index(wd, rows, r);
                    v = mul(alpha, x[ri + kc(compA) * ldx]);
                }
                rr[q] = v;
            }
        }
    }
    if constexpr (MF32) {
#pragma unroll
        for (int rb = 0; rb < MR; ++rb) facc32[rb] = v4f32{0.f, 0.f, 0.f, 0.f};
        if (TRN) {
            const int comp = 4 * (ln & 3) + (ln >> 2);  // the component this lane carries in the A operand (above)
#pragma unroll
            for (int q = 0; q < 4 * MR; ++q) {
                const int r = 4 * q + lk;
                float re = 0.f, im = 0.f;
                if (r < m && !BSM_DBG(DBG_NO_XGATHER)) {
                    const int ri = row_index(wd, rows, r);
                    const c64 xv = x[ri + kc(comp >> 1) * ldx];
                    re = alpha.re * xv.re - alpha.im * xv.im;  // (alpha goes in here)
                    im = alpha.re * xv.im + alpha.im * xv.re;
                }
                fr1[q] = (comp & 1) ? im : re;                    // X'
                fr2[q] = (comp & 1) ? re : -im;                   // X'' = i X
                if (cjf) fr2[q] = -fr2[q];
            }
        }
    }
    if (ps.live) {
        load_piece<FWD, TRN>(ps, wd, values, cols);
        const int nstrips = ps.nstrips;
        const int ncols = ps.ncols;
        const bool fwd_en = ps.fwd_en, trn_en = ps.trn_en;
        const Vec16<T> *vb = ps.vb;
        auto col_lookup = [&](int w, bool &off) -> int { return ps.col_lookup(w, off); };
        // (matrix-pipe path in accumulate mode: alpha goes into the slice, the forward sums leave from the accumulators)
        const bool fold = MFA && !(flags & (FLAG_DIRECT | FLAG_RMW));
        // (the lane that stages a column writes its K entries 64 / 128 bytes apart from its neighbours': 16- / 32-way bank
        // conflicts per store -- an XOR swizzle of the slot (k ^ column index within the bank row) was measured: +-0, the
        // staging is bound by the K x 64 scattered line requests of the gather, not by the LDS)
        auto stage_columns = [&](int c0) {
            if (fwd_en || (BSM_MULTI_IX && trn_en)) {
#pragma unroll
                for (int q = 0; q < XCH / 64; ++q) {
                    const int c = q * 64 + lane;
                    const int w = c0 + c;
                    if (BSM_DBG(DBG_NO_XGATHER)) {  // (timing probe: no column list, no x loads)
                        if (BSM_MULTI_IX && TRN) ixm[c] = w < ncols ? w : -1;
                        if (fwd_en) {
#pragma unroll
                            for (int k = 0; k < K; ++k) xs[c * K + k] = zero_of(T{});
                        }
                    } else if (MFA || w < ncols + NC) {  // (the matrix-pipe tiles read whole 16-column tiles of the slice)
                        bool ok = w < ncols, off = false;
                        const int xi = ok ? col_lookup(w, off) : 0;
                        // the chunk's y indices stay in LDS for the emission of its iterations (-1: the column takes no
                        // part): read from the column list there, every iteration waited for a dependent load in front
                        // of its atomics
                        if (BSM_MULTI_IX && TRN) ixm[c] = (ok && (opT || off)) ? xi : -1;
                        ok = ok && (!opT || off);
                        if (fwd_en) {
#pragma unroll
                            for (int k = 0; k < K; ++k)
                                xs[c * K + k] = ok ? (fold ? mul(alpha, x[xi + kc(k) * ldx]) : x[xi + kc(k) * ldx]) : zero_of(T{});
                        }
                    }
                }
            }
        };
        if constexpr (MF) {
            // one step = one row block (16 rows) of one column tile (16 columns): 4 loads of 16 bytes per lane, issued
            // one step ahead of their use
            const double *xsd = reinterpret_cast<const double *>(xs);
            const int nrb = (m + 15) >> 4;
            auto fetch = [&](c128(&b)[4], int t0, int rb) {
                const int row = rb * 16 + ln;
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    const int w = t0 + 4 * j + lk;
                    if (row < m && w < ncols && !BSM_DBG(DBG_NO_MATRIX)) {
                        const Vec16<T> q = load_stream16(&vb[(uint32_t)(w * m + row)]);
                        b[j] = q.v[0];
                    } else {
                        b[j] = c128{0.0, 0.0};
                    }
                }
            };
            // Vector-memory operations retire in issue order and an atomic's round trip to the memory side is long: sums
            // emitted right behind a tile would stand between the NEXT loads and their wait.  They are parked (4 sums, 4
            // indices per lane) and leave one step later, right BEHIND the following step's loads -- whose wait then
            // only has to let the 4 younger atomics pass.
            // The transposed sums come out TRANSPOSED (operands swapped: A = the x rows, B = the tile), lane = (column
            // ln, component n = lk + 4 r = Re / Im of k = n / 2): one wave-instruction adds Re and Im of 16 consecutive
            // columns for two k -- two runs of 256 contiguous bytes, 8-10 cache lines.  What the memory-side atomics
            // cost is the number of LINES a wave-instruction touches (measured on the BEM fixture, atomics alone:
            // 12-16 lines 390 us, 16-20 lines 520 us).
            double pd[4];
            int pyi = -1;
            bool pending = false;
            auto emit = [&]() {
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    const int n = lk + 4 * r;  // k = n / 2, Re / Im = n % 2 (alpha is in the x rows already)
                    const double val = pd[r];
                    if (pyi >= 0 && (n >> 1) < kact) {
                        double *yp = reinterpret_cast<double *>(&y[pyi + (n >> 1) * ldy]) + (n & 1);
                        if (flags & FLAG_RMW)
                            *yp += val;
                        else if (!BSM_DBG(DBG_NO_GLOBAL_ATOMICS))
                            atomicAdd(yp, val);
                    }
                }
                pending = false;
            };
            c128 nxt[4];
            fetch(nxt, 0, 0);
            for (int t0 = 0; t0 < ncols; t0 += 16) {
                const int c0 = t0 & ~(XCH - 1);
                if (t0 == c0) stage_columns(c0);
                const int t_end = min(ncols, c0 + XCH);
                v4f64 dt = {0.0, 0.0, 0.0, 0.0};
#pragma unroll
                for (int rb = 0; rb < MR; ++rb) {
                    if (rb >= nrb) break;  // (wave-uniform)
                    c128 b[4];
#pragma unroll
                    for (int j = 0; j < 4; ++j) b[j] = nxt[j];
                    if (rb + 1 < nrb)
                        fetch(nxt, t0, rb + 1);
                    else if (t0 + 16 < ncols)
                        fetch(nxt, t0 + 16, 0);
                    if (pending) emit();
                    if (fwd_en && !BSM_DBG(DBG_NO_FWD_HALF)) {
#pragma unroll
                        for (int j = 0; j < 4; ++j) {
                            const int wl = t0 - c0 + 4 * j + lk;  // column of the staged slice ([column][k] complex)
                            const double x1 = xsd[wl * 16 + ln];
                            double x2 = dppx<DPP_QUAD_XOR1>(x1);  // the other component of the same k: the neighbouring lane
                            x2 = (((ln & 1) == 0) != cjf) ? -x2 : x2;
                            facc[rb] = __builtin_amdgcn_mfma_f64_16x16x4f64(x1, b[j].re, facc[rb], 0, 0, 0);
                            facc[rb] = __builtin_amdgcn_mfma_f64_16x16x4f64(x2, b[j].im, facc[rb], 0, 0, 0);
                        }
                    }
                    if (trn_en && !BSM_DBG(DBG_NO_TRN_HALF)) {
#pragma unroll
                        for (int j = 0; j < 4; ++j) tile[(4 * j + lk) * 17 + ln].v[0] = b[j];
#pragma unroll
                        for (int q = 0; q < 4; ++q) {
                            const c128 u = tile[ln * 17 + 4 * q + lk].v[0];
                            const double r1 = xr1[rb * 4 + q];
                            double r2 = dppx<DPP_QUAD_XOR1>(r1);
                            r2 = (((ln & 1) == 0) != cjf) ? -r2 : r2;
                            dt = __builtin_amdgcn_mfma_f64_16x16x4f64(r1, u.re, dt, 0, 0, 0);
                            dt = __builtin_amdgcn_mfma_f64_16x16x4f64(r2, u.im, dt, 0, 0, 0);
                        }
                    }
                }
                if (trn_en) {
                    // lane (ln, lk) holds components lk + 4 r of column t0 + ln
#pragma unroll
                    for (int r = 0; r < 4; ++r) pd[r] = dt[r];
                    pyi = (t0 + ln < t_end) ? ixm[t0 + ln - c0] : -1;  // (read now: the next chunk's staging overwrites the list)
                    pending = true;
                }
            }
            if (pending) emit();
        }
        if constexpr (MF32) {
            // one step = one row block (16 rows) of one column tile (16 columns = 8 strips): 2 loads of 16 bytes per
            // lane (lane = row ln, strip 4 j + lk), issued one step ahead; everything else as in the ComplexF64 loop
            const float *xsf = reinterpret_cast<const float *>(xs);
            c64 *tile8 = reinterpret_cast<c64 *>(tile);
            const int comp = 4 * (ln & 3) + (ln >> 2);
            const int nrb = (m + 15) >> 4;
            auto fetch = [&](Vec16<T>(&b)[2], int t0, int rb) {
                const int row = rb * 16 + ln;
#pragma unroll
                for (int j = 0; j < 2; ++j) {
                    const int sidx = (t0 >> 1) + 4 * j + lk;
                    if (row < m && sidx < nstrips && !BSM_DBG(DBG_NO_MATRIX)) {
                        b[j] = load_stream16(&vb[(uint32_t)(sidx * m + row)]);
                    } else {
                        b[j].v[0] = c64{0.f, 0.f};
                        b[j].v[1] = c64{0.f, 0.f};
                    }
                }
            };
            float pd[4];
            int pyi = -1;
            bool pending = false;
            auto emit = [&]() {
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    const int kq = 2 * r + (lk >> 1);  // accumulator row 4 lk + r = component 4 r + lk
                    if (pyi >= 0 && kq < kact) {
                        float *yp = reinterpret_cast<float *>(&y[pyi + kq * ldy]) + (lk & 1);
                        if (flags & FLAG_RMW)
                            *yp += pd[r];
                        else if (!BSM_DBG(DBG_NO_GLOBAL_ATOMICS))
                            atomicAdd(yp, pd[r]);
                    }
                }
                pending = false;
            };
            Vec16<T> nxt[2];
            fetch(nxt, 0, 0);
            for (int t0 = 0; t0 < ncols; t0 += 16) {
                const int c0 = t0 & ~(XCH - 1);
                if (t0 == c0) stage_columns(c0);
                const int t_end = min(ncols, c0 + XCH);
                v4f32 dt = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
                for (int rb = 0; rb < MR; ++rb) {
                    if (rb >= nrb) break;  // (wave-uniform)
                    Vec16<T> b[2];
                    b[0] = nxt[0];
                    b[1] = nxt[1];
                    if (rb + 1 < nrb)
                        fetch(nxt, t0, rb + 1);
                    else if (t0 + 16 < ncols)
                        fetch(nxt, t0 + 16, 0);
                    if (pending) emit();
                    if (fwd_en && !BSM_DBG(DBG_NO_FWD_HALF)) {
#pragma unroll
                        for (int j = 0; j < 2; ++j)
#pragma unroll
                            for (int e = 0; e < 2; ++e) {
                                const int wl = t0 - c0 + 2 * (4 * j + lk) + e;  // column of the staged slice
                                const float x1 = xsf[wl * 16 + comp];  // (components in the transposed order, as the x rows)
                                float x2 = xsf[wl * 16 + (comp ^ 1)];
                                x2 = (((comp & 1) == 0) != cjf) ? -x2 : x2;
                                facc32[rb] = __builtin_amdgcn_mfma_f32_16x16x4f32(x1, b[j].v[e].re, facc32[rb], 0, 0, 0);
                                facc32[rb] = __builtin_amdgcn_mfma_f32_16x16x4f32(x2, b[j].v[e].im, facc32[rb], 0, 0, 0);
                            }
                    }
                    if (trn_en && !BSM_DBG(DBG_NO_TRN_HALF)) {
#pragma unroll
                        for (int j = 0; j < 2; ++j)
#pragma unroll
                            for (int e = 0; e < 2; ++e) tile8[(2 * (4 * j + lk) + e) * 17 + ln] = b[j].v[e];
#pragma unroll
                        for (int q = 0; q < 4; ++q) {
                            const c64 u = tile8[ln * 17 + 4 * q + lk];
                            dt = __builtin_amdgcn_mfma_f32_16x16x4f32(fr1[rb * 4 + q], u.re, dt, 0, 0, 0);
                            dt = __builtin_amdgcn_mfma_f32_16x16x4f32(fr2[rb * 4 + q], u.im, dt, 0, 0, 0);
                        }
                    }
                }
                if (trn_en) {
#pragma unroll
                    for (int r = 0; r < 4; ++r) pd[r] = dt[r];
                    pyi = (t0 + ln < t_end) ? ixm[t0 + ln - c0] : -1;
                    pending = true;
                }
            }
            if (pending) emit();
        }
        if constexpr (MFR) {
            // one step = one row block (16 rows) of one column tile (16 columns = 16 / E strips): 16 / (4 E) loads of
            // 16 bytes per lane (lane = row ln, strip 4 j + lk), issued one step ahead; E MFMAs per load and half
            using V4 = typename std::conditional<MFR64, v4f64, v4f32>::type;
            constexpr int NLD = 4 / E;  // loads per lane and step: 2 (Float64), 1 (Float32)
            T *tileT = reinterpret_cast<T *>(tile);
            const int nrb = (m + 15) >> 4;
            auto fetch = [&](Vec16<T>(&b)[NLD], int t0, int rb) {
                const int row = rb * 16 + ln;
#pragma unroll
                for (int j = 0; j < NLD; ++j) {
                    const int sidx = t0 / E + 4 * j + lk;
                    if (row < m && sidx < nstrips && !BSM_DBG(DBG_NO_MATRIX)) {
                        b[j] = load_stream16(&vb[(uint32_t)(sidx * m + row)]);
                    } else {
#pragma unroll
                        for (int e = 0; e < E; ++e) b[j].v[e] = zero_of(T{});
                    }
                }
            };
            auto comp_of = [&](int r) { return MFR64 ? lk + 4 * r : 4 * r + lk; };  // accumulator row -> right-hand side
            T pd[4];
            int pyi = -1;
            bool pending = false;
            auto emit = [&]() {
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    const int kq = comp_of(r);
                    if (pyi >= 0 && kq < kact) {
                        T *yp = &y[pyi + kq * ldy];
                        if (flags & FLAG_RMW)
                            *yp += pd[r];
                        else if (!BSM_DBG(DBG_NO_GLOBAL_ATOMICS))
                            atomicAdd(yp, pd[r]);
                    }
                }
                pending = false;
            };
            Vec16<T> nxt[NLD];
            fetch(nxt, 0, 0);
            for (int t0 = 0; t0 < ncols; t0 += 16) {
                const int c0 = t0 & ~(XCH - 1);
                if (t0 == c0) stage_columns(c0);
                const int t_end = min(ncols, c0 + XCH);
                V4 dt = {0, 0, 0, 0};
#pragma unroll
                for (int rb = 0; rb < MR; ++rb) {
                    if (rb >= nrb) break;  // (wave-uniform)
                    Vec16<T> b[NLD];
#pragma unroll
                    for (int j = 0; j < NLD; ++j) b[j] = nxt[j];
                    if (rb + 1 < nrb)
                        fetch(nxt, t0, rb + 1);
                    else if (t0 + 16 < ncols)
                        fetch(nxt, t0 + 16, 0);
                    if (pending) emit();
                    if (fwd_en && !BSM_DBG(DBG_NO_FWD_HALF)) {
#pragma unroll
                        for (int j = 0; j < NLD; ++j)
#pragma unroll
                            for (int e = 0; e < E; ++e) {
                                const int wl = t0 - c0 + E * (4 * j + lk) + e;  // column of the staged slice
                                const T x1 = xs[wl * 16 + compA];
                                if constexpr (MFR64) facc[rb] = mfma16(x1, b[j].v[e], facc[rb]);
                                if constexpr (MFR32) facc32[rb] = mfma16(x1, b[j].v[e], facc32[rb]);
                            }
                    }
                    if (trn_en && !BSM_DBG(DBG_NO_TRN_HALF)) {
#pragma unroll
                        for (int j = 0; j < NLD; ++j)
#pragma unroll
                            for (int e = 0; e < E; ++e) tileT[(E * (4 * j + lk) + e) * 17 + ln] = b[j].v[e];
#pragma unroll
                        for (int q = 0; q < 4; ++q) dt = mfma16(rr[rb * 4 + q], tileT[ln * 17 + 4 * q + lk], dt);
                    }
                }
                if (trn_en) {
#pragma unroll
                    for (int r = 0; r < 4; ++r) pd[r] = dt[r];
                    pyi = (t0 + ln < t_end) ? ixm[t0 + ln - c0] : -1;
                    pending = true;
                }
            }
            if (pending) emit();
        }
    }
    if constexpr (MFA) {
        // The forward sums sit in the accumulators TRANSPOSED as well (A = the x slice, B = the tile): lane = (row ln of
        // the row block, lk), register r = component  lk + 4 r (ComplexF64) / 4 r + lk (ComplexF32: the slice enters
        // in transposed component order), i.e. Re and Im of two k for 16 consecutive rows per wave-instruction.
        // (real types, K = 16: a component is a right-hand side)
        using R = typename std::conditional<MF || MFR64, double, float>::type;
        constexpr bool M64 = MF || MFR64;  // the f64 accumulator map
        constexpr int CS = MFR ? 0 : 1;    // component -> k: comp >> CS; Re / Im: comp & CS
        auto comp_of = [&](int r) { return M64 ? lk + 4 * r : 4 * r + lk; };
        if (FWD && !(flags & (FLAG_DIRECT | FLAG_RMW))) {
            // atomic mode: every wave adds its own partial sums (alpha is in the slice already) -- contiguous runs
            // again instead of Re and Im of one k per instruction, no slab, no combine (a group's waves add separately;
            // coloured launches keep the combine: their plain read-modify-write is race-free between groups only)
            if (wd.npieces > 0 && (!(flags & FLAG_OPT) || (wd.first.kind & kKindHasOff)) && !BSM_DBG(DBG_NO_FWD_OUT)) {
#pragma unroll
                for (int rb = 0; rb < MR; ++rb) {
                    const int row = rb * 16 + ln;
                    if (rb * 16 >= m) break;
                    int yi = -1;
                    if (row < m) yi = row_index(wd, rows, row);
#pragma unroll
                    for (int r = 0; r < 4; ++r) {
                        const int cq = comp_of(r);
                        R val;
                        if constexpr (M64) val = facc[rb][r]; else val = facc32[rb][r];
                        if (yi >= 0 && (cq >> CS) < kact)
                            atomicAdd(reinterpret_cast<R *>(&y[yi + (cq >> CS) * ldy]) + (cq & CS), val);
                    }
                }
            }
            return true;
        }
        if (FWD) {
            // exclusive launches (plain stores, beta fused, groups combined in LDS by the caller): lane = row, K complex
            // sums -- through the dead x slice, 64 rows x 16 components, component n of row i at i * 16 + (n ^ s(i))
            R *sl = reinterpret_cast<R *>(xs);
            auto swz = [&](int row) { return M64 ? ((row >> 1) & 15) : (row & 15); };
#pragma unroll
            for (int rb = 0; rb < MR; ++rb) {
                const int row = rb * 16 + ln;
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    R val;
                    if constexpr (M64) val = facc[rb][r]; else val = facc32[rb][r];
                    sl[row * 16 + (comp_of(r) ^ swz(row))] = val;
                }
            }
            const int sw = swz(lane);
#pragma unroll
            for (int k = 0; k < K; ++k) {
                T a = zero_of(T{});
                if (lane < 16 * MR) {
                    if constexpr (MFR) {
                        a = sl[lane * 16 + (k ^ sw)];
                    } else {
                        a.re = sl[lane * 16 + ((2 * k) ^ sw)];
                        a.im = sl[lane * 16 + ((2 * k + 1) ^ sw)];
                    }
                }
                out[k] = a;
            }
        }
        return false;
    }
    return false;
}

template <typename T, int L, bool FWD, bool TRN, int K>
__global__ void __launch_bounds__(64 * kWavesPerWg, (MultiShape<T, L, TRN, K>::WGS))
    panel_kernel_multi(const WaveWork *__restrict__ waves, const uint4 *__restrict__ values,
                       const int *__restrict__ rows, const int *__restrict__ cols,
                       const T *__restrict__ x, long long ldx, T *__restrict__ y, long long ldy, T alpha,
                       T beta, int flags, unsigned wg_base) {
    using SH = MultiShape<T, L, TRN, K>;
    __shared__ __attribute__((aligned(16))) T xs[kWavesPerWg][FWD ? SH::XS : 1];
    __shared__ Vec16<T> tl[kWavesPerWg][TRN ? SH::TILE : 1];
    __shared__ int ixm[kWavesPerWg][SH::IXM];

    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int lane = threadIdx.x & 63;
    const WaveD wd = load_wave(waves + ((size_t)(blockIdx.x + wg_base) * kWavesPerWg + wave));
    const int work = wd.work;
    const int m = wd.m;

    T u[K];
#pragma unroll
    for (int k = 0; k < K; ++k) u[k] = zero_of(T{});
    bool fwd_done = false;  // the wave has added its forward sums to y itself (matrix-pipe path, accumulate mode)
    if (work == WORK_PANEL) {
        constexpr PathTag<SH::path> path{};
        if (m <= 8)
            fwd_done = panel_multi<T, L, 8, FWD, TRN, K>(path, wd, values, rows, cols, x, ldx, y, ldy, alpha, flags, lane, xs[wave], tl[wave], ixm[wave], u);
        else if (m <= 16)
            fwd_done = panel_multi<T, L, 16, FWD, TRN, K>(path, wd, values, rows, cols, x, ldx, y, ldy, alpha, flags, lane, xs[wave], tl[wave], ixm[wave], u);
        else if (m <= 32)
            fwd_done = panel_multi<T, L, 32, FWD, TRN, K>(path, wd, values, rows, cols, x, ldx, y, ldy, alpha, flags, lane, xs[wave], tl[wave], ixm[wave], u);
        else
            fwd_done = panel_multi<T, L, 64, FWD, TRN, K>(path, wd, values, rows, cols, x, ldx, y, ldy, alpha, flags, lane, xs[wave], tl[wave], ixm[wave], u);
    }
    const bool direct = (flags & FLAG_DIRECT) != 0;
    const bool sz = (flags & FLAG_STRONG_ZERO) != 0;
    const int kact = kact_of<K>(flags);
    if (FWD) {
        if (wd.wg_sync) {
            // a wave's staged x slice is dead once it has left its loop: reuse it as this wave's
            // part of the combine slab [wave][lane][k]
#pragma unroll
            for (int k = 0; k < K; ++k) xs[wave][lane * K + k] = u[k];
            __syncthreads();
        }
        if (work == WORK_PANEL && wd.lead && !fwd_done && !BSM_DBG(DBG_NO_FWD_OUT)) {
            for (int w2 = 1; w2 < wd.grp; ++w2)
#pragma unroll
                for (int k = 0; k < K; ++k) u[k] = add(u[k], xs[wave + w2][lane * K + k]);
            if (lane < m) {
                const int yi = row_index(wd, rows, lane);
#pragma unroll
                for (int k = 0; k < K; ++k) {
                    if (k >= kact) continue;
                    T *yp = &y[yi + k * ldy];
                    const T val = mul(alpha, u[k]);
                    if (direct) {
                        *yp = sz ? val : madd(val, beta, *yp);
                    } else if (flags & FLAG_RMW) {
                        *yp = add(*yp, val);
                    } else {
                        atomic_acc(yp, val);
                    }
                }
            }
        }
    }
    if (work == WORK_SCALE && direct) {
        const int cnt = wd.first.ncols;
        for (int r = lane; r < cnt; r += 64)
#pragma unroll
            for (int k = 0; k < K; ++k) {
                if (k >= kact) continue;
                T *yp = &y[wd.rbase + r + k * ldy];
                *yp = sz ? zero_of(T{}) : mul(beta, *yp);
            }
    }
}

// K right-hand sides per pass
template <typename T, int L, int K>
static hipError_t launch_typed_multi(const Product &p, int kact) {
    const DeviceImage &img = p.img;
    const bool opT = p.opT;
    const int strong_zero = p.strong_zero;
    hipStream_t stream = p.stream;
    const T *xd = (const T *)p.x;
    T *yd = (T *)p.y;
    const long long ldx = p.ldx, ldy = p.ldy;
    const T alpha = load_scalar<T>(p.alpha, 1.0), beta = load_scalar<T>(p.beta, 0.0);
    int flags = base_flags(opT, p.conj, strong_zero);
    if (kact < K) flags |= kact << FLAG_KACT_SHIFT;  // a padded batch: kact of the K slots carry columns
    const uint4 *values = (const uint4 *)img.d_values;
    const int *rows = (const int *)img.d_rows;
    const int *cols = (const int *)img.d_cols;
    auto panel = [&](auto fwd, auto trn, const WaveWork *waves, dim3 grid, unsigned wg_base) {
        hipLaunchKernelGGL((panel_kernel_multi<T, L, decltype(fwd)::value, decltype(trn)::value, K>), grid, dim3(64 * kWavesPerWg),
                           0, stream, waves, values, rows, cols, xd, ldx, yd, ldy, alpha, beta, flags, wg_base);
    };
    if (!opT && img.exclusive_fwd) {
        flags |= FLAG_DIRECT;
        if (img.nwg_total > 0)
            panel(std::true_type{}, std::false_type{}, (const WaveWork *)img.d_waves, dim3((unsigned)img.nwg_total), 0u);
        return hipGetLastError();
    }
    const YRange r = y_range(img, opT, p.zrange);
    if (r.hi > r.lo && (strong_zero || !is_one(beta)))
        launch_scale(p.vt, yd, ldy, r.lo, r.hi, &beta, strong_zero, (unsigned)kact, stream);
    if (!img.color_wg_ptr.empty()) flags |= FLAG_RMW;
    for_each_launch(img, true, [&](const WaveWork *waves, dim3 grid, unsigned wg_base) {
        with_halves(opT, img.has_off, [&](auto fwd, auto trn) { panel(fwd, trn, waves, grid, wg_base); });
    });
    return hipGetLastError();
}

// the instance of a MULTI batch: <L, width> (same-type pairs only: the plan names none for the others)
hipError_t launch_multi(const Product &p, const Batch &b) {
    return with_pair(p.img.dtype, p.vt, [&](auto t, auto s) {
        using T = decltype(t);
        if constexpr (std::is_same<decltype(s), T>::value) {
            if constexpr (kMfmaReal<T, 16>)
                if (b.width == 16) return launch_typed_multi<T, 4, 16>(p, b.kact);
            return b.width == 8 ? launch_typed_multi<T, 4, 8>(p, b.kact)
                   : b.L == 4   ? launch_typed_multi<T, 4, 4>(p, b.kact)
                                : launch_typed_multi<T, 8, 4>(p, b.kact);
        }
        return hipErrorInvalidValue;
    });
}

}  // namespace bsm
