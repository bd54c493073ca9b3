// bsm_plan.cpp -- the multi-column policy (bsm_plan.h): thresholds, their measurements and the knobs that override them.
#include "bsm_plan.h"

#include <algorithm>
#include <climits>
#include <cstdlib>

#include "../../include/bsm_rocm.h"

namespace bsm {

// BSM_MULTI_IL: 0 = never, 1 = automatic (default: images that accumulate with atomics -- short scattered panels, mean
// group height below 32, in every element type; ComplexF64 / ComplexF32 from BSM_MFMA_MIN_COLS columns on, real types
// from BSM_IL_REAL_MIN_COLS), 2 = every image that accumulates with atomics (A / B)
// BSM_MFMA_MIN_COLS, default 3: (BEM fixture x 4: 362 us padded against 486 us through the 4-column kernel)
// BSM_IL_REAL_MIN_COLS, default 5:
//   (8 components per index from 5 columns on: BEM fp64 x 8 318 -> 202 us, C3 x 8 256 -> 217 us; 4 columns stay on the
//   vector kernels: BEM 194 us, C3 195 us against ~ 200 / 217)
static int env_int(const char *name, int unset) {
    const char *e = std::getenv(name);
    return e ? std::atoi(e) : unset;
}
const PlanKnobs &plan_knobs() {
    static const PlanKnobs knobs = {env_int("BSM_MULTI_IL", 1), env_int("BSM_MFMA_MIN_COLS", 3), env_int("BSM_IL_REAL_MIN_COLS", 5),
                                    std::getenv("BSM_IL_MIXED_MIN_COLS") ? std::min(std::max(env_int("BSM_IL_MIXED_MIN_COLS", 0), 2), 8) : 0,
                                    env_int("BSM_MFMA_REAL_MIN_COLS", 0), env_int("BSM_IL_XCD", -1)};
    return knobs;
}

static bool is_cvec(int dtype, int vt) { return (dtype == BSM_F32 && vt == BSM_C64) || (dtype == BSM_F64 && vt == BSM_C128); }

// fewest columns of a mixed-storage product that take the pass (a batch of 8 or more always does).  What the pass
// replaces is nrhs one-column products, i.e. nrhs streams of the matrix, against ONE stream and two vector sweeps.
// Pass / nrhs one-column products, us (docs/experiments_r09.md):
//                          x 2          x 3          x 4          x 5
//   C2 (forward VBCRS)     31.0 / 20.2  30.5 / 30.2  30.6 / 40.3  31.0 / 50.1
//   1 GB forward VBCRS     265 / 213    270 / 319    274 / 426    282 / 532
//   ... op T               259 / 241    263 / 362    268 / 483    279 / 603
//   C3 (fused symmetric)   184 / 194    184 / 291    184 / 388    184 / 484
//   tiled BEM, complex     265 / 286    267 / 429    270 / 572    353 / 715
// Symmetric operators (both halves in every product) take the pass from two columns on; on the others two columns stay
// two one-column products and three take the pass.  BSM_IL_MIXED_MIN_COLS (2 .. 8) overrides both.
static int il_mixed_min_cols(const PlanInput &in, const PlanKnobs &kn) {
    return kn.il_mixed_min_cols ? kn.il_mixed_min_cols : (in.has_off ? 2 : 3);
}

// The fewest columns LEFT that take the interleaved pass in a product of in.K > 1 columns; kNever: the product has no
// IL batch.  (A product of fewer columns than the threshold has none either: it never has that many left.)
constexpr long long kNever = LLONG_MAX;
static long long il_least(const PlanInput &in, const PlanKnobs &kn) {
    if (!in.arrays || kn.multi_il == 0) return kNever;
    if (in.colored) return kNever;   // coloured launches keep their bitwise reproducible read-modify-write
    if (std::max(in.nrows, in.ncols) >= (1ll << 30)) return kNever;  // (staged entries carry two role bits)
    // complex vectors under a real image: the pass over 2 x nrhs real components streams the matrix once where the
    // alternative is nrhs one-column products -- every image class takes it, exclusive forward ones included.
    if (is_cvec(in.dtype, in.vt)) return 2;
    // Mixed storage (values in single precision under double vectors): the same alternative, the same answer -- from
    // il_mixed_min_cols columns on
    if (in.vt != in.dtype) return il_mixed_min_cols(in, kn);
    if (!in.opT && in.exclusive_fwd) return kNever;   // plain stores with beta fused: nothing to gain
    // automatic: short scattered panels, and tall panels where the product is FUSED (symmetric operators: both halves, the
    // transposed one all atomics -- C3 x 16 377 -> 305 us, x 8 264 -> 220, C5 slice x 16 1607 -> 1131; the C3 structure with
    // complex entries, tools/c3_complex.py: ComplexF64 x 8 175 -> 138 us, ComplexF32 76 -> 63).  Forward-only products of
    // tall panels keep their kernels: on the C4 slice (128 x 128 fp32 blocks of one GPU of eight, vectors of the full 2 M
    // entries) the pass's two vector sweeps cost more than it saves (x 8 363 -> 457 us, x 16 453 -> 562).
    if (!(kn.multi_il == 2 || in.mean_rows < 32.f || in.has_off)) return kNever;
    return in.vt >= BSM_C64 ? kn.mfma_min_cols : kn.il_real_min_cols;
}

// loads per lane in flight of the one-column kernels.  Every one-column launch takes it -- single products and the
// single columns a multi-RHS product ends with.
//   S = T: L = 4 where it was measured faster, on products that are fused (symmetric operators, accumulating), 8
//     everywhere else.  complex64: 61 VGPRs, 8 waves per SIMD; with 8 the fused instance needs 93-95 (5 waves): tiled
//     BEM fixture 105.9 -> 95.1 us (profiles/r04_c64_l4.txt).  fp32, SHORT panels only: tiled BEM fixture 48.6 -> 46.5
//     us; 16-256-row operators lose 3-5 % with it and keep 8 (profiles/r04_fused_loads_per_lane.txt)
//   S != T: 4 in every direction.  Mixed storage (S = float / c64 stored, T = double / c128 vectors): a lane's 4 strips
//     hold 16 fp64 / 8 complex128 values after widening -- what the fp64 / complex128 instances of L = 8 hold -- and the
//     forward instance with 8 loads needed 96 VGPRs and still spilled (the widened x reads of 8 strips: 64 VGPRs), i.e.
//     5 resident waves against 6-8 with 4.  Complex vectors under a real image (T = c128 / c64, S = double / float): a
//     lane's 4 strips meet 8 complex128 / 16 complex64 x entries.
static Batch one_column(const PlanInput &in) {
    int L = 4;
    if (in.vt == in.dtype) {
        L = in.vt == BSM_F32 ? BSM_F32_L : in.vt == BSM_F64 ? BSM_F64_L : in.vt == BSM_C64 ? BSM_C64_L : BSM_C128_L;
        const bool fused = in.has_off && !in.exclusive_fwd && (in.vt != BSM_F32 || in.mean_rows < 32.f);
        if (!fused) L = 8;
    }
    return {Batch::ONE, 1, L, 1, 0, 0};
}

// The products of one (vector type T, stored type S) pair for K right-hand sides, in this order:
//   1. the interleaved pass over the image's own type S, where il_least says so (and its work arrays are claimed) --
//      every pair has one;
//   2. same-type images only: the multi-RHS kernels;
//   3. the columns left, one at a time on the one-column kernels.
Batch next_batch(const PlanInput &in, long long taken) {
    // (one column: the one-column kernels, whatever the thresholds say)
    if (in.K == 1) return one_column(in);
    const PlanKnobs &kn = plan_knobs();
    const long long left = in.K - taken;
    const bool real = in.vt <= BSM_F64;
    // The interleaved pass: complex types in batches of 8 columns, real types of 16, then one padded remainder (at most
    // half a batch left: 8 components per index, 64-byte lines).  Complex vectors under a real image: the 2 x 8 (2 x 4)
    // real components of 8 (4) complex columns on the real pass, from 2 columns on.  Mixed storage: the batches of the
    // vector type over the single-precision image, a remainder from il_mixed_min_cols columns on.
    if (left >= il_least(in, kn)) {
        const int KK = real ? 16 : 8, kact = (int)std::min<long long>(KK, left);
        // BSM_IL_XCD = R: XCD-aware workgroup order, runs of R consecutive workgroups per XCD (0: plain order).  Default:
        // 16 for operators with tall panels (C3 x 16 312 -> 262 us -- neighbouring 64-row panels read the same 9 x 64
        // lines of Xr, L2 hits 0.5 M -> of 9.5 M read requests with the plain order; R = 4 ... 64 alike), plain for
        // short scattered panels (the tiled BEM fixture: +-0, 367 / 204 / 359 us against 374 / 208 / 352)
        const bool small = in.max_rows <= 32;
        const int xcd = kn.il_xcd >= 0 ? kn.il_xcd : (small ? 0 : 16);
        // (tall panels: all row blocks of the next 16 columns in flight -- il_panel's DEEP form, worth 1-6 % over one
        // step ahead with the XCD-aware order, profiles/r05_il_tall_panels.txt)
        return {Batch::IL, kact <= KK / 2 ? KK / 2 : KK, 0, kact, small ? 2 : 4, xcd};
    }
    // (mixed storage and complex vectors under a real image: no multi-RHS kernels)
    if (in.vt != in.dtype) return one_column(in);
    // batches of 8, then 4, then single columns: A is streamed once per batch.  The 8-column
    // kernels keep L = 4 loads per lane in flight instead of 8: with 8 accumulators and 8 x values
    // per lane the registers, i.e. the resident waves, are worth more than the deeper load queue
    // (fp64 fused: 143 -> 103 VGPRs; C3 3.0x -> 3.3x, 8-28-row blocks 2.0x -> 2.4x over 8 products).
    // A remainder of 5-7 columns is one PADDED 8-column pass and 3 columns one padded 4-column pass (the idle
    // slots repeat the last column and are never written): a pass costs 1.2-1.8 (8) / 1.1-1.4 (4) single products
    // on the large operators, 3.9 / 3.0 on the BEM fixture -- never more than the 4 + singles it replaces; two
    // columns stay two single products (a 4-column pass over 3-28-row panels costs three).
    // real types, 9 columns and more: batches of 16 on the matrix pipe (N = 16 of v_mfma_*_16x16x4: kMfmaReal), a
    // remainder of 9-15 as one padded pass (C3 x 16: 374 us against 2 x 264, C4 slice 442 against 2 x 364; x 9: one
    // padded pass against an 8-column pass + a single product).  Short scattered panels (the BEM fixture: mean group
    // height below 32) gain nothing below 15 columns: their passes are bound by the x gather and the atomics, which
    // grow with the padded width (fp64 x 16: 615 us against 2 x 320).  BSM_MFMA_REAL_MIN_COLS overrides (17: off).
    auto multi = [](int width, int L, long long cols) { return Batch{Batch::MULTI, width, L, (int)std::min<long long>(cols, width), 0, 0}; };
    if (BSM_MFMA_REAL && real) {
        const int mr_min = kn.mfma_real_min_cols ? kn.mfma_real_min_cols : (in.mean_rows < 32.f ? 15 : 9);
        if (left >= 16 ? mr_min <= 16 : left >= mr_min) return multi(16, 4, left);
    }
    if (left >= 8) return multi(8, 4, left);
    // (ComplexF64: the 8-column pass runs on the matrix pipe -- a padded pass beats the 4-column register kernel
    // from 3 columns on: BSM_MFMA_MIN_COLS)
    const bool mfma8 = (in.vt == BSM_C128 && BSM_MFMA_C128) || (in.vt == BSM_C64 && BSM_MFMA_C64);
    if (left >= (mfma8 ? kn.mfma_min_cols : 5)) return multi(8, 4, left);
    // (two columns: a padded 4-column pass where the row groups fill their lanes -- 1.1-1.3 single products on C3 /
    // C4 -- and two single products over short panels, where the pass would cost 2.6)
    if (left >= 3 || (left == 2 && in.lane_fill >= 0.85f)) {
        // (real arithmetic and a transposed half in the product: L = 4, i.e. the tile-pipelined kernels -- BEM fp64
        // x 4 249 -> 211 us, C3 / C5 +-0; forward-only launches and complex: 8 loads per lane on the register path,
        // C4 slice x 4 1.10 vs 1.16 single products with L = 4)
        const bool fwd_only = !in.opT && (in.exclusive_fwd || !in.has_off);
        // (ComplexF64: L = 4 on the register path, BEM x 4 518 -> 490 us)
        return multi(4, (real || in.vt == BSM_C128) && !fwd_only ? 4 : 8, left);
    }
    return one_column(in);
}

bool wants_il_arrays(PlanInput in) {
    in.arrays = true;
    for (long long k = 0; k < in.K;) {
        const Batch b = next_batch(in, k);
        if (b.kind == Batch::IL) return true;
        k += b.kact;
    }
    return false;
}

}  // namespace bsm

// test hook (unexported in the header, like bsm_debug_move_image_array): the batches of a product of K columns of a pair
// launch_mul runs, 6 ints each (kind, width, L, kact, nrb, xcd_run) into out[0 .. 6 cap); flags: 1 exclusive_fwd, 2
// has_off, 4 coloured, 8 opT, 16 work arrays at hand.  *wants = wants_il_arrays.  Returns the number of batches
extern "C" int bsm_debug_plan(int dtype, int vt, long long nrows, long long ncols, double mean_rows, double lane_fill, int max_rows,
                              int flags, long long K, int *out, int cap, int *wants) {
    const bsm::PlanInput in{dtype, vt, nrows, ncols, (float)mean_rows, (float)lane_fill, max_rows, (flags & 1) != 0, (flags & 2) != 0,
                            (flags & 4) != 0, (flags & 8) != 0, K, (flags & 16) != 0};
    *wants = bsm::wants_il_arrays(in);
    int n = 0;
    for (long long k = 0; k < K; ++n) {
        const bsm::Batch b = bsm::next_batch(in, k);
        const int rec[6] = {b.kind, b.width, b.L, b.kact, b.nrb, b.xcd_run};
        if (n < cap) std::copy(rec, rec + 6, out + 6 * n);
        k += b.kact;
    }
    return n;
}
