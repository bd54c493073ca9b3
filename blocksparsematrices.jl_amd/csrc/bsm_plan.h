// bsm_plan.h -- which kernel takes the next columns of a product: the one place the multi-column policy lives.  Plain
// C++ (no device, no handle): launch_pair (bsm_kernels.hip) executes what next_batch names, bsm_capi.cpp / bsm_dist.cpp
// ask wants_il_arrays before they claim the work arrays, tests/test_plan_cpu.py pins the table.
#pragma once

// Compile-time choices the plan reads and the kernels are built for (make variant EXTRA=-D...: both see the same value)
#ifndef BSM_MFMA_C128  // ComplexF64, 8 columns: on the matrix pipe (bsm_multi.hip: kMfmaPath)
#define BSM_MFMA_C128 1
#endif
#ifndef BSM_MFMA_C64  // ComplexF32 likewise (kMfmaPath32)
#define BSM_MFMA_C64 1
#endif
#ifndef BSM_MFMA_REAL  // real types, 16 columns: on the matrix pipe (kMfmaReal)
#define BSM_MFMA_REAL 1
#endif
#ifndef BSM_C64_L
#define BSM_C64_L 4
#endif
// (developer builds: loads per lane of the fused kernels of the other element types)
#ifndef BSM_F32_L
#define BSM_F32_L 4
#endif
#ifndef BSM_F64_L
#define BSM_F64_L 8
#endif
#ifndef BSM_C128_L
#define BSM_C128_L 8
#endif

namespace bsm {

// The environment knobs of the policy, read once per process: BSM_MULTI_IL (default 1), BSM_MFMA_MIN_COLS (3),
// BSM_IL_REAL_MIN_COLS (5), BSM_IL_MIXED_MIN_COLS (clamped to 2 .. 8), BSM_MFMA_REAL_MIN_COLS, BSM_IL_XCD (the last
// three 0 / 0 / -1 when unset: the default depends on the image)
struct PlanKnobs {
    int multi_il, mfma_min_cols, il_real_min_cols, il_mixed_min_cols, mfma_real_min_cols, il_xcd;
};
const PlanKnobs &plan_knobs();

// What the policy reads of a product: the image's traits (bsm_kernels.h: plan_input), the op, the dtype code vt of the
// vectors, the total column count K, and whether the interleaved pass's work arrays are at hand.
struct PlanInput {
    int dtype, vt;
    long long nrows, ncols;
    float mean_rows, lane_fill;
    int max_rows;
    bool exclusive_fwd, has_off, colored, opT;
    long long K;
    bool arrays;
};

// One launch group of a product: `kact` columns on the kernels of `width` columns (the K / KK template argument) -- the
// interleaved pass (nrb: its row-block instance, 2 / 4; runs of xcd_run workgroups per XCD, 0: plain order), the
// multi-RHS kernels or the one-column kernels (L: loads per lane in flight)
struct Batch {
    enum Kind { IL, MULTI, ONE } kind;
    int width, L, kact, nrb, xcd_run;
};

// The batch that takes the columns from `taken` (< in.K) on, for a pair launch_mul runs.  A function of the columns left
// and of `in` alone -- no allocation, no lock; one column (K = 1) is answered before anything else is looked at.
Batch next_batch(const PlanInput &in, long long taken);
// whether the product uses the work arrays: its plan WITH them contains an IL batch
bool wants_il_arrays(PlanInput in);

}  // namespace bsm
