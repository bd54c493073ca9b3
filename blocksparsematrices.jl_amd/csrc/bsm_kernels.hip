// bsm_kernels.hip -- the product entry point of the hand-written gfx950 (CDNA4, wave64) kernels of the block-sparse
// mat-vec engine, and the index of where they live.  One translation unit per kernel family (Makefile: KSRC), all of
// them streaming the STRIP-packed pieces of bsm_layout.h:
//
//   bsm_device.h    what several families use: element types and arithmetic, load_stream16, the DPP / butterfly
//                   reductions, the launch flags, PieceD / WaveD / load_wave, col_decode / row_index, and the host
//                   frame of every launcher (scalars, base_flags, y_range, for_each_launch, with_halves,
//                   stream_policy, with_pair)
//   bsm_families.h  what the families export to this file: Product, launch_one / _multi / _interleaved, launch_scale
//   bsm_one.hip     one column: run_panel, panel_kernel, scale_kernel, gather_kernel, launch_typed
//   bsm_multi.hip   4 / 8 / 16 columns per pass: MultiShape, PanelSetup, panel_multi (one overload per path: register,
//                   tile pipeline, matrix pipe), panel_kernel_multi, launch_typed_multi
//   bsm_il.hip      the interleaved multi-RHS pass: ILT, il_panel, panel_kernel_il, il_pack_kernel, il_finish_kernel,
//                   launch_il
//   bsm_util.hip    fan-out vector helpers, COO export, pack / pack-convert, synth, the stream floor
//   (bsm_refill.hip: bsm_update_blocks, outside the build id)
//
// Here: launch_mul / launch_pair, the loop over the batches bsm_plan.cpp names.
#include "bsm_device.h"
#include "bsm_families.h"

namespace bsm {

// The products of one (T, S) pair -- T: the type of x, y, alpha, beta; S: the type the image stores -- for K right-hand
// sides: executes the batches bsm_plan.cpp names, A streamed once per batch (the gather workspace only when K = 1).
// p: the whole product (x, y at column 0; il: the work arrays of the interleaved pass, null when not claimed).
template <typename T, typename S> static hipError_t launch_pair(Product p, long long K) {
    if constexpr (kCvec<T, S>) p.conj = false;  // (op C of a real image is op T: `conj` has nothing to act on)
    const PlanInput in = plan_input(p.img, p.opT, p.vt, K, p.il != nullptr);
    const T *xd = (const T *)p.x;
    T *yd = (T *)p.y;
    p.use_gather = p.use_gather && K == 1;
    for (long long k = 0; k < K;) {
        const Batch b = next_batch(in, k);
        p.x = xd + k * p.ldx;
        p.y = yd + k * p.ldy;
        count_value_pass(p.img);
        const hipError_t e = b.kind == Batch::IL      ? launch_interleaved(p, b)
                             : b.kind == Batch::MULTI ? launch_multi(p, b)
                                                      : launch_one(p, b);
        if (e != hipSuccess) return e;
        k += b.kact;
    }
    return hipSuccess;
}

hipError_t launch_mul(const DeviceImage &img, bool opT, bool conj, long long K, const void *x, long long ldx, void *y,
                      long long ldy, const void *alpha_p, const void *beta_p, int strong_zero, hipStream_t stream,
                      bool use_gather, const long long *zrange, ILWork *il, int vt) {
    const Product p{img, opT, conj, x, ldx, y, ldy, alpha_p, beta_p, strong_zero, stream, use_gather, zrange, il, vt};
    return with_pair(img.dtype, vt, [&](auto t, auto s) { return launch_pair<decltype(t), decltype(s)>(p, K); });
}

#ifdef BSM_TRACE
extern "C" int bsm_debug_set_trace(void *buf) {
    const hipError_t e = set_trace_one(buf);
    return (int)(e != hipSuccess ? e : set_trace_il(buf));
}
#endif

}  // namespace bsm
