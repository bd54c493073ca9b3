// bsm_families.h -- what the kernel families (one translation unit each; bsm_kernels.hip has the index) export to the
// batch loop of launch_mul.  Plain functions: each finds the <T, S> pair of the product itself (bsm_device.h: with_pair)
// and picks its own kernel instance from the batch.
#pragma once
#include "bsm_kernels.h"

namespace bsm {

// One batch of a product Y = alpha*op(A)*X + beta*Y (bsm_kernels.h: launch_mul has the meaning of every field): x and y
// point at the batch's first column, alpha / beta at one scalar of the vector type vt (null: 1 / 0).
struct Product {
    const DeviceImage &img;
    bool opT, conj;
    const void *x;
    long long ldx;
    void *y;
    long long ldy;
    const void *alpha, *beta;
    int strong_zero;
    hipStream_t stream;
    bool use_gather;
    const long long *zrange;
    ILWork *il;
    int vt;
};

hipError_t launch_one(const Product &p, const Batch &b);          // bsm_one.hip: panel_kernel (+ scale / gather)
hipError_t launch_multi(const Product &p, const Batch &b);        // bsm_multi.hip: panel_kernel_multi
hipError_t launch_interleaved(const Product &p, const Batch &b);  // bsm_il.hip: pack, panel_kernel_il, finish

// y[lo, hi) = beta * y (or 0) for ncols columns ldy apart, element type vt, beta: pointer to one element (bsm_one.hip:
// scale_kernel -- the `y .*= beta` pass in front of every accumulating product)
void launch_scale(int vt, void *y, long long ldy, long long lo, long long hi, const void *beta, int strong_zero, unsigned ncols,
                  hipStream_t stream);

#ifdef BSM_TRACE
hipError_t set_trace_one(void *buf);  // the g_trace copy of each family that stamps
hipError_t set_trace_il(void *buf);
#endif

}  // namespace bsm
