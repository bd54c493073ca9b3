// bsm_refill.hip -- refill_kernel (bsm_update_blocks, include/bsm_rocm.h): new values into an existing image.
// Kept out of the product kernel units (bsm_kernels.hip has their index): the build id (Makefile BUILD_ID) names the kernels and schedule of the PRODUCTS, and a
// refill changes neither.
#include <hip/hip_runtime.h>

#include "bsm_refill.h"

namespace bsm {

// ========================================================================================
// refill (bsm_update_blocks): new VALUES into an existing image through the replayable plan of the analysis
// (Analysis::refill).  Written for the store side: a lane assembles a whole 16-byte unit of the strip layout
// (E columns of one row) and stores it with one 16-byte store, consecutive lanes consecutive units, so a wave
// writes 1 KB contiguous per instruction; its E loads walk down the block's columns (consecutive lanes =
// consecutive rows).  A wave takes one item: up to 64 segments (strip / column ranges of chunks) of at most
// kRefillItemUnits units in all, so a run of small chunks shares a wave instead of one workgroup each.  The
// lane of a unit finds its segment by a binary search over the segments' prefix sums, held one per lane
// (shuffles, no LDS).  Units shared with a neighbouring chunk (woff not a multiple of E) and scattered
// placements are written element by element: no two waves ever write the same bytes, the strip tails are
// never touched.  Transposed sources (the transposed image) map consecutive lanes along the stored row
// instead, so that the loads stay contiguous there.
// ========================================================================================
template <typename U>
__global__ void __launch_bounds__(256) refill_kernel(const RefillChunk *__restrict__ chunks, const int *__restrict__ colpos,
                                                     const RefillSeg *__restrict__ segs, const RefillItem *__restrict__ items,
                                                     const int32_t *__restrict__ list, long long nitems,
                                                     const RefillSrc *__restrict__ table, U *__restrict__ values) {
    constexpr int E = 16 / (int)sizeof(U);
    const int lane = threadIdx.x & 63;
    const long long w = (long long)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (w >= nitems) return;  // whole waves leave: the shuffles below only ever run with all 64 lanes
    const RefillItem it = items[list ? list[w] : w];
    // lane j < seg_count holds segment j: its chunk, its source and the exclusive prefix of the units
    RefillSeg sg{0, 0, 0, 0};
    RefillChunk ch{};
    RefillSrc sr{0, 0};
    if (lane < it.seg_count) {
        sg = segs[it.seg_first + lane];
        ch = chunks[sg.chunk];
        sr = table[ch.id];
    }
    int pre = sg.units;  // inclusive scan over the lanes
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        const int t = __shfl_up(pre, d, 64);
        if (lane >= d) pre += t;
    }
    const int total = __shfl(pre, 63, 64);
    pre -= sg.units;  // exclusive
    for (int base = 0; base < total; base += 64) {
        const int u = base + lane;
        // segment of unit u: the last lane j < seg_count with pre_j <= u (binary search over the lanes)
        int j = 0;
#pragma unroll
        for (int step = 32; step >= 1; step >>= 1) {
            const int pj = __shfl(pre, j + step, 64);
            if (j + step < it.seg_count && pj <= u) j += step;
        }
        const int r = u - __shfl(pre, j, 64);
        const int lo = __shfl(sg.lo, j, 64), hi = __shfl(sg.hi, j, 64);
        const int mc = __shfl((int)ch.mc, j, 64), trans = __shfl((int)ch.trans, j, 64);
        const int ra = __shfl(ch.ra, j, 64), n = __shfl(ch.n, j, 64), woff = __shfl(ch.woff, j, 64);
        const int perm_off = __shfl(ch.perm_off, j, 64);
        const unsigned long long dst_unit = __shfl((unsigned long long)ch.dst_unit, j, 64);
        const U *__restrict__ src = reinterpret_cast<const U *>(__shfl((unsigned long long)sr.ptr, j, 64));
        const long long ld = __shfl((long long)sr.ld, j, 64);
        if (u >= total) continue;
        U *__restrict__ panel = values + dst_unit * (uint64_t)E;
        if (perm_off >= 0) {  // scattered placement: element (i, w) of the chunk, rows fastest
            const int wc = lo + r / mc, i = r % mc;
            const int q = colpos[perm_off + wc];
            const U v = trans ? src[(int64_t)wc + (int64_t)(ra + i) * ld] : src[(int64_t)(ra + i) + (int64_t)wc * ld];
            panel[((int64_t)(q / E) * mc + i) * E + (q % E)] = v;
            continue;
        }
        int s, i;
        if (trans) {  // lanes along the stored row
            const int ns = hi - lo;
            s = lo + r % ns;
            i = r / ns;
        } else {
            s = lo + r / mc;
            i = r % mc;
        }
        const int w0 = s * E - woff;  // block column of slot 0 of this unit
        const int e_lo = max(0, -w0), e_hi = min(E, n - w0);
        U v[E];
#pragma unroll
        for (int e = 0; e < E; e++) {
            const int we = min(max(w0 + e, 0), n - 1);  // clamped: slots outside the block are not stored
            v[e] = trans ? src[(int64_t)we + (int64_t)(ra + i) * ld] : src[(int64_t)(ra + i) + (int64_t)we * ld];
        }
        U *d = panel + ((int64_t)s * mc + i) * E;
        if (e_lo == 0 && e_hi == E) {
            uint4 q;
            __builtin_memcpy(&q, v, 16);
            *reinterpret_cast<uint4 *>(d) = q;
        } else {
#pragma unroll
            for (int e = 0; e < E; e++)
                if (e >= e_lo && e < e_hi) d[e] = v[e];
        }
    }
}

hipError_t launch_refill(int es, const void *d_chunks, const void *d_colpos, const void *d_segs, const void *d_items,
                         const int32_t *d_list, long long nitems, const RefillSrc *d_src, void *d_values, hipStream_t stream) {
    if (nitems <= 0) return hipSuccess;
    const dim3 grid((unsigned)((nitems + 3) / 4)), block(256);
#define BSM_REFILL(U)                                                                                                  \
    hipLaunchKernelGGL((refill_kernel<U>), grid, block, 0, stream, (const RefillChunk *)d_chunks, (const int *)d_colpos, \
                       (const RefillSeg *)d_segs, (const RefillItem *)d_items, d_list, nitems, d_src, (U *)d_values)
    if (es == 4)
        BSM_REFILL(uint32_t);
    else if (es == 8)
        BSM_REFILL(uint64_t);
    else if (es == 16)
        BSM_REFILL(uint4);
    else
        return hipErrorInvalidValue;
#undef BSM_REFILL
    return hipGetLastError();
}

}  // namespace bsm
