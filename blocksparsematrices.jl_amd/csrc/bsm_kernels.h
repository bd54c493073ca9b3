// bsm_kernels.h -- interface between the C ABI glue and the HIP kernels (bsm_kernels.hip: which family lives where).
#pragma once
#include <hip/hip_runtime_api.h>

#include <cstdint>
#include <vector>

#include "bsm_plan.h"

namespace bsm {

struct DeviceImage {
    int dtype = 1;
    int device = 0;
    long long nrows = 0, ncols = 0;
    long long own_lo = 0, own_hi = 0;  // 0-based [lo, hi) rows of y scaled by this handle
    void *d_values = nullptr, *d_rows = nullptr, *d_cols = nullptr;
    void *d_waves = nullptr;
    long long nwg_main = 0, nwg_total = 0;
    void *d_waves_multi = nullptr;  // coarser split of the same panels for the multi-RHS kernels (may be null)
    long long nwg_multi = 0;
    float mean_rows = 64.f;  // Analysis::mean_rows: fused fp32 products of short panels keep 4 loads per lane in flight
    float lane_fill = 1.f;  // Analysis::lane_fill: two right-hand sides go through a padded 4-column pass above 0.85
    int max_rows = 64;      // tallest row group of the image (the interleaved multi-RHS kernels: row blocks per panel)
    bool exclusive_fwd = false;
    bool has_off = false;  // SymmetricBlockMatrix off-diagonal pieces present
    long long device_bytes = 0;
    long long value_bytes = 0;  // packed matrix bytes (decides the cache policy of the matrix loads)
    std::vector<long long> color_wg_ptr;  // non-empty: coloured launches, plain read-modify-write
    // gather mode (BSM_ACC_GATHER): workspace + inverted indices for op N [0] and op T / C [1]
    void *d_ws = nullptr;
    // complex vectors under a real image (bsm_mul_cvec): the workspace in the complex type, (ws_slots + 8) * 2 * vs bytes,
    // allocated at the first complex gather product that holds the claim (bsm_capi.cpp); null until then
    void *d_wsc = nullptr;
    void *d_inv_ptr[2] = {nullptr, nullptr}, *d_inv_idx[2] = {nullptr, nullptr};
    long long ws_fbase = 0;
    // bsm_value_passes: streams of d_values enqueued by products of this image (launch_mul counts; relaxed atomic adds)
    mutable long long value_passes = 0;
};

// dst[0..n) += src[0..n);   y[0..n) = beta * y + r   (element type `dtype`, beta: pointer to one T)
hipError_t launch_vec_add(int dtype, void *dst, const void *src, long long n, hipStream_t stream);
hipError_t launch_vec_axpby(int dtype, void *y, const void *r, long long n, const void *beta, hipStream_t stream);

// Fused vector traffic of multi-device handles (peer-accessible devices): up to kMaxVecPieces sources per launch,
// each a virtual base pointer (element i of the global vector at base + i; column k of a multi-RHS batch
// `ld` elements further when strided) valid for indices [lo, hi).
constexpr int kMaxVecPieces = 8;
struct VecPieces {
    const void *base[kMaxVecPieces];
    long long lo[kMaxVecPieces], hi[kMaxVecPieces];
    int strided[kMaxVecPieces];
};
// dst[i + k * ld_dst] = piece(i)[k * ld_src] for every piece's range, K columns
hipError_t launch_vec_fetch(int dtype, void *dst, long long ld_dst, const VecPieces &pc, int npieces, long long ld_src, int K,
                            hipStream_t stream);
// y[i] = beta * y[i] + w[i] + sum of the pieces covering i, i in [lo, hi), K columns (w and the pieces: column stride
// ldw); accumulate_only: the sum goes back to w instead (more than kMaxVecPieces contributions)
hipError_t launch_vec_finish(int dtype, void *y, long long ldy, void *w, long long ldw, const VecPieces &pc, int npieces,
                             long long lo, long long hi, const void *beta, int strong_zero, int accumulate_only, int rezero, int K,
                             hipStream_t stream);

// y[lo_c + i] += base_c[i] for npieces <= kMaxVecPieces disjoint segments [lo_c, hi_c) of y, one launch
hipError_t launch_vec_add_segments(int dtype, void *y, const VecPieces &pc, int npieces, hipStream_t stream);

// Work arrays of the INTERLEAVED multi-RHS pass (bsm_il.hip: panel_kernel_il): X and the accumulated Y row-major,
// one 128-byte line per vector index.  Owned by the handle (bsm_capi.cpp: Claim), one product in flight.
struct ILWork {
    void *xr = nullptr;   // rows x 128 bytes: alpha * X, K-interleaved
    void *w = nullptr;    // rows x 128 bytes: the sums; zero between products (the finish pass zeroes behind its read)
    long long rows = 0;   // capacity of both, in vector entries
    bool w_clean = false; // w is known to be zero
};
// what the plan reads of a product of this image (bsm_plan.h).  Callers claim -- and allocate -- the work arrays only for
// products that wants_il_arrays(plan_input(..., false)) names, and pass arrays = true where launch_mul gets them
inline PlanInput plan_input(const DeviceImage &img, bool opT, int vt, long long K, bool arrays) {
    return {img.dtype, vt, img.nrows, img.ncols, img.mean_rows, img.lane_fill, img.max_rows, img.exclusive_fwd, img.has_off,
            !img.color_wg_ptr.empty(), opT, K, arrays};
}

// Enqueues Y = alpha*op(A)*X + beta*Y on `stream` for K right-hand sides, X (ldx) and Y (ldy) column-major device
// pointers.  No allocation, no synchronisation (graph-capturable).
// opT: apply the transposed operator of the image; conj: conjugate every stored entry.
// K == 1: the one-column kernels; use_gather: take the two-launch gather path (only if the image has a workspace).
// K > 1: A is streamed once per batch of <= 16 columns; il: the work arrays of the interleaved pass (null: not claimed).
// zrange = {lo, hi} (0-based, exclusive): the y entries the `y .*= beta` pass of the accumulate path covers instead of
// the image's own range (multi-device fan-out; ignored by exclusive forward images, whose coverage is part of the image)
// vt: the dtype code (BSM_F32 .. BSM_C128) of x, y, alpha, beta.  With the image's dtype it names the pair the product
// runs on: the image's own type (BSM_F64 / BSM_C128 for the mixed storage codes), or the complex type of a REAL image's
// precision (bsm_mul_cvec: use_gather then takes img.d_wsc, and il batches of 8 complex columns run the real interleaved
// pass over their 16 components).  Any other pair: hipErrorInvalidValue.
hipError_t launch_mul(const DeviceImage &img, bool opT, bool conj, long long K, const void *x, long long ldx, void *y,
                      long long ldy, const void *alpha, const void *beta, int strong_zero, hipStream_t stream,
                      bool use_gather, const long long *zrange, ILWork *il, int vt);

// rowcolvals(A): COO triples (1-based int64 rows / cols, values of the image's vector type) written from
// the packed device image; d_out_off[w] = first output slot of wave descriptor w (host prefix sum of
// m * ncols + m * #KIND_OFF columns)
hipError_t launch_export_coo(int dtype, const void *d_waves, long long nwaves, const void *d_out_off,
                             const void *d_values, const void *d_rows, const void *d_cols, void *orow, void *ocol,
                             void *oval, hipStream_t stream);

// bsm_submatrices / bsm_diag (bsm_extract.hip): entries of the operator added into caller windows, from the packed
// device image.  maps: the set (-1: not requested) and the position inside it of every row / column of the STORED
// operator (device arrays, nrows / ncols int32 each); d_table: one ExtractOut per set.  Entry (r, c) with rset[r] ==
// cset[c] = s goes to table[s].ptr[rpos[r] + ld * cpos[c]] (opT: [cpos[c] + ld * rpos[r]]; conj: conjugated).
// maps == nullptr: diag(A) -- every entry with r == c is added to d_diag[r].  The windows must be zero beforehand.
struct ExtractMaps {
    const int *rset, *rpos, *cset, *cpos;
};
struct ExtractOut {
    uint64_t ptr;  // device address of the window's first element (vector type of the image)
    long long ld;
};
static_assert(sizeof(ExtractOut) == 16, "ExtractOut must be 16 bytes");
hipError_t launch_extract(int dtype, const void *d_waves, long long nwaves, const void *d_values, const void *d_rows,
                          const void *d_cols, const ExtractMaps *maps, const void *d_table, void *d_diag, long long nrows,
                          long long ncols, bool opT, bool conj, hipStream_t stream);
// the ni x nj window of every set = 0: d_shape = {ni, nj} int64 pairs, vt the vector type, largest = max ni * nj
hipError_t launch_zero_windows(int vt, const void *d_table, const void *d_shape, long long nsets, long long largest,
                               hipStream_t stream);

// bsm_invert_blocks (bsm_invert.hip): d_table[0 .. count) = the blocks of ONE launch, one 256-thread workgroup each, all
// of one regime -- resident: n * n * sizeof(T) <= BSM_INVERT_LDS_BYTES, eliminated in LDS; else in place, n <= 1024 --
// and none larger than nmax, which sizes the launch's dynamic LDS (invert_lds).  d_info[id] = 0, or the 1-based step whose
// pivot was zero or not finite.  dtype: BSM_F32 .. BSM_C128.
struct InvertBlock {
    uint64_t ptr;  // device address of the block's first element
    long long ld;  // leading dimension, elements
    int n, id;     // order; position in the caller's arrays (info)
};
static_assert(sizeof(InvertBlock) == 24, "InvertBlock must be 24 bytes");
// byte offsets into the dynamic LDS of a launch whose largest block has order nmax (es: element bytes): the staged pivot
// row and column, the row swaps, the column order of the write-back and -- resident launches -- the block itself; the
// first 128 bytes hold the four records of the pivot search
struct InvertLds {
    int prow, pcol, piv, perm, mat, total;
};
__host__ __device__ inline InvertLds invert_lds(int nmax, int es, bool resident) {
    const int v = (nmax * es + 15) & ~15, w = (nmax * 4 + 15) & ~15;
    InvertLds l;
    l.prow = 128;
    l.pcol = l.prow + v;
    l.piv = l.pcol + v;
    l.perm = l.piv + w;
    l.mat = l.perm + w;
    l.total = l.mat + (resident ? nmax * nmax * es : 0);
    return l;
}
hipError_t launch_invert(int dtype, const void *d_table, long long count, int nmax, bool resident, void *d_info,
                         hipStream_t stream);

// executes Analysis::pack_plan on the device (blocks already in HBM): d_plan = PackChunk[nchunks],
// d_colpos = int32 placements (may be null when no chunk is scattered), es = stored element bytes, src_es = the caller's
// (= es, or 2 es for the mixed-precision dtypes: the values are rounded to the stored type as they are placed)
hipError_t launch_pack(int es, int src_es, const void *d_plan, long long nchunks, const void *d_colpos, void *d_values,
                       hipStream_t stream);

// synthetic operators generated in HBM (include/bsm_synth.h); d_desc = SynthBlock[nblocks]
struct SynthBlockDesc {
    uint64_t dst, stream;
    int32_t m, n, symmetrise, pad;
};
// bare streaming read of `bytes` at src (bsm_bench_stream): sink >= 8 KB of scratch, hop = optional table of one
// 64-byte record per wave whose first int64 is the wave's position (a dependent scalar load per wave)
hipError_t launch_stream_floor(const void *src, long long bytes, void *sink, const void *hop, hipStream_t stream);
hipError_t launch_synth_blocks(int dtype, const void *d_desc, long long nblocks, int tiles, hipStream_t stream);
hipError_t launch_synth_vector(int dtype, void *dst, long long n, unsigned long long stream_seed, hipStream_t stream);

}  // namespace bsm
