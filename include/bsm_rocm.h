/* bsm_rocm.h -- C ABI of libbsmrocm.so: the MI355X (gfx950) block-sparse mat-vec engine.
 *
 * Drop-in boundary for ONE hot path of djukic14/BlockSparseMatrices.jl: the
 * `LinearMaps._unsafe_mul!(y, A, x[, alpha, beta])` methods of its three storage types
 * (and their Adjoint/Transpose wrappers) plus the constructors that feed them.
 * The reference is pure Julia and has no FFI; a Julia maintainer binds these entry
 * points with `ccall` from methods of the same names (INTEGRATION.md shows the stub).
 *
 * Conventions (chosen so a Julia caller passes its data untouched):
 *   - every index is 1-BASED int64 (Julia Int);
 *   - a block is a column-major m x n array with leading dimension ld (a Julia Matrix);
 *   - `blocks` is an array of nblocks pointers (pointer.(blocks) of a Vector{Matrix});
 *   - *_create COPIES everything into library-owned device memory (repacked for
 *     coalesced 16-byte lane loads); the caller may free its arrays afterwards;
 *   - all functions return 0 on success, a negative bsm_status otherwise, never throw;
 *     bsm_last_error() returns a thread-local message for the last failure;
 *   - a handle's STRUCTURE is fixed at creation (block positions, shapes, index lists, options);
 *     its VALUES can be replaced in place with bsm_update_blocks, the counterpart of the reference
 *     holding the caller's blocks by reference.  Concurrent bsm_mul calls with distinct y (and
 *     distinct streams) are legal.
 */
#ifndef BSM_ROCM_H
#define BSM_ROCM_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct bsm_matrix_s *bsm_matrix_t;

typedef enum {
    BSM_OK = 0,
    BSM_ERR_INVALID = -1,   /* bad argument (null pointer, negative size, index out of range) */
    BSM_ERR_UNSUPPORTED = -2,
    BSM_ERR_DEVICE = -3,    /* HIP runtime error, or no device image (analysis-only handle) */
    BSM_ERR_ALLOC = -4
} bsm_status;

/* element type T of blocks, x, y, alpha, beta -- and, for the two MIXED-PRECISION codes, the type S the device image
 * stores the values in:
 *   BSM_F64_F32  (4): blocks, x, y, alpha, beta are double, the image stores float;
 *   BSM_C128_C64 (5): blocks, x, y, alpha, beta are complex double, the image stores complex float.
 * Every product is bound by the bytes of the value stream; a mixed handle streams half of them and keeps the vectors
 * and every sum in double precision.  Each entry is rounded ONCE, when the image is packed (host or device blocks
 * alike, bit-identical): the IEEE round-to-nearest-even cast of numpy's astype(float32) / astype(complex64) --
 * subnormals are kept, magnitudes beyond the float range become +-inf.  The image then has exactly the layout of a
 * BSM_F32 / BSM_C64 handle of the rounded blocks.  In a product each 16-byte lane load delivers 16 / sizeof(S) stored
 * values, which are widened in registers and combined with x by double-precision FMAs; partial sums, LDS windows,
 * atomics and the gather workspace are double.  All five *_create functions accept the codes; bsm_mul takes every
 * op, accumulate mode and transpose_image setting.
 * bsm_mul_multi streams the single-precision image ONCE per batch of 16 double (8 complex double) columns: the
 * interleaved pass over the stored type with double arithmetic (see bsm_mul_multi).
 * What a mixed handle does NOT offer:
 *   - bsm_options.ctx (multi-device handles): BSM_ERR_UNSUPPORTED;
 *   - bsm_update_blocks: BSM_ERR_UNSUPPORTED (create a new handle from the new blocks);
 *   - bsm_vec_add_segments takes vector types only: the mixed codes are BSM_ERR_INVALID there. */
typedef enum { BSM_F32 = 0, BSM_F64 = 1, BSM_C64 = 2, BSM_C128 = 3, BSM_F64_F32 = 4, BSM_C128_C64 = 5 } bsm_dtype;

/* which operator of A is applied: A, transpose(A), A' -- the reference's
 * LinearMaps.TransposeMap / AdjointMap wrappers (src/blockmatrix.jl:154-160,200-206,
 * src/symmetricblockmatrix.jl:345-365, src/vbcrs.jl:298-354) */
typedef enum { BSM_OP_N = 0, BSM_OP_T = 1, BSM_OP_C = 2 } bsm_op;

/* where x and y live */
typedef enum { BSM_MEM_HOST = 0, BSM_MEM_DEVICE = 1 } bsm_memspace;

/* reference `scheduler=` keyword: SerialScheduler() gives the single colour
 * [1:nblocks] (src/blockmatrix.jl:91-92), anything else colours the blocks
 * (src/blockmatrix.jl:94-98, src/symmetricblockmatrix.jl:104-110) */
typedef enum { BSM_SCHED_SERIAL = 0, BSM_SCHED_DYNAMIC = 1 } bsm_scheduler;

/* how contributions of different blocks to the same y entries are combined on the GPU */
typedef enum {
    BSM_ACC_AUTO = 0,    /* exclusive direct stores when provably conflict-free, else atomics.  Large
                            conflict-free operators made of deep row groups (most bytes in row groups
                            above 128 KiB, e.g. 128x128 blocks, 16 per block row) are ALSO scheduled as
                            32 KiB work items combined with atomics: 8 % faster, but the last bits then
                            depend on the order of the adds -- BSM_ACC_DIRECT keeps them exclusive */
    BSM_ACC_ATOMIC = 1,  /* hardware fp atomics into y, blocks ordered by colour class */
    BSM_ACC_COLORED = 2, /* one launch per colour class, plain read-modify-write: bitwise
                            reproducible run to run (the reference's own scheme) */
    BSM_ACC_GATHER = 3,  /* no atomics at all: every block contribution is stored once in a
                            workspace owned by the handle and a second launch sums, per y entry,
                            its contributions in a fixed order (and applies alpha, beta): bitwise
                            reproducible, two launches.  The workspace makes products on ONE handle
                            stream-ordered: a call that finds another product of the same handle
                            still in flight on a DIFFERENT stream (or being enqueued by another
                            thread) uses the atomic path for that call.  Single right-hand side
                            only. */
    BSM_ACC_DIRECT = 4   /* like AUTO, but a conflict-free operator always takes the exclusive direct
                            stores (one launch, no atomics, bitwise reproducible) */
} bsm_accumulate;

/* colouring algorithms of bsm_color / bsm_options.coloring (GraphsColoring.jl's names) */
typedef enum { BSM_COLOR_WORKSTREAM_DSATUR = 0, BSM_COLOR_DSATUR = 1 } bsm_coloring;

#define BSM_DEVICE_CURRENT (-1)
#define BSM_DEVICE_NONE (-2) /* analysis only: bookkeeping queries work, bsm_mul fails */

typedef struct {
    int32_t struct_size; /* = sizeof(bsm_options) */
    int32_t device;      /* HIP ordinal, BSM_DEVICE_CURRENT or BSM_DEVICE_NONE */
    int32_t scheduler;   /* bsm_scheduler */
    int32_t accumulate;  /* bsm_accumulate */
    int32_t validate;    /* kept for ABI stability: every index is ALWAYS range-checked at create time
                            (an out-of-range index must never reach a kernel) */
    /* 1: VBCRS / BlockSparseMatrix handles also keep a SECOND, transposed ordering of the blocks
     * (the reference's own TODO, src/vbcrs.jl:124): transpose(A)*x and A'*x then run as a forward
     * product on it -- one launch, no atomics, bitwise reproducible -- at twice the device
     * memory.  0 (default): the transposed products run on the single image with atomics.
     * 2: build the second ordering when it is cheap -- packed values of at most 1/16 of the device's
     * free memory -- else behave like 0 (the default of the Julia binding's ROCmScheduler: Krylov
     * solvers that apply A' every iteration get the one-launch transposed product). */
    int32_t transpose_image;
    /* rows of y this handle is responsible for scaling by beta (1-based, inclusive);
     * 0,0 = all rows.  Used when block rows are partitioned over several GPUs. */
    int64_t own_lo, own_hi;
    /* non-NULL: a bsm_ctx_t (below).  The handle is then spread over the context's devices -- the
     * block rows are partitioned among them, bsm_mul fans out to one stream per device and exchanges
     * the overlapping y segments over xGMI -- exactly where the reference has its `@tasks` fan-out
     * (src/vbcrs.jl:275-276, src/blockmatrix.jl:233-245, src/symmetricblockmatrix.jl:395-432).
     * `device`, own_lo/own_hi and transpose_image are ignored for such a handle. */
    void *ctx;
    /* where the BLOCK arrays passed to *_create live: BSM_MEM_HOST (0, default) or BSM_MEM_DEVICE:
     * device pointers valid on the handle's device (e.g. AMDGPU.jl ROCArrays); the repacking then
     * runs as a kernel on that device and no matrix byte crosses PCIe.  Index lists, sizes and the
     * pointer arrays themselves are always host memory. */
    int64_t blocks_memspace;
    /* the reference's `coloringalgorithm=` keyword (src/blockmatrix.jl:67,86): which algorithm produces
     * the colour classes reported through bsm_get_bookkeeping -- bsm_coloring, default
     * BSM_COLOR_WORKSTREAM_DSATUR like the reference (src/BlockSparseMatrices.jl:10) */
    int64_t coloring;
    int64_t reserved[1];
} bsm_options;

/* The layout the bindings mirror field by field (julia/BlockSparseMatricesROCm.jl: BsmOptions, BsmPartInfo;
 * blocksparsematrices.jl_amd/_lib.py: BsmOptions, BsmPartInfo, BsmStats; tests/test_c_abi_from_c.py asserts the
 * same numbers against the ctypes mirror): a field added or moved here fails the build instead of drifting silently
 * away from a binding that cannot be compiled against this header. */
#if defined(__cplusplus) && __cplusplus >= 201103L
#define BSM_LAYOUT_ASSERT(cond, msg) static_assert(cond, msg)
#elif !defined(__cplusplus) && defined(__STDC_VERSION__) && __STDC_VERSION__ >= 201112L
#define BSM_LAYOUT_ASSERT(cond, msg) _Static_assert(cond, msg)
#else /* C99 / pre-C++11 consumers of the C ABI: the header still compiles, the checks are the library build's */
#define BSM_LAYOUT_ASSERT(cond, msg) struct bsm_layout_assert_unused_
#endif
BSM_LAYOUT_ASSERT(sizeof(bsm_options) == 72, "bsm_options is 72 bytes");
BSM_LAYOUT_ASSERT(offsetof(bsm_options, device) == 4 && offsetof(bsm_options, scheduler) == 8 &&
                      offsetof(bsm_options, accumulate) == 12 && offsetof(bsm_options, validate) == 16 &&
                      offsetof(bsm_options, transpose_image) == 20,
                  "bsm_options: six int32 fields first");
BSM_LAYOUT_ASSERT(offsetof(bsm_options, own_lo) == 24 && offsetof(bsm_options, own_hi) == 32 &&
                      offsetof(bsm_options, ctx) == 40 && offsetof(bsm_options, blocks_memspace) == 48 &&
                      offsetof(bsm_options, coloring) == 56 && offsetof(bsm_options, reserved) == 64,
                  "bsm_options: 8-byte fields from offset 24");

/* ---- several GPUs of one node behind ONE handle -------------------------------------------------
 * The reference runs its block rows / colour classes as tasks of one process (OhMyThreads `@tasks`
 * with the scheduler stored in the matrix).  The MI355X counterpart of that fan-out is a context of
 * devices: a handle created with bsm_options.ctx set keeps one packed image per device (contiguous
 * ranges of block rows, balanced by stored bytes) and bsm_mul / bsm_mul_multi
 *   1. make x available on every device (host memory: one H2D copy per device over its own PCIe
 *      link; device memory: peer copies from the device that holds x),
 *   2. run the local products concurrently, one stream per device,
 *   3. exchange ONLY the y segments a device produced for rows another device owns (symmetric /
 *      index-list operators: the halo; transposed products of a row partition: a reduce-scatter
 *      onto equal column chunks) as direct peer-to-peer copies over the xGMI links + a local add,
 *   4. deliver the owned y ranges to the caller's y (host memory or the device that holds y).
 * VBCRS forward products need no step 3 (block rows own disjoint y ranges, src/vbcrs.jl:275-283).
 * The same device may be listed several times (virtual devices: how the exchange is tested on a
 * one-GPU machine).  One process per GPU with RCCL collectives is the OTHER way to use several GPUs
 * (blocksparsematrices.jl_amd/distributed.py: every rank creates an ordinary single-device handle
 * with own_lo/own_hi from bsm_partition_rows). */
typedef struct bsm_ctx_s *bsm_ctx_t;
int bsm_ctx_create(const int32_t *device_ids, int32_t ndevices, bsm_ctx_t *out);
int bsm_ctx_destroy(bsm_ctx_t ctx); /* after every handle created with it has been destroyed */
/* devices of the context (device_ids may be NULL); returns the count through *ndevices */
int bsm_ctx_devices(bsm_ctx_t ctx, int32_t *ndevices, int32_t *device_ids, int32_t capacity);

/* The row partition both multi-GPU layers use.  Block b has row key rowkey[b] (its smallest row
 * index, 1-based) and weight[b] (stored entries).  The distinct keys, ascending, are cut into
 * nparts contiguous ranges of about equal weight; part_of_block[b] receives the part of block b,
 * own_lo[p] / own_hi[p] (1-based, inclusive; own_hi = own_lo - 1 for an empty part) the rows part p
 * owns: from its first key up to the next part's first key - 1 (part 0 from row 1, the last one to
 * nrows).  Deterministic; blocks with equal keys always land in the same part. */
int bsm_partition_rows(int64_t nrows, int64_t nblocks, const int64_t *rowkey, const int64_t *weight,
                       int32_t nparts, int32_t *part_of_block, int64_t *own_lo, int64_t *own_hi);

/* Per-device view of a multi-device handle (tests, reports): rows owned / touched by part p
 * (1-based inclusive), its device ordinal and the bytes of its packed image. */
typedef struct {
    int32_t device, reserved32;
    int64_t own_lo, own_hi, touched_lo, touched_hi, device_bytes, nblocks;
    /* the part's share of the COLUMN partition (1-based inclusive): what it holds of a vector of length
     * size(A,2) in bsm_mul_parts.  Square operators: the row partition itself (own_lo..own_hi), so that the
     * y parts of one product are the x parts of the next; otherwise equal chunks of the columns. */
    int64_t col_lo, col_hi;
    int64_t reserved[2];
} bsm_part_info_t;
BSM_LAYOUT_ASSERT(sizeof(bsm_part_info_t) == 88 && offsetof(bsm_part_info_t, own_lo) == 8 &&
                      offsetof(bsm_part_info_t, col_lo) == 56 && offsetof(bsm_part_info_t, reserved) == 72,
                  "bsm_part_info_t layout");
int bsm_part_info(bsm_matrix_t A, int32_t part, bsm_part_info_t *out);

/* fills *o with defaults (device = current, serial scheduler, auto accumulate, validate) */
void bsm_options_default(bsm_options *o);

/* VariableBlockCompressedRowStorage(matrices, rowindices, colindices, size; scheduler)
 * -- reference src/vbcrs.jl:78-122.  rowstart/colstart: first row/column of each block
 * (1-based), blocks in any order; the library sorts them exactly as the reference does
 * (stable by (rowstart, colstart)) and builds rowptr.  nblocks >= 1. */
int bsm_vbcrs_create(int dtype, int64_t nrows, int64_t ncols, int64_t nblocks,
                     const void *const *blocks, const int64_t *m, const int64_t *n,
                     const int64_t *ld, const int64_t *rowstart, const int64_t *colstart,
                     const bsm_options *opts, bsm_matrix_t *out);

/* VariableBlockCompressedRowStorage(sbm::SymmetricBlockMatrix; scheduler) -- reference
 * src/vbcrs.jl:189-264.  The reference expands the matrix into [diagonals..., offdiagonals...,
 * transpose(offdiagonals)...] and MATERIALISES the transposes (twice the off-diagonal storage).
 * Here the bookkeeping (perm, rowptr, colindices, rowindices over those ndiag + 2*noff virtual
 * blocks) is identical, but the device image keeps every off-diagonal block once and the product
 * applies it and its transpose from one read.  Like the reference's converter only the FIRST
 * index of every list is used (contiguous ranges are assumed, src/vbcrs.jl:183-184,230-240). */
int bsm_vbcrs_create_from_symmetric(int dtype, int64_t nrows, int64_t ncols, int64_t ndiag,
                                    const void *const *diag, const int64_t *dsize,
                                    const int64_t *dld, const int64_t *diagstart, int64_t noff,
                                    const void *const *off, const int64_t *m, const int64_t *n,
                                    const int64_t *ld, const int64_t *rowstart,
                                    const int64_t *colstart, const bsm_options *opts,
                                    bsm_matrix_t *out);

/* VariableBlockCompressedRowStorage(bsm::BlockSparseMatrix; scheduler) -- reference
 * src/vbcrs.jl:150-160 with the functors of :201-215: block i is placed at
 * (first(rowindices(bsm, i)), first(colindices(bsm, i))), i.e. only the FIRST entry of every index
 * list is used (contiguous ranges are assumed, like the reference's "no sanity checks", :146).
 * Arguments as bsm_blocksparse_create; blocks with an empty list are rejected. */
int bsm_vbcrs_create_from_blocksparse(int dtype, int64_t nrows, int64_t ncols, int64_t nblocks,
                                      const void *const *blocks, const int64_t *m, const int64_t *n,
                                      const int64_t *ld, const int64_t *const *rowidx,
                                      const int64_t *const *colidx, const bsm_options *opts,
                                      bsm_matrix_t *out);

/* BlockSparseMatrix(blocks, rowindices, colindices, size; scheduler, coloringalgorithm)
 * -- reference src/blockmatrix.jl:62-109.  rowidx[b] has m[b] entries, colidx[b] n[b]. */
int bsm_blocksparse_create(int dtype, int64_t nrows, int64_t ncols, int64_t nblocks,
                           const void *const *blocks, const int64_t *m, const int64_t *n,
                           const int64_t *ld, const int64_t *const *rowidx,
                           const int64_t *const *colidx, const bsm_options *opts,
                           bsm_matrix_t *out);

/* SymmetricBlockMatrix(diagonals, diagonalindices, offdiagonals, rowindices, colindices,
 * size; scheduler) -- reference src/symmetricblockmatrix.jl:73-126.  Diagonal block d is
 * dsize[d] x dsize[d] on index list diagidx[d]; only one triangle of the off-diagonal
 * blocks is passed, the product applies each of them and its transpose. */
int bsm_symmetric_create(int dtype, int64_t nrows, int64_t ncols, int64_t ndiag,
                         const void *const *diag, const int64_t *dsize, const int64_t *dld,
                         const int64_t *const *diagidx, int64_t noff, const void *const *off,
                         const int64_t *m, const int64_t *n, const int64_t *ld,
                         const int64_t *const *rowidx, const int64_t *const *colidx,
                         const bsm_options *opts, bsm_matrix_t *out);

/* y = alpha * op(A) * x + beta * y  -- LinearMaps._unsafe_mul!(y, A, x, alpha, beta):
 * reference src/blockmatrix.jl:225-247, src/symmetricblockmatrix.jl:386-435,
 * src/vbcrs.jl:266-288 (forward), :303-354 (adjoint/transpose).
 *   alpha, beta : pointers to one T each (host memory); NULL = 1 resp. 0.
 *   beta_strong_zero != 0 : beta is Julia's Bool `false` (the 3-arg form,
 *     src/abstractblockmatrix.jl:27-34): y is OVERWRITTEN, NaN/Inf in the incoming y do
 *     not propagate.  With beta_strong_zero == 0 a numeric beta = 0 multiplies.
 *   memspace BSM_MEM_DEVICE: x, y are device pointers valid on the handle's device; the
 *     call only enqueues work on `stream` (a hipStream_t, NULL = default stream) and
 *     returns; no allocation or synchronisation happens, so it can be graph-captured (single-device handles
 *     only: a multi-device handle issues on several streams and devices and must not be captured; a
 *     BSM_ACC_GATHER handle takes its atomic path while the stream is capturing -- the workspace of the
 *     gather path admits one product in flight, which a replayed graph could not promise).
 *   memspace BSM_MEM_HOST: x, y are host arrays; the library stages them through device
 *     buffers and returns when y is complete.
 * x has size(op(A),2) entries, y size(op(A),1); they must not alias. */
int bsm_mul(bsm_matrix_t A, int op, const void *x, void *y, const void *alpha,
            const void *beta, int beta_strong_zero, int memspace, void *stream);

/* bsm_mul for a multi-device handle (bsm_options.ctx) with x and y PARTITIONED over its devices -- what an
 * iterative solver on N GPUs holds: block rows own disjoint y ranges (reference src/vbcrs.jl:275-283), so
 * nobody ever needs the whole of x or y in one place.  Part p (bsm_part_info) passes
 *   x_parts[p]: device pointer ON ITS DEVICE to the x entries it holds -- op N: columns col_lo..col_hi,
 *               op T / C: rows own_lo..own_hi (first entry of the range at x_parts[p][0]);
 *   y_parts[p]: device pointer on its device to the y entries it receives -- op N: rows own_lo..own_hi,
 *               op T / C: columns col_lo..col_hi.  Empty ranges may pass NULL.
 * Only what a device's blocks read beyond its own part travels (the x halo), and only the y segments it
 * produced for rows of another device (symmetric / index-list operators; a reduce-scatter for products across
 * the partition): both as ONE fused kernel per device that reads its peers' memory over xGMI -- no copy of the
 * full x to anybody, no staging.  streams[p] (may be NULL = the device's default stream; the array itself may be
 * NULL): the stream of part p's device on which x_parts[p] / y_parts[p] are produced and consumed; the call
 * orders its work behind them and them behind its result, and returns without synchronising.
 * Needs peer access between all devices of the context (BSM_ERR_UNSUPPORTED otherwise).  alpha, beta,
 * beta_strong_zero as in bsm_mul. */
int bsm_mul_parts(bsm_matrix_t A, int op, const void *const *x_parts, void *const *y_parts, const void *alpha,
                  const void *beta, int beta_strong_zero, void *const *streams);

/* A HIP stream for the products of a rank that exchanges vector segments with its neighbours WHILE it multiplies (one
 * process per GPU, RCCL): its CU mask leaves `reserved_cus` compute units -- rounded up to a multiple of 8, one per XCD
 * -- to the collective layer's kernels.  Beside a product launch that fills every CU those kernels otherwise wait for
 * the launch to drain (measured: DESIGN.md section 5b).  0 = an ordinary non-blocking stream.  Pass the stream to
 * bsm_mul / bsm_mul_multi like any other (`stream` argument); the reference has no counterpart (shared-memory tasks,
 * src/symmetricblockmatrix.jl:395-432). */
int bsm_stream_create_reserved(int device, int reserved_cus, void **stream);
int bsm_stream_destroy(void *stream);

/* y[offset[s] + i] += src[s][i], i < len[s], for nseg DISJOINT segments of a device vector y, in ONE launch on
 * `stream` (dtype BSM_F32 .. BSM_C128 as in the *_create calls -- a mixed storage code is BSM_ERR_INVALID here;
 * offsets 0-based, in elements).  The delivery step of a row-partitioned
 * product in a process-per-GPU layer above this ABI (blocksparsematrices.jl_amd/distributed.py: the own rows of the
 * boundary blocks' sums + every partial-y segment received from a neighbour -- the y segments other tasks of the
 * reference's fan-out would have added in shared memory, src/symmetricblockmatrix.jl:407-418): one launch behind
 * the join of the exchange instead of one per segment.  Overlapping segments are refused (BSM_ERR_INVALID). */
int bsm_vec_add_segments(int dtype, void *y, int32_t nseg, const int64_t *offset, const void *const *src,
                         const int64_t *len, void *stream);

/* Page-locks a HOST vector the caller keeps using as x or y of BSM_MEM_HOST products (a Julia
 * Vector{T} that lives through a solver loop): bsm_mul then moves it by DMA straight from / to the
 * caller's memory instead of copying it through the library's pinned mirrors (C2-sized product:
 * measured in DESIGN.md section 6).  The memory must stay allocated until bsm_host_unregister; the
 * Julia binding registers in the constructor of its vector wrapper and unregisters in the finalizer.
 * (hipHostRegister / hipHostUnregister, exported so that the host language needs no HIP binding.) */
int bsm_host_register(void *ptr, int64_t bytes);
int bsm_host_unregister(void *ptr);

/* Y = alpha * op(A) * X + beta * Y for nrhs right-hand sides -- `A * X` / `mul!(Y, A, X, a, b)`
 * with matrices.  LinearMaps loops the columns of X through _unsafe_mul! (nrhs full sweeps of A);
 * here A is streamed ONCE per batch of up to 8 columns (16 for Float32 / Float64 matrices from 9 columns on; a
 * remainder is one padded pass; nothing outside the nrhs columns of X and Y is read or written).  The 8-column
 * passes of the complex types and the 16-column passes of the real ones run on the matrix pipe (8 complex
 * columns = 16 real ones = N of v_mfma_{f64,f32}_16x16x4).  X is size(op(A),2) x nrhs
 * and Y is size(op(A),1) x nrhs, both column-major with leading dimensions ldx / ldy (elements).
 * Every other argument as in bsm_mul; each column gives what nrhs = 1 semantics prescribe (same
 * alpha, beta, strong zero).  nrhs = 1 is bsm_mul: the same kernels and, on a BSM_ACC_GATHER handle, the
 * same bitwise reproducible gather path.
 * Mixed-precision handles (BSM_F64_F32, BSM_C128_C64): from 3 columns on (2 on handles with symmetric pieces; BSM_IL_MIXED_MIN_COLS = 2 .. 8 overrides) the
 * single-precision image is streamed ONCE per batch of 16 double / 8 complex double columns, on every image class
 * (exclusive forward ones included): the stored values are widened in registers and meet X on the f64 matrix pipe, every
 * sum is double.  A last batch of at most 8 / 4 columns is one pass over 8 components; columns below the threshold
 * are one-column products.  These passes use the handle's interleaved work arrays (2 x 128 bytes per vector entry,
 * allocated at the first multi-column product that takes them; atomics: the last bits depend on the order of the
 * adds).  A product that does not get them -- another product in flight on them, graph capture, no memory --, a
 * coloured image (BSM_ACC_COLORED: bitwise reproducible read-modify-write), vectors of 2^30 entries and more, or
 * BSM_MULTI_IL=0 in the environment run nrhs one-column products, one after another on `stream`: the matrix is then
 * streamed nrhs times (bsm_value_passes tells which happened). */
int bsm_mul_multi(bsm_matrix_t A, int op, int64_t nrhs, const void *X, int64_t ldx, void *Y,
                  int64_t ldy, const void *alpha, const void *beta, int beta_strong_zero, int memspace,
                  void *stream);

/* y = alpha * op(A) * x + beta * y for a REAL handle (BSM_F32 / BSM_F64) and COMPLEX vectors of the same precision
 * (complex float / complex double): x, y, alpha, beta are complex; op C = op T on a real matrix.  A Float64 operator
 * applied to ComplexF64 vectors (the Gram matrix, near fields of static kernels, real preconditioners in a BEM solve:
 * the reference's generic loops, src/abstractblockmatrix.jl:27-34) in ONE pass over the matrix: each stored real
 * value meets the complex x entry in two FMAs, nothing is widened to complex.  Every semantic of bsm_mul carries over
 * (strong zero, own rows, memspaces, graph capture, accumulate modes, transpose_image, the bitwise reproducible
 * gather path of BSM_ACC_GATHER handles).  Memory: host vectors are staged through buffers of twice the real
 * handle's vector bytes; a BSM_ACC_GATHER image gets a second, complex workspace of (workspace slots + 8) x 2 x
 * sizeof(real) bytes, allocated at the first complex product that takes the gather path (never under graph capture:
 * until it exists, a captured product takes the atomic path, as a busy workspace does).
 * Refused before anything is enqueued: a complex handle (BSM_ERR_INVALID: bsm_mul takes its vectors), a mixed-storage
 * handle (BSM_F64_F32, BSM_C128_C64) or a multi-device handle (bsm_options.ctx): BSM_ERR_UNSUPPORTED; bad op / memspace
 * or null pointers: BSM_ERR_INVALID; an analysis-only handle: BSM_ERR_DEVICE. */
int bsm_mul_cvec(bsm_matrix_t A, int op, const void *x, void *y, const void *alpha, const void *beta,
                 int beta_strong_zero, int memspace, void *stream);
/* bsm_mul_multi with complex vectors under a real handle (refusals and memory as bsm_mul_cvec).  Batches of 8 complex
 * columns are ONE pass of the real multi-RHS kernels over their 16 real components (Re / Im interleaved; a last batch
 * of at most 4 columns over 8): alpha is applied as X is interleaved, beta as Y is written back.  These passes use the
 * handle's interleaved work arrays (128 bytes per vector entry each, allocated at the first product that takes them);
 * when a product does not get them (another product in flight on them, graph capture) or the image is coloured
 * (BSM_ACC_COLORED: bitwise reproducible read-modify-write), it runs as nrhs one-column products.  nrhs = 1 is
 * bsm_mul_cvec. */
int bsm_mul_multi_cvec(bsm_matrix_t A, int op, int64_t nrhs, const void *X, int64_t ldx, void *Y, int64_t ldy,
                       const void *alpha, const void *beta, int beta_strong_zero, int memspace, void *stream);

/* Replaces the VALUES of blocks of an existing handle -- what a Julia caller gets by editing block(A, i) in place
 * (the reference keeps the caller's matrices by reference, src/vbcrs.jl:98,114, src/blockmatrix.jl:26-34).
 * Structure, index lists, shapes, options and the layout of the device image stay as created: no analysis runs.
 *   ids: nupd 1-based positions in the block order of the *_create call that made the handle -- `blocks` of
 *     bsm_vbcrs_create / _blocksparse_create / _vbcrs_create_from_blocksparse (the caller's order, NOT the
 *     VBCRS-sorted one), `diag` followed by `off` for bsm_symmetric_create / _vbcrs_create_from_symmetric;
 *     NULL = all blocks in that order (nupd must then equal the count).
 *   blocks[k] / ld[k]: block ids[k], same m x n as at creation, column-major, ld[k] >= m (ld may differ from the
 *     one given at creation).  memspace: where the blocks live.
 *   BSM_MEM_DEVICE: enqueued on `stream`, returns without synchronising; the blocks must stay valid until the
 *     stream reaches the update.  The first update of a handle uploads its refill plan (allocates, synchronises);
 *     after it an update allocates nothing.  The kernels read a table of sources (device address + ld per block):
 *     an update that names the same blocks, arrays and ids as the previous one reuses the table and makes `stream`
 *     wait for that update; one that names others first waits on the host for the previous update's kernels, then
 *     copies its table on `stream`.
 *     Graph capture (single-device handles, after one uncaptured update): a captured update carries its OWN copy of
 *     the table -- a captured copy from a pinned snapshot taken at capture time into a device table only captured
 *     updates use -- so a replay reads the addresses its capture saw (they must still be valid, and the data there is
 *     what the replay refills from), whatever uncaptured updates ran in between.  A handle holds one such snapshot:
 *     every captured update of it must name the same blocks, arrays and ids (BSM_ERR_UNSUPPORTED otherwise), and
 *     host-block updates cannot be captured.
 *   BSM_MEM_HOST: returns when the image holds the new values (the caller may reuse its arrays).  The blocks go
 *     through pinned 64 MB staging windows, double-buffered, once over PCIe; the same kernel places them.
 * Every image the handle owns is refilled: the forward one, the transposed one (bsm_options.transpose_image) and
 * every part of a multi-device handle on its own device.  A multi-device handle's update waits for `stream` and for
 * every earlier product of the handle, and returns when all parts hold the new values.  Analysis-only handles
 * (BSM_DEVICE_NONE) take BSM_MEM_HOST updates (their host image, bsm_get_image, is rewritten).
 * Products enqueued on `stream` after the call see the new values.  Products on other streams, and products
 * running in other threads on the same handle, are the caller's to order (as for any write the caller makes to x):
 * an update is stream-ordered like a product and takes no lock on the product path.
 * Every argument is checked before the first byte is written: a failing call leaves the handle unchanged
 * (BSM_ERR_INVALID: null handle or pointer, id out of range, duplicate id, nupd != count with ids == NULL, ld < m,
 * bad memspace, BSM_MEM_DEVICE on an analysis-only handle).  Mixed-precision handles (BSM_F64_F32, BSM_C128_C64) are
 * refused with BSM_ERR_UNSUPPORTED.
 * Memory: a handle keeps its block list from creation on (index lists copied).  The first update derives the refill
 * plan from it -- the value-blind placement of the create, re-run and checked against the image -- and keeps it on the
 * host and on the device until bsm_destroy: 32 B per <= 64-row chunk of every image, 16 B per segment of <= 16 KB,
 * 8 B per wave item, 16 B per block id, 4 B per stored column of scattered index-list groups; on the device also the
 * two 16 B per block source tables (uncaptured, captured) and their pinned host mirrors.  bsm_stats_t does not count it. */
int bsm_update_blocks(bsm_matrix_t A, int64_t nupd, const int64_t *ids, const void *const *blocks,
                      const int64_t *ld, int memspace, void *stream);

/* *count = how many times products of this handle have streamed a value image since it was created.  Counted when a
 * product is enqueued: a one-column product is 1; a multi-column batch that streams the matrix once (interleaved pass
 * or multi-RHS kernels) is 1 whatever its width and however many colour launches it takes; columns that run one at a
 * time are 1 each.  A product captured into a graph counts when it is captured, not when the graph is replayed.  So a
 * bsm_mul_multi of nrhs columns that adds nrhs here ran column by column (e.g. it did not get the handle's work
 * arrays).  Both images of a transpose_image handle count.  Single-device handles (an analysis-only one answers 0);
 * a multi-device handle: BSM_ERR_UNSUPPORTED; null handle or pointer: BSM_ERR_INVALID. */
int bsm_value_passes(bsm_matrix_t A, int64_t *count);

/* Bookkeeping queries (bit-exact contract; every value 1-based int64 like the reference).
 * Call with out == NULL to obtain the required length in *len. */
typedef enum {
    BSM_BK_VBCRS_PERM = 0,        /* sortperm of src/vbcrs.jl:84 */
    BSM_BK_VBCRS_ROWPTR = 1,      /* src/vbcrs.jl:97-117, length nblockrows+1 */
    BSM_BK_VBCRS_COLINDICES = 2,  /* per block, sorted order */
    BSM_BK_VBCRS_ROWINDICES = 3,  /* per block ROW */
    /* colour sets, flattened as [ncolors, len_1, ids_1..., len_2, ids_2..., ...] */
    BSM_BK_COLORS = 4,            /* BlockSparseMatrix.colors / Symmetric offdiagonalcolors */
    BSM_BK_TRANSPOSECOLORS = 5,   /* transposecolors / transposeoffdiagonalcolors */
    BSM_BK_DIAGONALCOLORS = 6     /* Symmetric diagonalcolors */
} bsm_bookkeeping;
int bsm_get_bookkeeping(bsm_matrix_t A, int which, int64_t *out, int64_t *len);

/* rowcolvals(A) -- reference src/sparse.jl:17-123, the COO triples behind `sparse(A)`
 * (src/sparse.jl:125-129): written by a kernel straight from the packed DEVICE image -- every stored
 * entry once, the off-diagonal blocks of a SymmetricBlockMatrix a second time transposed -- so that a
 * CSR / CSC matrix can be assembled on the GPU without the blocks ever returning to the host.
 * rows / cols: 1-based int64, vals: the handle's element type T (mixed-precision handles: the stored values widened
 * to T, i.e. exactly blocks.astype(S).astype(T)), all with room for *count entries
 * (call with NULL arrays to obtain the count = nnz(A) as the reference defines it).  The order of the
 * triples is fixed but unspecified (`sparse` sums duplicates, like mul!'s +=).  memspace: where the
 * three arrays live (BSM_MEM_DEVICE: on the handle's device).  Synchronous. */
int bsm_rowcolvals(bsm_matrix_t A, int64_t *rows, int64_t *cols, void *vals, int64_t *count, int memspace,
                   void *stream);

/* A[I, J]: entries of the operator read out of its packed image --
 *   out[s][a + b * ldo[s]] = op(A)[I[s][a], J[s][b]]   for a < ni[s], b < nj[s], s < nsets
 * in ONE pass over the image, whatever nsets is: what `A[i, j]`, `A[:, j]`, `A[I, J]` of the reference's LinearMap
 * surface and the self-interaction blocks A[I_k, I_k] of a block-Jacobi / near-field preconditioner ask for (by unit
 * vectors: one pass per 8 or 16 requested columns).  The pass reads only the strips that hold a requested column of a
 * requested row's set.
 *   Index lists: I, J, ni, nj, ldo and the `out` pointer array are host memory.  Indices are 1-based int64, in any
 *     order; I[s] indexes rows of op(A), J[s] its columns.  The row sets must be pairwise disjoint and free of repeats,
 *     and so must the column sets (a row then belongs to at most one set: that is what lets one pass serve every set; a
 *     binding expands repeated indices itself).  ni[s] == 0 or nj[s] == 0 is legal and out[s] may then be NULL;
 *     ldo[s] >= max(ni[s], 1).
 *   Values: the sum of every stored entry at that position -- overlapping blocks of a BlockSparseMatrix add, as in
 *     sparse(A) (reference src/sparse.jl:127-129) and in mul!'s +=; an off-diagonal block of a symmetric operator counts
 *     at (r, c) and, transposed and not conjugated, at (c, r): the enumeration of bsm_rowcolvals.  op T swaps the roles
 *     of the index lists, op C also conjugates.  The element type is the handle's vector type T; mixed-precision handles
 *     deliver the stored value widened (exactly blocks.astype(S).astype(T)).  Where several stored entries meet, the
 *     last bits depend on the order of the adds.
 *   Output: the ni x nj window of every out[s] is OVERWRITTEN (zeroed, then summed: NaN in the incoming buffer does not
 *     survive); no byte outside the windows is written, the ldo padding included.
 *   memspace: where the out[s] arrays live.  BSM_MEM_DEVICE: on the handle's device, the work goes on `stream`.  The
 *     call is SYNCHRONOUS either way, like bsm_rowcolvals: it uploads its maps (4 bytes per row and per column, twice)
 *     and is a setup-time call, not to be graph-captured.
 *   Analysis-only handles (BSM_DEVICE_NONE) answer BSM_MEM_HOST calls from their host image.
 *   Multi-device handles (bsm_options.ctx): every stored entry lives in exactly one part, so the parts run one after
 *     another, each into a zeroed staging buffer on its own device; the buffers return to the host, are added there and
 *     delivered (to host or device windows).  Cost linear in the OUTPUT size per part, on top of the pass.
 *   What is read: the forward image only.  A transpose_image handle, any accumulate mode and an own_lo / own_hi slice
 *     give the entries of the blocks the handle holds.
 * Every argument is checked before the first byte is written.  BSM_ERR_INVALID: null handle or pointer, bad op or
 * memspace, an index outside 1..size(op(A), dim), an index in two sets or twice in one, ldo too small, nsets < 0,
 * BSM_MEM_DEVICE on an analysis-only handle. */
int bsm_submatrices(bsm_matrix_t A, int op, int64_t nsets, const int64_t *const *I, const int64_t *ni,
                    const int64_t *const *J, const int64_t *nj, void *const *out, const int64_t *ldo, int memspace,
                    void *stream);
/* diag(A): d[k] = A[k + 1, k + 1], k < min(nrows, ncols) -- the same pass without index lists (values, memspace,
 * synchronisation, handle kinds and refusals as bsm_submatrices; d is overwritten).  Only the strips that cross the
 * diagonal are read. */
int bsm_diag(bsm_matrix_t A, void *d, int memspace, void *stream);

/* Batched inverse of dense blocks of different sizes, in place:
 *   blocks[b][i + j * ld[b]], i, j < n[b]   becomes   inv(block b)      for b < nblocks
 * -- the step between bsm_submatrices (the self-interaction blocks A[I_s, I_s] of an operator) and the block-Jacobi /
 * near-field preconditioner M = sum_s E_s inv(A[I_s, I_s]) E_s^T, which is then an ordinary BlockSparseMatrix handle
 * built from the inverted blocks (blocks_memspace = BSM_MEM_DEVICE) and applied by bsm_mul.  (No counterpart in the
 * reference: its LinearMap surface offers A[I, J] and leaves factorisations to the caller.)
 *   Arguments: dtype BSM_F32 .. BSM_C128 (the mixed storage codes are BSM_ERR_INVALID, as in bsm_vec_add_segments).
 *     blocks, n, ld and info are HOST arrays; block b is column-major with leading dimension ld[b] >= max(n[b], 1).
 *     n[b] == 0 is legal and blocks[b] may then be NULL; n[b] > 1024 is BSM_ERR_UNSUPPORTED (one workgroup eliminates
 *     one block: this is a setup-time call for preconditioner blocks).  The blocks must not overlap in memory (the
 *     caller's contract, not checked).
 *   Algorithm (fixed, so that host and device choose the same pivots): in-place Gauss-Jordan elimination with partial
 *     row pivoting.  At step k the pivot is the entry of column k in rows k .. n-1 with the largest magnitude -- |v| for
 *     real, |re| + |im| for complex types (LAPACK's cabs1), a NaN counted as +inf --, ties to the smallest row; the rows
 *     are swapped, the pivot row is scaled by the reciprocal of the pivot, every other row is reduced by a rank-1
 *     update with its multiplier A[i, k] / pivot (a true division: a row that duplicates the pivot row cancels exactly
 *     and the block is reported singular); after the last step the column swaps are undone in reverse order.  As for
 *     any explicit inverse the forward error grows with the condition number of the block: ill-conditioned blocks want
 *     a factorisation.
 *   info (may be NULL): info[b] = 0 -- block b holds its inverse; info[b] = k (1-based) -- the pivot of step k was
 *     exactly zero or not finite, the contents of that block are then unspecified, the other blocks are unaffected.  The
 *     call still returns BSM_OK (LAPACK style).
 *   memspace: where the blocks live.
 *     BSM_MEM_DEVICE: pointers valid on the current device, or on the device of `stream` when one is given; the work
 *       is enqueued on `stream`.  One 256-thread workgroup per block, the largest blocks first.  A block with
 *       n * n * sizeof(T) <= BSM_INVERT_LDS_BYTES is eliminated in LDS, a larger one in place in device memory.  The
 *       call is SYNCHRONOUS like bsm_submatrices -- it uploads a table of (address, n, ld) per block and reads info
 *       back -- and is not to be graph-captured.  Results are bit-identical from run to run.
 *     BSM_MEM_HOST: the same elimination, serially on the host in plain C++; needs no device (works wherever
 *       analysis-only handles do); `stream` is ignored.
 *   Nothing outside the n x n windows is written, the ld padding included.  Every argument is checked before the first
 *   byte is written.  BSM_ERR_INVALID: null blocks / n / ld with nblocks > 0, nblocks < 0, a negative n, ld too small,
 *   bad dtype or memspace, a NULL block with n > 0. */
#define BSM_INVERT_LDS_BYTES 131072 /* of the 160 KiB of LDS per CU; staging arrays take less than 8 KiB more */
#define BSM_INVERT_MAX_N 1024
int bsm_invert_blocks(int dtype, int64_t nblocks, void *const *blocks, const int64_t *n, const int64_t *ld,
                      int64_t *info, int memspace, void *stream);

/* Batched eigendecomposition of dense HERMITIAN blocks of different sizes, in place:
 *   (B_b + B_b^H) / 2 = V_b diag(w_b) V_b^H,   B_b = blocks[b][i + j * ld[b]], i, j < n[b]       for b < nblocks
 * -- what a spectral block-Jacobi preconditioner needs where the explicit inverse of bsm_invert_blocks does not serve: an
 * indefinite A[I_s, I_s] (M_ss = V diag(1 / |w|) V^H is Hermitian positive definite, which MINRES, LOBPCG and CG ask of M) or
 * a singular one (the pseudo-inverse); bsm_spectral_blocks puts such an M_ss together.  (No counterpart in the reference.)
 *   Arguments: those of bsm_invert_blocks -- dtype BSM_F32 .. BSM_C128 (the mixed storage codes are BSM_ERR_INVALID); blocks,
 *     n, ld, w, info and sweeps are HOST arrays; block b is column-major with ld[b] >= max(n[b], 1); n[b] == 0 is legal with a
 *     NULL block; the blocks must not overlap.  w[b] points to n[b] entries of the REAL type of dtype (float for BSM_F32 /
 *     BSM_C64, double for BSM_F64 / BSM_C128) in the memory space of the blocks.  n[b] > BSM_EIGH_MAX_N is BSM_ERR_UNSUPPORTED
 *     (one workgroup decomposes one block).  info and sweeps may be NULL.
 *   What is decomposed: H = (B + B^H) / 2 -- both triangles are read and symmetrised at load, the imaginary part of the
 *     diagonal is dropped, so the rounding-level asymmetry of an extracted A[I_s, I_s] is harmless.
 *   Result: w[b] holds the eigenvalues ascending, ties in the order of the diagonal positions they came from (a stable sort).
 *     vectors != 0: block b holds the orthonormal eigenvectors as its columns, in that order.  vectors == 0: the contents of
 *     the block are unspecified.
 *   info[b] = 0 -- done;  1 -- block b holds an entry that is not finite: the block is untouched, w[b] is filled with NaN;
 *     2 -- the sweep cap was hit: w, V hold the pairs as they stand, sorted.  The other blocks are unaffected and the call
 *     returns BSM_OK in all three cases (LAPACK style).  sweeps[b]: the sweeps that rotated (BSM_EIGH_MAX_SWEEPS with info 2).
 *   Algorithm (fixed, so that host and device run the same sequence of rotations): two-sided Jacobi in the block's own type
 *     in a round-robin (tournament) order.  m = n rounded up to even; a sweep has m - 1 steps; step t = 0 .. m-2 holds the
 *     m / 2 disjoint pairs (t, m-1) and ((t + k) mod (m-1), (t - k) mod (m-1)), k = 1 .. m/2 - 1, in each p = min, q = max; a
 *     pair with q >= n (the padding index of an odd n) idles.  The rotation of a pair is that of the project's host-side
 *     Jacobi solvers: with a_pq = g omega, g = |a_pq|, nothing is done if g == 0; the pair is skipped and a_pq = a_qp = 0 is
 *     set when |a_pp| + g == |a_pp| and |a_qq| + g == |a_qq| in the working type; otherwise tau = (a_qq - a_pp) / (2 g),
 *     t = sign(tau) / (|tau| + sqrt(1 + tau^2)), c = 1 / sqrt(1 + t^2), s = t c; columns: x = col_p, y = conj(omega) col_q,
 *     col_p <- c x - s y, col_q <- s x + c y, for A and for V; rows: the same with omega; then a_pp <- a_pp - t g, a_qq <-
 *     a_qq + t g, a_pq = a_qp = 0.  All pairs of a step derive their rotations first and rotate together: the column phase of
 *     every pair, then the row phase of every pair -- J^H (A J) with J the product of the step's commuting rotations.  The
 *     method ends with the first sweep that rotates nothing.  The order of w is a rank sort: rank_i = #{j : w_j < w_i or
 *     (w_j == w_i and j < i)}.
 *   memspace: where the blocks and the w[b] live.
 *     BSM_MEM_DEVICE: pointers valid on the current device, or on the device of `stream` when one is given; the work is
 *       enqueued on `stream`.  One 256-thread workgroup per block, the largest blocks first.  A block with 2 * n * n *
 *       sizeof(T) <= BSM_EIGH_LDS_BYTES (n <= 128 / 90 / 90 / 64 for float / double / complex float / complex double) keeps A
 *       and V in LDS for the whole solve; a larger one is rotated in place in device memory, its V in a scratch array the call
 *       allocates and frees.  The call is SYNCHRONOUS like bsm_invert_blocks -- it uploads a table of (block, n, ld, w) and
 *       reads info and sweeps back -- and is not to be graph-captured.  Results are bit-identical from run to run; host and
 *       device results agree to rounding, not to the bit.
 *     BSM_MEM_HOST: the same rotations, serially on the host in plain C++, in the block's own type; needs no device (works
 *       wherever analysis-only handles do); `stream` is ignored.
 *   Nothing outside the n x n windows and the n entries of w[b] is written.  Every argument is checked before the first byte
 *   is written.  BSM_ERR_INVALID: what bsm_invert_blocks refuses, null w, a NULL w[b] with n[b] > 0. */
#define BSM_EIGH_LDS_BYTES 131072 /* A and V of a resident block; the staging arrays take less than 8 KiB more */
#define BSM_EIGH_MAX_N 512
#define BSM_EIGH_MAX_SWEEPS 60
int bsm_eigh_blocks(int dtype, int64_t nblocks, void *const *blocks, const int64_t *n, const int64_t *ld,
                    void *const *w, int32_t vectors, int64_t *info, int32_t *sweeps, int memspace, void *stream);

/* out_b = V_b diag(f(w_b)) V_b^H from the eigenpairs of bsm_eigh_blocks (any V and real w are taken: V need not be orthogonal):
 *   out[i, j] = sum_k f_k V[i, k] conj(V[j, k]),   the sum over k ascending with fused multiply-adds (t = f_k V[i, k] rounded,
 * then acc += t conj(V[j, k])), computed for i >= j and mirrored: out is Hermitian TO THE BIT with a real diagonal, and the
 * same bytes from run to run.  With wmax = the largest |w_k| over the finite w_k of the block and bound = rcond * wmax (0 when
 * rcond == 0), f_k is
 *   BSM_SPEC_VALUES  w_k -- the caller has applied its function already;
 *   BSM_SPEC_INV     1 / w_k;
 *   BSM_SPEC_ABSINV  1 / max(|w_k|, bound) -- always positive: with rcond > 0 the result is Hermitian positive definite;
 *   BSM_SPEC_PINV    1 / w_k where |w_k| > bound, else 0 -- the Hermitian pseudo-inverse.
 * info[b] (may be NULL) = 0, or the 1-based index of the first eigenvalue at which f is undefined -- BSM_SPEC_INV: w_k zero or
 * not finite; BSM_SPEC_ABSINV: w_k not finite, or max(|w_k|, bound) zero; BSM_SPEC_PINV: w_k not finite --: out[b] is then not
 * written, the other blocks are unaffected and the call still returns BSM_OK.
 *   V, n, ldv, w, out, ldo, info are HOST arrays; V[b] and out[b] are column-major with ldv[b], ldo[b] >= max(n[b], 1), w[b]
 * holds n[b] reals, all in `memspace`.  out must overlap neither V nor w (the caller's contract, as in bsm_invert_blocks).
 * Device: one workgroup per block, largest first, V staged in LDS when n * n * sizeof(T) <= BSM_EIGH_LDS_BYTES and read from
 * device memory otherwise; orders, the synchronous contract and the plain C++ host route are those of bsm_eigh_blocks.
 * Nothing outside the n x n windows of out is written.  BSM_ERR_INVALID: a negative or NaN rcond, an unknown func, null
 * arrays, and what bsm_eigh_blocks refuses; n[b] > BSM_EIGH_MAX_N: BSM_ERR_UNSUPPORTED. */
enum { BSM_SPEC_VALUES = 0, BSM_SPEC_INV = 1, BSM_SPEC_ABSINV = 2, BSM_SPEC_PINV = 3 };
int bsm_spectral_blocks(int dtype, int64_t nblocks, const void *const *V, const int64_t *n, const int64_t *ldv,
                        const void *const *w, int32_t func, double rcond, void *const *out, const int64_t *ldo,
                        int64_t *info, int memspace, void *stream);

/* ---- Krylov building block and solver: restarted GMRES wholly on the device ----------------------------------------
 * What consumes a preconditioner handle M (block_jacobi: bsm_submatrices + bsm_invert_blocks + a BlockSparseMatrix
 * handle): A x = b for the non-symmetric and complex operators the reference exists for, without a Krylov loop in the
 * host language that issues a dozen tiny kernels and several synchronisations per iteration.  (No counterpart in the
 * reference: its operators are LinearMaps, handed to a Julia solver package.)
 *
 * bsm_krylov_orth -- ONE classical Gram-Schmidt pass of w against the first k columns of a basis V (n x k, column-major,
 * leading dimension ldv >= max(n, 1), element type T = dtype):
 *     h = V[:, 0:k]^H w;   w -= V[:, 0:k] h;   hsum[0:k] += h;   nrm[0] = || w ||_2 of the result (one REAL of T's precision).
 * A solver runs it twice per iteration (CGS2) on the same hsum.  All pointers are DEVICE pointers (valid on the current
 * device, or on the device of `stream` when one is given: the launches are issued with that device current); the call enqueues three launches on `stream` and returns: no
 * allocation, no synchronisation, no scalar crosses to the host, so it can be graph-captured.  The dot phase reads V
 * and w once for all k columns; every sum -- per wave, per workgroup, the per-workgroup partials in `work` -- has a
 * fixed order and there are no floating-point atomics: results are bit-identical from run to run.  16-byte loads are
 * used when V, w and ldv * sizeof(T) are congruent modulo 16; any other alignment of whole elements works element by
 * element.  `work`: bsm_krylov_orth_work(dtype, n, k) bytes, 16-byte aligned, contents unspecified before and after.
 * k = 0 gives only the norm; n = 0 is legal (nrm = 0, hsum unchanged).  Nothing of V, and nothing outside the n entries
 * of w, hsum[0:k] and nrm[0], is written.
 * BSM_ERR_INVALID: a mixed storage code or a bad dtype (as in bsm_vec_add_segments), n < 0, k < 0 or k >
 * BSM_GMRES_MAX_RESTART, ldv < max(n, 1) with k > 0, a null pointer that is needed (hsum with k > 0; V with k > 0 and n > 0;
 * w with n > 0; nrm; work), a work array that is not 16-byte aligned, a negative result of the size query for bad arguments. */
#define BSM_GMRES_MAX_RESTART 128
int64_t bsm_krylov_orth_work(int dtype, int64_t n, int64_t k);
int bsm_krylov_orth(int dtype, int64_t n, int64_t k, const void *V, int64_t ldv, void *w, void *hsum, void *nrm,
                    void *work, void *stream);

/* bsm_gmres_*: right-preconditioned restarted GMRES(restart) for op(A) x = b with M ~ inv(op(A)) applied as opM(M).
 *   r = b - op(A) x,  beta = ||r||,  v_0 = r / beta;  iteration j: z = M v_j (skipped without M), w = op(A) z, two
 *   classical Gram-Schmidt passes against v_0 .. v_j (the pass of bsm_krylov_orth), one one-wave kernel that applies the j
 *   stored Givens rotations to the new Hessenberg column, forms rotation j and the residual estimate |g[j + 1]|, then
 *   v_{j+1} = w / ||w||.  At the end of a cycle, or at convergence after k iterations: back substitution R y = g[0:k] (one
 *   wave), u = V[:, 0:k] y, x += M u, and the next cycle starts from the TRUE residual b - op(A) x.  Right preconditioning:
 *   the estimate is the residual norm of the unpreconditioned system.
 *   What runs is bsm_gmres_multi_* (below) with ONE column: the same solver object created with nrhs_max = 1, the same
 *   kernels (csrc/bsm_gmres_multi.hip), every decision taken on the device, the host reading one record per start and
 *   iteration from a ring of pinned slots, one step behind its enqueues.  These entry points only translate the structs:
 *   b and x are a matrix of one column, info is filled from bsm_cg_info and the one bsm_cg_column.
 * create: bsm_gmres_multi_create with nrhs_max = 1 -- one device allocation on A's device: restart + 3 vectors (the basis
 *   v_0 .. v_restart, w, the solver's own x), restart + 4 with M (z), the small arrays of a cycle and the partial sums.
 *   vdtype (BSM_F32 .. BSM_C128) is the type of b and x.  Each of A, M must have that vector type -- a mixed-storage
 *   handle counts with its double vectors -- or be a real, unmixed handle of the same precision under a complex vdtype,
 *   which is then driven through bsm_mul_cvec.  The handles must outlive the solver.  Refusals: null A or out, bad op / vdtype, a type pair not named above, op(A) not square, M of another
 *   order or on another device, restart < 1 or > BSM_GMRES_MAX_RESTART: BSM_ERR_INVALID; a multi-device handle, or one
 *   that owns a row range only (bsm_options.own_lo / own_hi: its products define the owned rows of y alone):
 *   BSM_ERR_UNSUPPORTED; an analysis-only handle: BSM_ERR_DEVICE.
 * solve: b, x of n elements, any element alignment: they are touched only by the start (b is read, x too with use_x0 != 0)
 *   and by the final copy-out of the n entries of x.  Converged when the estimate is <= max(rtol * ||b||_2, atol).  maxiter
 *   bounds the iterations (products with A inside cycles); values above INT32_MAX count as INT32_MAX (the counters on the
 *   device are 32-bit).  use_x0 == 0: x is overwritten (NaN in the incoming x does not survive); else x is the initial
 *   guess.  b = 0 gives x = 0, 0 iterations, status 0.
 *   The answer uses exactly the k iterations up to the first one whose estimate met the tolerance; what the host enqueued
 *   beyond it finds the column frozen and writes nothing: iterations, history and x do not depend on timing.
 *   history (may be NULL): history[i] = the absolute estimate after iteration i + 1, at most history_capacity entries.
 *   Two exits report status 0: an iteration whose ESTIMATE met the tolerance (the last history entry is then <= the
 *   tolerance and info.residual equals it), and the start of a cycle whose TRUE residual b - op(A) x already met it (the
 *   last cycle ended with an estimate just above the tolerance, or x0 solves the system: info.residual is that true
 *   residual norm, no history entry is written for it, and the last history entry, if any, still lies above the tolerance).
 *   memspace: BSM_MEM_DEVICE -- b, x on A's device; BSM_MEM_HOST -- staged through device buffers the solver allocates
 *   at its first host solve.  The call is SYNCHRONOUS: it returns when x is complete.  It runs wholly on `stream` and
 *   must not be graph-captured.  One solve at a time per solver object.
 *   BSM_ERR_INVALID: null S / b / x / p / info with n > 0, x overlapping b, negative rtol / atol / maxiter /
 *   history_capacity, NaN tolerances, bad memspace, struct_size mismatch.
 * info.status: 0 converged; 1 maxiter reached; 2 a residual norm or estimate was not finite (NaN / Inf in b, x0 or the
 *   operator): x holds the last finished cycle.  The call returns BSM_OK for all three.  cycles = ceil(iterations / restart).
 *   a_products = iterations + one per cycle for the true residual (none for the first cycle with use_x0 == 0, where
 *   r = b); m_products (0 without M) = iterations + one per cycle that ran an iteration (x += M u).  With use_x0 != 0 the
 *   product op(A) x0 is enqueued before anything is known about b: a non-finite b then reports status 2 with
 *   a_products = 1, not 0.
 *   workspace / workspace_bytes: the device address and size of the allocation made by create (fixed for its life). */
typedef struct bsm_gmres_s *bsm_gmres_t;
typedef struct {
    int32_t struct_size; /* = sizeof(bsm_gmres_params) */
    int32_t use_x0;
    double rtol, atol;
    int64_t maxiter;
    int64_t history_capacity;
} bsm_gmres_params;
typedef struct {
    int32_t status, cycles;
    int64_t iterations;
    double residual; /* absolute: the last estimate (or true residual norm at a restart) */
    double bnorm;
    int64_t a_products, m_products;
    int64_t workspace_bytes;
    uint64_t workspace;
} bsm_gmres_info;
BSM_LAYOUT_ASSERT(sizeof(bsm_gmres_params) == 40 && offsetof(bsm_gmres_params, rtol) == 8 &&
                      offsetof(bsm_gmres_params, maxiter) == 24,
                  "bsm_gmres_params layout");
BSM_LAYOUT_ASSERT(sizeof(bsm_gmres_info) == 64 && offsetof(bsm_gmres_info, iterations) == 8 &&
                      offsetof(bsm_gmres_info, a_products) == 32 && offsetof(bsm_gmres_info, workspace) == 56,
                  "bsm_gmres_info layout");
int bsm_gmres_create(bsm_matrix_t A, int opA, bsm_matrix_t M, int opM, int vdtype, int32_t restart, bsm_gmres_t *out);
/* (S is a bsm_gmres_t: `struct bsm_gmres_s *` is the same type spelled out.  The spelling is an artefact -- the static
 * checker of the bindings, tests/test_julia_ccall_signatures.py, classifies a parameter as a pointer by its `*` or by the
 * two handle typedefs it knows --, not a second type: pass the bsm_gmres_t that bsm_gmres_create returned.) */
int bsm_gmres_solve(struct bsm_gmres_s *S, const void *b, void *x, const bsm_gmres_params *p, bsm_gmres_info *info,
                    double *history, int memspace, void *stream);
int bsm_gmres_destroy(struct bsm_gmres_s *S);

/* bsm_cg_*: preconditioned conjugate gradients for SYMMETRIC operators, nrhs = 1 .. BSM_CG_MAX_RHS right-hand sides in
 * lockstep, wholly on the device.  The short recurrence GMRES cannot use: 4 work vectors per right-hand side (5 with M)
 * instead of restart + 4, and 3 vector launches per iteration (4 with M) beside the products; the K systems advance on
 * ONE multi-column product op(A) P per iteration (bsm_mul_multi: the matrix is streamed once per batch of columns).
 * (No counterpart in the reference: its operators are LinearMaps handed to a Julia solver package.)
 *   Method, per column c:
 *     r = b - op(A) x0 (or b);  z = opM(M) r (or r);  p = z;  rz = <r, z>
 *     repeat:  q = op(A) p;  pq = <p, q>;  alpha = rz / pq;  x += alpha p;  r -= alpha q;  rn = ||r||_2
 *              z = opM(M) r (or r);  rz' = <r, z>;  beta = rz' / rz;  p = z + beta p;  rz = rz'
 *   method = BSM_CG_METHOD_CG:   <u, v> = sum conj(u_i) v_i -- real symmetric / Hermitian positive definite op(A), opM(M);
 *   method = BSM_CG_METHOD_COCG: <u, v> = sum u_i v_i       -- complex symmetric ones (S' = conj(S): the operators of a
 *     SymmetricBlockMatrix with complex blocks).  The two coincide for real types.  ||r|| is always the 2-norm.
 *   THE CALLER asserts that op(A) and opM(M) are symmetric / Hermitian: nothing checks it, and the solver takes any kind
 *   of handle and any op.  Column c is converged when rn_c <= tol_c = max(rtol * ||b_c||_2, atol).
 * create: one device allocation on A's device, reported in info: X, R, P, Q (and Z with M) as n x nrhs_max column-major
 *   with the leading dimension rounded up to whole 16-byte groups, the per-workgroup partial sums, the column states; a
 *   ring of pinned record slots and events.  vdtype (BSM_F32 .. BSM_C128) is the type of B and X; the (handle, vector)
 *   pairings are those of bsm_gmres_create: a handle of that vector type (a mixed-storage handle counts with its double
 *   vectors) goes through bsm_mul_multi, a real unmixed handle of the same precision under a complex vdtype through
 *   bsm_mul_multi_cvec (one column is bsm_mul / bsm_mul_cvec: the same entry).  The handles must outlive the solver.
 *   Refusals: null A or out, bad op / vdtype / method, another pairing, op(A) not square, M of another order or on another
 *   device, nrhs_max outside 1 .. BSM_CG_MAX_RHS: BSM_ERR_INVALID; a multi-device handle, or one that owns a row range
 *   only (bsm_options.own_lo / own_hi: its products define the owned rows of y alone): BSM_ERR_UNSUPPORTED; an
 *   analysis-only handle: BSM_ERR_DEVICE.
 * solve: B (n x nrhs, leading dimension ldb) and X (ldx), column-major, ldb / ldx >= max(n, 1), any element alignment.
 *   They are touched only by the start (B is read, X too with use_x0 != 0) and by the final copy-out, which writes the n
 *   rows of the nrhs columns of X and nothing else.  use_x0 == 0: the solve starts from zero (NaN in the incoming X does
 *   not survive).
 *   Kernels (csrc/bsm_cg.hip), launched as (row ranges, columns): cg_start (r, the shares of ||b||^2 and ||r||^2),
 *   cg_dot (<p, q>, <r, z>: one partial per workgroup and column), cg_update (x, r, the shares of ||r||^2 and, without M,
 *   of <r, r>), cg_dir (p; its workgroup 0 writes the column's state and record).  Per iteration: product, cg_dot,
 *   cg_update, cg_dir without M; product A, cg_dot, cg_update, product M, cg_dot, cg_dir with M.  Every workgroup of a
 *   column adds that column's partials itself in one fixed order: no scalar kernel, no floating-point atomic, nobody
 *   waits; a launch never reads a scalar that the same launch replaces (two slots alternating by iteration parity).
 *   The decisions are taken ON THE DEVICE: a column whose rn met its tolerance (status 0), whose rn is not finite
 *   (status 2: NaN / Inf in B, X0 or the operator) or that broke down -- pq == 0 or rz == 0 while rn > tol, status 3; no
 *   division by zero is executed -- is FROZEN from the next launch on: its workgroups return at once, x and r do not
 *   change again whatever the host enqueues.  The host enqueues iteration j + 1 before it waits for the record of
 *   iteration j (per column rn, ||b||, status and iteration count, in a pinned slot behind an event) and stops when no
 *   column is running or maxiter is reached: X, every column's iterations and history do not depend on how late it
 *   notices.  Columns still running after maxiter lockstep iterations report status 1.
 *   What lockstep costs: the multi-column products run on all nrhs columns until the LAST column stops -- the vector
 *   kernels skip a frozen column, the products do not --, so an iteration does not get cheaper as columns finish; and a
 *   solve that ends before maxiter has paid one product of A (and of M) more than it reports, for the iteration that was
 *   enqueued ahead of the last record.
 *   history (may be NULL): history[it * nrhs + c] = rn_c after iteration it + 1, it < history_capacity; a frozen column
 *   repeats its last value.  cols (may be NULL): nrhs entries.
 *   info: status = the largest column status; iterations = the largest column count; a_products = iterations (+ 1 with
 *   use_x0) and m_products = iterations + 1 with M, 0 without: the multi-column products the answer uses (the iteration
 *   enqueued ahead of the last record costs one more product on frozen columns, which is not counted).
 *   memspace: BSM_MEM_DEVICE -- B, X on A's device; BSM_MEM_HOST -- staged through device buffers the solver keeps from
 *   its first host solve on.  SYNCHRONOUS; runs wholly on `stream`; must not be graph-captured; one solve at a time per
 *   solver.  n == 0: status 0, nothing touched.
 *   BSM_ERR_INVALID: null S / p / info, null B / X with n > 0, nrhs outside 1 .. nrhs_max, ldb or ldx < max(n, 1), X
 *   overlapping B, negative or NaN rtol / atol, negative maxiter / history_capacity, bad memspace, graph capture, a
 *   struct_size mismatch.  The call returns BSM_OK for every column status. */
#define BSM_CG_MAX_RHS 16
enum { BSM_CG_METHOD_CG = 0, BSM_CG_METHOD_COCG = 1 };
struct bsm_cg_s;
typedef struct {
    int32_t struct_size; /* = sizeof(bsm_cg_params) */
    int32_t use_x0;
    double rtol, atol;
    int64_t maxiter;
    int64_t history_capacity; /* rows of `history` */
} bsm_cg_params;
typedef struct {
    int32_t status;            /* the largest column status */
    int32_t columns_converged; /* columns with status 0 */
    int64_t iterations;        /* lockstep iterations the answer uses: the largest column count */
    int64_t a_products, m_products;
    int64_t workspace_bytes;
    uint64_t workspace;
} bsm_cg_info;
typedef struct {
    int32_t status; /* 0 converged, 1 maxiter reached, 2 non-finite residual, 3 breakdown */
    int32_t reserved;
    int64_t iterations;
    double residual; /* absolute: ||r||_2 by the recurrence when the column stopped */
    double bnorm;
} bsm_cg_column;
BSM_LAYOUT_ASSERT(sizeof(bsm_cg_params) == 40 && offsetof(bsm_cg_params, rtol) == 8 && offsetof(bsm_cg_params, maxiter) == 24,
                  "bsm_cg_params layout");
BSM_LAYOUT_ASSERT(sizeof(bsm_cg_info) == 48 && offsetof(bsm_cg_info, iterations) == 8 && offsetof(bsm_cg_info, a_products) == 16 &&
                      offsetof(bsm_cg_info, workspace) == 40,
                  "bsm_cg_info layout");
BSM_LAYOUT_ASSERT(sizeof(bsm_cg_column) == 32 && offsetof(bsm_cg_column, iterations) == 8 && offsetof(bsm_cg_column, residual) == 16,
                  "bsm_cg_column layout");
/* (the handle is spelled `struct bsm_cg_s *` for the static checker of the bindings, as in bsm_gmres_solve) */
int bsm_cg_create(bsm_matrix_t A, int opA, bsm_matrix_t M, int opM, int vdtype, int32_t nrhs_max, int32_t method,
                  struct bsm_cg_s **out);
int bsm_cg_solve(struct bsm_cg_s *S, int32_t nrhs, const void *B, int64_t ldb, void *X, int64_t ldx, const bsm_cg_params *p,
                 bsm_cg_info *info, bsm_cg_column *cols /* nrhs, may be NULL */,
                 double *history /* history_capacity x nrhs, may be NULL */, int memspace, void *stream);
int bsm_cg_destroy(struct bsm_cg_s *S);

/* bsm_bicgstab_*: right-preconditioned BiCGSTAB for operators that need NOT be symmetric, nrhs = 1 .. BSM_CG_MAX_RHS
 * right-hand sides in lockstep, wholly on the device.  The short recurrence for what bsm_cg cannot take and bsm_gmres takes
 * one column at a time: 6 work vectors per right-hand side (7 with M) whatever the iteration count, instead of restart + 4,
 * two products per iteration, both of them ONE multi-column product on all K systems (bsm_mul_multi: the matrix is
 * streamed once per batch of columns), and no transposed product.  Parameters, info and columns are those of bsm_cg_*.
 * (No counterpart in the reference: its operators are LinearMaps handed to a Julia solver package.)
 *   Method, per column c, with <u, v> = sum conj(u_i) v_i always:
 *     r = b - op(A) x0 (or b);  rhat = r;  rho = <rhat, r>;  p = r
 *     repeat:  phat = opM(M) p (or p);  v = op(A) phat;  sigma = <rhat, v>;  alpha = rho / sigma
 *              x += alpha phat;  r -= alpha v  (r now holds s);  sn = ||r||_2
 *              shat = opM(M) r (or r);  t = op(A) shat;  ts = <t, r>;  tt = <t, t>
 *              sn <= tol_c:  the column converges HERE (x already holds the half step)
 *              omega = ts / tt;  x += omega shat;  r -= omega t;  rn = ||r||_2;  rho' = <rhat, r>
 *              beta = (rho' / rho) (alpha / omega);  p = r + beta (p - omega v);  rho = rho'
 *   Column c is converged when sn_c or rn_c <= tol_c = max(rtol * ||b_c||_2, atol); the starting residual is checked too
 *   (0 iterations).  The residual is that of the unpreconditioned system (right preconditioning).
 * create: one device allocation on A's device, reported in info: X, R, Rhat, P, V, T (and Z with M: it serves as phat and,
 *   after the half step has been accumulated into x, as shat) as n x nrhs_max column-major with the leading dimension
 *   rounded up to whole 16-byte groups, the per-workgroup partial sums, the column states; a ring of pinned record slots
 *   and events.  vdtype (BSM_F32 .. BSM_C128) is the type of B and X; the (handle, vector) pairings are those of
 *   bsm_cg_create: a handle of that vector type (a mixed-storage handle counts with its double vectors) goes through
 *   bsm_mul_multi, a real unmixed handle of the same precision under a complex vdtype through bsm_mul_multi_cvec.  The
 *   handles must outlive the solver.  Refusals: null A or out, bad op / vdtype, another pairing, op(A) not square, M of
 *   another order or on another device, nrhs_max outside 1 .. BSM_CG_MAX_RHS: BSM_ERR_INVALID; a multi-device handle, or
 *   one that owns a row range only (bsm_options.own_lo / own_hi): BSM_ERR_UNSUPPORTED; an analysis-only handle:
 *   BSM_ERR_DEVICE.
 * solve: B (n x nrhs, leading dimension ldb) and X (ldx), column-major, ldb / ldx >= max(n, 1), any element alignment.
 *   They are touched only by the start (B is read, X too with use_x0 != 0) and by the final copy-out, which writes the n
 *   rows of the nrhs columns of X and nothing else.  use_x0 == 0: the solve starts from zero (NaN in the incoming X does
 *   not survive).
 *   Kernels (csrc/bsm_bicgstab.hip), launched as (row ranges, columns): bicg_start (r = rhat, the shares of ||b||^2 and
 *   ||r||^2), bicg_dot (<rhat, v>; <t, s> and ||t||^2 in one pass: one partial per workgroup and column), bicg_half (x, r,
 *   the shares of ||s||^2), bicg_update (x, r, the shares of ||r||^2 and <rhat, r>), bicg_dir (p; its workgroup 0 writes
 *   the column's state and record).  Per iteration: [product M,] product A, bicg_dot, bicg_half, [product M,] product A,
 *   bicg_dot, bicg_update, bicg_dir.  Every workgroup of a column adds that column's partials itself in one fixed order:
 *   no scalar kernel, no floating-point atomic, nobody waits; alpha, omega and every decision are re-derived by each
 *   launch that needs them from the same partials, and a launch never reads a scalar that the same launch replaces (two
 *   slots alternating by iteration parity).
 *   The decisions are taken ON THE DEVICE, per iteration in this order:
 *     rho == 0 or sigma == 0 at the top: breakdown, status 3; nothing is written and the column's count does not advance;
 *     sn not finite: status 2;  sn <= tol_c: status 0;  else tt == 0, ts == 0 or a quotient ts / tt that underflows to 0:
 *       breakdown, status 3 -- all three with
 *       the half step in x, s in r, the iteration counted and sn as the residual (at n = 1 the method ends through
 *       sn <= tol_c with tt possibly zero: the order matters);
 *     rn not finite: status 2;  rn <= tol_c: status 0.
 *   No division by zero is executed.  A column that has a status is FROZEN from the next launch on: its workgroups return
 *   at once, x and r do not change again whatever the host enqueues (the products write V, T and Z only).  The host
 *   enqueues iteration j + 1 before it waits for the record of iteration j (per column the residual, ||b||, status and
 *   iteration count, in a pinned slot behind an event) and stops when no column is running or maxiter is reached: X,
 *   every column's iterations and history do not depend on how late it notices.  Columns still running after maxiter
 *   lockstep iterations report status 1.
 *   What lockstep costs: the multi-column products run on all nrhs columns until the LAST column stops -- the vector
 *   kernels skip a frozen column, the products do not --, and a solve that ends before maxiter has paid up to two
 *   products of A (and of M) more than it reports, for the iteration that was enqueued ahead of the last record.
 *   history (may be NULL): history[it * nrhs + c] = the residual norm of column c after iteration it + 1 (rn, or sn where
 *   the column ended at the half step), it < history_capacity; a frozen column repeats its last value.  cols (may be
 *   NULL): nrhs entries.
 *   info: status = the largest column status; iterations = the largest column count; a_products = 2 * iterations (+ 1
 *   with use_x0) and m_products = 2 * iterations with M, 0 without: the multi-column products the answer uses (the
 *   iteration enqueued ahead of the last record costs up to two more of each on frozen columns, which are not counted).
 *   memspace: BSM_MEM_DEVICE -- B, X on A's device; BSM_MEM_HOST -- staged through device buffers the solver keeps from
 *   its first host solve on.  SYNCHRONOUS; runs wholly on `stream`; must not be graph-captured; one solve at a time per
 *   solver.  n == 0: status 0, nothing touched.
 *   BSM_ERR_INVALID: null S / p / info, null B / X with n > 0, nrhs outside 1 .. nrhs_max, ldb or ldx < max(n, 1), X
 *   overlapping B, negative or NaN rtol / atol, negative maxiter / history_capacity, bad memspace, graph capture, a
 *   struct_size mismatch.  The call returns BSM_OK for every column status. */
struct bsm_bicgstab_s;
int bsm_bicgstab_create(bsm_matrix_t A, int opA, bsm_matrix_t M, int opM, int vdtype, int32_t nrhs_max,
                        struct bsm_bicgstab_s **out);
int bsm_bicgstab_solve(struct bsm_bicgstab_s *S, int32_t nrhs, const void *B, int64_t ldb, void *X, int64_t ldx,
                       const bsm_cg_params *p, bsm_cg_info *info, bsm_cg_column *cols /* nrhs, may be NULL */,
                       double *history /* history_capacity x nrhs, may be NULL */, int memspace, void *stream);
int bsm_bicgstab_destroy(struct bsm_bicgstab_s *S);

/* bsm_gmres_multi_*: right-preconditioned restarted GMRES(restart) for op(A) X = B on nrhs = 1 .. BSM_CG_MAX_RHS right-hand
 * sides in lockstep, wholly on the device (bsm_gmres_* above is this solver with one column): the method for operators
 * that need not be symmetric when the residual has to go down monotonically and no breakdown is acceptable, on ONE
 * multi-column product per iteration (bsm_mul_multi: the matrix is streamed once per batch of columns).  Parameters, info and columns are those of bsm_cg_*.  Per column it is the method
 * bsm_gmres_solve documents -- two classical Gram-Schmidt passes, Givens rotations, the estimate |g[j + 1]|, x += opM(M) V y
 * at the end of a cycle, the next cycle from the TRUE residual --, so column c of a lockstep solve is, as a method, the
 * stand-alone solve of b_c.  All columns start together and restart together, every `restart` iterations: a column's cycle
 * boundaries are the ones it would have alone.  Inside a cycle each column has its own basis, Hessenberg factor, rotations
 * and g.  (No counterpart in the reference: its operators are LinearMaps handed to a Julia solver package.)
 * create: one device allocation on A's device, reported in info: the basis V_0 .. V_restart, W, X (and Z with M) -- restart + 3
 *   matrices, restart + 4 with M -- as n x nrhs_max column-major with the leading dimension rounded up to whole 16-byte
 *   groups (basis vector i of ALL columns is one such matrix, so op(A) V_j is a plain multi-column product), per column the
 *   small arrays of a cycle and the per-workgroup partial sums of a pass, the column states; a ring of pinned record slots
 *   and events.  vdtype and the (handle, vector) pairings are those of bsm_cg_create.  The handles must outlive the solver.
 *   Refusals: those of bsm_cg_create (a handle that owns a row range only among them), and restart outside 1 ..
 *   BSM_GMRES_MAX_RESTART: BSM_ERR_INVALID.
 * solve: B, X, ldb, ldx, use_x0, memspace, stream, history layout, cols and the refusals as in bsm_cg_solve.
 *   Kernels (csrc/bsm_gmres_multi.hip), vector launches as (row ranges, columns): gm_start (r = B - op(A) X -> V_0, the shares
 *   of ||r||^2 and ||b||^2), gm_begin (V_0 /= beta; g = beta e_1; the decision of a start), per iteration [product M,] product
 *   A, twice gm_dot / gm_update (one partial per workgroup, basis vector and column; every workgroup adds them itself in one
 *   fixed order), gm_hess (one wave per column: the new Hessenberg column, rotation, estimate, the decision), gm_scale; at
 *   the end of a cycle gm_trsolve (one wave per column), gm_combine (U = V y), [product M,] gm_axpy.  No floating-point
 *   atomic, nobody waits, and a launch never reads a scalar that the same launch replaces (gm_begin and gm_hess read one
 *   slot of the state and write the other).
 *   The decisions are taken ON THE DEVICE.  Column c converges when its estimate is <= tol_c = max(rtol * ||b_c||_2, atol)
 *   (status 0: its answer uses exactly the iterations of the open cycle up to that one, added to x at the end of that
 *   cycle), or when the TRUE residual at a start or restart already meets it (status 0, no history row for it, `residual`
 *   is that true norm).  A non-finite norm or estimate gives status 2, and x_c holds its last finished cycle.  Status 3 is
 *   never reported: a lucky breakdown ||w|| = 0 is convergence (1 / ||w|| is replaced by 0, no NaN).  A column that has a
 *   status is FROZEN: the workgroups of every vector launch return before their first vector load, and the products write
 *   W and Z only, so nothing the host enqueues late reaches its x, count or history.
 *   The host only enqueues; it reads one record per gm_begin / gm_hess from the pinned ring, one step behind its enqueues.
 *   It ends a cycle early when no column runs, always enqueues the cycle's end (harmless on columns that owe nothing), and
 *   enqueues the restart without waiting.  maxiter bounds the lockstep iterations; columns still running after it report
 *   status 1; a cycle that maxiter cuts short has min(restart, maxiter - done) iterations.
 *   history[it * nrhs + c] = the residual ESTIMATE of column c after lockstep iteration it + 1, it < history_capacity; a
 *   frozen column repeats its last value (its `residual`).  Only gm_hess records fill rows.
 *   info: status = the largest column status; iterations = the largest column count, which also gives the cycles:
 *   ceil(iterations / restart).  a_products = iterations + one true-residual product per restart that found a column running
 *   (+ 1 with use_x0); m_products = iterations + one per cycle that ran an iteration, 0 without M.  These count multi-column
 *   products the answer uses.
 *   What lockstep costs: the products run on all nrhs columns until the last column stops, and every column keeps its own
 *   basis: the orthogonalisation does not share across columns.  The look-ahead: a solve that ends before maxiter has paid
 *   at most ONE product of A and one of M beyond these counts -- the iteration, or the restart's op(A) X, that was enqueued
 *   ahead of the record that showed no column running. */
struct bsm_gmres_multi_s;
int bsm_gmres_multi_create(bsm_matrix_t A, int opA, bsm_matrix_t M, int opM, int vdtype, int32_t nrhs_max, int32_t restart,
                           struct bsm_gmres_multi_s **out);
int bsm_gmres_multi_solve(struct bsm_gmres_multi_s *S, int32_t nrhs, const void *B, int64_t ldb, void *X, int64_t ldx,
                          const bsm_cg_params *p, bsm_cg_info *info, bsm_cg_column *cols /* nrhs, may be NULL */,
                          double *history /* history_capacity x nrhs, may be NULL */, int memspace, void *stream);
int bsm_gmres_multi_destroy(struct bsm_gmres_multi_s *S);

/* bsm_minres_*: symmetric-preconditioned MINRES (Paige and Saunders) for SYMMETRIC / HERMITIAN operators that need NOT be
 * definite -- shifted or Helmholtz-like near fields, saddle-point couplings --, nrhs = 1 .. BSM_CG_MAX_RHS right-hand sides in
 * lockstep, wholly on the device.  The short recurrence for what bsm_cg breaks down or diverges on and bsm_gmres_multi takes
 * with restart + 3 matrices: 7 work vectors per right-hand side (9 with M) whatever the iteration count, a residual norm
 * that does not grow (without M; with M it is the M-norm that is minimised), and ONE multi-column product op(A) Z per iteration (bsm_mul_multi: the matrix is streamed once per
 * batch of columns).  Parameters, info and columns are those of bsm_cg_*.
 * (No counterpart in the reference: its operators are LinearMaps handed to a Julia solver package.)
 *   Method, per column c.  Every scalar is REAL and held in the real type of vdtype; <u, v> is the real part of
 *   sum conj(u_i) v_i.  opM(M) must be symmetric / Hermitian POSITIVE definite (right preconditioning would not keep the
 *   symmetry); THE CALLER asserts that and the symmetry of op(A), as for bsm_cg.
 *     v_old = w_old = w = 0;  r = v = b - op(A) x0 (or b);  z = opM(M) v (or v);  gamma = sqrt<v, z>;  gamma_old = 1;
 *     eta = gamma;  s_old = s = 0;  c_old = c = 1
 *     repeat:  q = op(A) z;  delta = <z, q> / (gamma gamma);  ig = 1 / gamma
 *              v_new = (ig q - (delta ig) v) - (gamma / gamma_old) v_old
 *              z_new = opM(M) v_new (or v_new);  gamma_new = sqrt<v_new, z_new>
 *              a0 = c delta - c_old s gamma;  a1 = sqrt(a0 a0 + gamma_new gamma_new);  a2 = s delta + c_old c gamma;
 *              a3 = s_old gamma;  ia = 1 / a1;  c_new = a0 ia;  s_new = gamma_new ia
 *              w_new = ((ig z - a3 w_old) - a2 w) ia;  x += (c_new eta) w_new;  eta_new = -s_new eta
 *              r = (s_new s_new) r + (c_new eta_new / gamma_new) v_new   (gamma_new == 0: r = (s_new s_new) r);  rn = ||r||_2
 *              (v_old, v, z, w_old, w, gamma_old, gamma, eta, c_old, c, s_old, s) <- (v, v_new, z_new, w, w_new, gamma,
 *              gamma_new, eta_new, c, c_new, s, s_new)
 *   z is kept unnormalised: the 1 / gamma factors ride in the scalars, no pass scales a vector.  r is the CARRIED residual
 *   b - op(A) x of the unpreconditioned system, and column c is converged when rn_c <= tol_c = max(rtol * ||b_c||_2, atol),
 *   the rule of the other lockstep solvers -- not |eta|, which with M is the residual in the M-norm.  The starting residual is
 *   checked too (0 iterations; a zero column ends there with x = 0).
 * create: one device allocation on A's device, reported in info: X, R, V0, V1, W0, W1, Q (and Z0, Z1 with M) as n x nrhs_max
 *   column-major with the leading dimension rounded up to whole 16-byte groups, the per-workgroup partial sums, the column
 *   states; a ring of pinned record slots and events.  v_new is written into the storage of v_old, w_new into that of
 *   w_old, z_new beside z (w_new needs z after gamma_new is known); the host swaps the pointers by the parity of the
 *   iteration.  vdtype and the (handle, vector) pairings are those of bsm_cg_create.  The handles must outlive the solver.
 *   Refusals: those of bsm_cg_create but the method (a handle that owns a row range only among them).
 * solve: B, X, ldb, ldx, use_x0, memspace, stream, history layout, cols and the refusals as in bsm_cg_solve.
 *   Kernels (csrc/bsm_minres.hip), vector launches as (row ranges, columns): mr_start (r = v, the shares of ||b||^2 and
 *   ||r||^2, the zero vectors), mr_dot (<z, q>, <v_new, z_new>: one partial per workgroup and column), mr_lanczos (v_new;
 *   without M the shares of ||v_new||^2), mr_update (every workgroup derives gamma_new and the rotation from the partials
 *   and the state; w_new, x, r in one pass, the shares of ||r||^2), mr_decide (one wave per column: the decision, the state
 *   of the next iteration, the record).  Per iteration: product A, mr_dot, mr_lanczos, [product M, mr_dot,] mr_update,
 *   mr_decide.  No floating-point atomic, nobody waits, and a launch never reads a scalar that the same launch replaces
 *   (two slots alternating by iteration parity; mr_update leaves the rotation it derived beside them for mr_decide).
 *   The decisions are taken ON THE DEVICE: rn not finite: status 2;  rn <= tol_c: status 0;  breakdown, status 3: <v, z> of
 *   the start not a positive finite number while rn > tol_c, <v_new, z_new> negative or not finite (M is not positive
 *   definite, or op(A) holds NaN / Inf), a1 not a positive finite number -- in these two the iteration is not counted and x,
 *   r keep what the last complete iteration left --, gamma_new == 0 while rn > tol_c.  No division by zero and no root of a
 *   negative number is executed.  A column that has a status is FROZEN from the next launch on: its workgroups return before
 *   their first vector load, x and r do not change again whatever the host enqueues.  The host enqueues iteration j + 1
 *   before it waits for the record of iteration j and stops when no column is running or maxiter is reached: X, every
 *   column's iterations and history do not depend on how late it notices.  Columns still running after maxiter lockstep
 *   iterations report status 1.
 *   history[it * nrhs + c] = rn_c after iteration it + 1, it < history_capacity; a frozen column repeats its last value.
 *   info: status = the largest column status; iterations = the largest column count; a_products = iterations (+ 1 with
 *   use_x0) and m_products = iterations + 1 with M, 0 without; a solve that ends before maxiter has paid at most one product
 *   of A and one of M beyond these counts, for the iteration enqueued ahead of the last record. */
struct bsm_minres_s;
int bsm_minres_create(bsm_matrix_t A, int opA, bsm_matrix_t M, int opM, int vdtype, int32_t nrhs_max, struct bsm_minres_s **out);
int bsm_minres_solve(struct bsm_minres_s *S, int32_t nrhs, const void *B, int64_t ldb, void *X, int64_t ldx, const bsm_cg_params *p,
                     bsm_cg_info *info, bsm_cg_column *cols /* nrhs, may be NULL */,
                     double *history /* history_capacity x nrhs, may be NULL */, int memspace, void *stream);
int bsm_minres_destroy(struct bsm_minres_s *S);

/* bsm_lsqr_*: LSQR (Paige and Saunders) for RECTANGULAR, rank-deficient and damped least-squares problems --
 * over-determined fits and collocation systems, under-determined systems (the minimum-norm solution), singular square
 * operators --, nrhs = 1 .. BSM_CG_MAX_RHS right-hand sides in lockstep, wholly on the device.  The one solver here that
 * takes an op(A) that is not square, and the one that issues the ADJOINT product: per iteration one multi-column product
 * with op(A) and one with op(A)^H (bsm_mul_multi: the matrix is streamed once per batch of columns), 6 work vectors per
 * right-hand side whatever the iteration count (4 of X's length, 2 of B's).  Info and columns are those of bsm_cg_*.
 * (No counterpart in the reference: its operators are LinearMaps handed to a Julia solver package.)
 *   Method, per column c: it minimises ||b - op(A) x||^2 + damp^2 ||x - x0||^2.  Every scalar is REAL and held in the real
 *   type of vdtype; the norms are 2-norms, the real parts of sum conj(u_i) u_i.  The Lanczos vectors u~ (m = rows(op(A))
 *   entries) and v~ (n = cols(op(A)) entries) are kept UNNORMALISED, u~ = beta u and v~ = alpha v: the 1 / alpha, 1 / beta
 *   factors ride in the scalars, no pass scales a vector.
 *     start:  u~ = b - op(A) x0 (or b);  beta = ||u~||;  bnorm = ||b||;  tol_c = max(rtol bnorm, atol)
 *             v~ = op(A)^H u~ / beta;  alpha = ||v~||;  w = v~ / alpha;  phibar = beta;  rhobar = alpha;  res2 = 0;  anorm = 0
 *             rnorm = beta;  arnorm = alpha beta;  the decision below is taken here too (0 iterations)
 *     repeat: u~ = op(A) v~ / alpha - (alpha / beta) u~;  beta' = ||u~||
 *             anorm = sqrt(anorm^2 + alpha^2 + beta'^2 + damp^2)
 *             v~ = op(A)^H u~ / beta' - (beta' / alpha) v~;  alpha' = ||v~||      (beta' == 0: v~ = 0, alpha' = 0, no division)
 *             rhobar1 = sqrt(rhobar^2 + damp^2);  cs1 = rhobar / rhobar1;  sn1 = damp / rhobar1;  psi = sn1 phibar;
 *             phibar = cs1 phibar
 *             rho = sqrt(rhobar1^2 + beta'^2);  c = rhobar1 / rho;  s = beta' / rho;  theta = s alpha';  rhobar = -c alpha';
 *             phi = c phibar;  phibar = s phibar;  tau = s phi
 *             x += (phi / rho) w;  w = v~ / alpha' - (theta / rho) w          (alpha' == 0: w is not needed again)
 *             res2 += psi^2;  rnorm = sqrt(phibar^2 + res2);  arnorm = alpha' |tau|
 *     decide: rnorm or arnorm not finite: status 2;  rnorm <= tol_c: 0;  arnorm <= ntol anorm rnorm: 0;  alpha' == 0 or
 *             beta' == 0: 0 (the Krylov space ended: the iterate IS the solution);  else the column runs on
 *   rnorm is the estimate of ||[b; damp x0] - [op(A); damp I] x||, without damp that is ||b - op(A) x||; arnorm estimates
 *   the norm of the normal-equation residual op(A)^H r - damp^2 (x - x0); anorm is the running Frobenius-norm estimate of
 *   the bidiagonal factor (scipy's anorm).  The FIRST rule ends a column of a consistent system, the SECOND one a column whose
 *   residual cannot vanish.  With use_x0 the damping term pulls towards X0, not towards zero.  Status 3 is never reported:
 *   every breakdown of LSQR is convergence.  No division by zero and no root of a negative number is executed.
 * create: one device allocation on A's device, reported in info: X, V, W, P (n rows) and U, Q (m rows) as column-major
 *   matrices of nrhs_max columns with the leading dimension rounded up to whole 16-byte groups, the per-workgroup partial
 *   sums of both lengths, the column states; a ring of pinned record slots and events.  vdtype and the (handle, vector)
 *   pairings are those of bsm_cg_create.  op(A)^H is BSM_OP_C of the handle for opA = BSM_OP_N, BSM_OP_N for BSM_OP_C, and
 *   for BSM_OP_T BSM_OP_N on a real handle; on a COMPLEX handle opA = BSM_OP_T would need conj(A), which no product offers:
 *   BSM_ERR_UNSUPPORTED.  The other refusals are those of bsm_cg_create without M, method and the square requirement.  The
 *   handle must outlive the solver.  There is no preconditioner argument.
 * solve: B (m x nrhs, ldb >= max(m, 1)) and X (n x nrhs, ldx >= max(n, 1)), column-major, any element alignment, touched as
 *   in bsm_cg_solve.  use_x0, memspace, stream, history layout (rnorm per row), cols and the refusals as in bsm_cg_solve
 *   with bsm_lsqr_params in the place of bsm_cg_params; ntol or damp negative or NaN: BSM_ERR_INVALID.  arnorm, anorm (may
 *   be NULL): nrhs doubles each, the two estimates of every column when it stopped, copied out once after the solve's final
 *   synchronisation.  m == 0 or n == 0: status 0, B and X untouched.
 *   Kernels (csrc/bsm_lsqr.hip).  The vectors have two lengths, so a solve runs on TWO grids: (krylov_grid(m), columns) for
 *   U and Q, (krylov_grid(n), columns) for X, V, W, P; a kernel of the n-grid that needs ||u~||^2 adds the partials the
 *   m-grid left.  ls_start (m: u~, the shares of ||b||^2 and ||u~||^2), ls_begin (n: v~ = P / beta, the shares of ||v~||^2),
 *   ls_u (m), ls_v (n; at iteration 0 it also leaves w = v~ / alpha), ls_update (n: every workgroup derives alpha', beta',
 *   the rotations and the decision from the partials and the state -- lsqr_step of csrc/bsm_lsqr.h, one function for host
 *   and device --; x and w in one pass), ls_decide (one wave per column: the state of the next iteration, the record).  Per
 *   iteration: product op(A), ls_u, product op(A)^H, ls_v, ls_update, ls_decide.  No floating-point atomic, nobody waits,
 *   and a launch never reads a scalar that the same launch replaces (two slots alternating by iteration parity; ls_update
 *   leaves the step it derived beside them for ls_decide).  A column that has a status is FROZEN from the next launch on.
 *   Run-to-run reproducibility: the SOLVER's kernels add in one fixed order, so two runs of a solve agree to the bit where
 *   BOTH products do.  One of the two products of an iteration is always a transposed one: on a handle without a second
 *   ordering (bsm_options.transpose_image = 0, the default) it accumulates with floating-point atomics, the last bits of X
 *   and of the estimates may then differ from run to run, and a count may move by one.  With transpose_image = 1 both
 *   products are forward passes (exclusive stores on a conflict-free operator) and X, counts and history are bit-identical.
 *   The solvers above never issue a transposed product unless asked to (opA), so this is particular to bsm_lsqr.
 *   The host enqueues iteration j + 1 before it waits for the record of iteration j and stops when no column is running or
 *   maxiter is reached: X, every column's iterations and history do not depend on how late it notices.
 *   info: a_products = 2 * iterations + 1 (+ 1 with use_x0), m_products = 0; a solve that ends before maxiter has paid at
 *   most two products beyond that, for the iteration enqueued ahead of the last record. */
typedef struct {
    int32_t struct_size; /* = sizeof(bsm_lsqr_params) */
    int32_t use_x0;
    double rtol, atol; /* rnorm <= max(rtol ||b||, atol) */
    double ntol;       /* arnorm <= ntol anorm rnorm */
    double damp;
    int64_t maxiter;
    int64_t history_capacity; /* rows of `history` */
} bsm_lsqr_params;
BSM_LAYOUT_ASSERT(sizeof(bsm_lsqr_params) == 56 && offsetof(bsm_lsqr_params, rtol) == 8 && offsetof(bsm_lsqr_params, ntol) == 24 &&
                      offsetof(bsm_lsqr_params, maxiter) == 40,
                  "bsm_lsqr_params layout");
struct bsm_lsqr_s;
int bsm_lsqr_create(bsm_matrix_t A, int opA, int vdtype, int32_t nrhs_max, struct bsm_lsqr_s **out);
int bsm_lsqr_solve(struct bsm_lsqr_s *S, int32_t nrhs, const void *B, int64_t ldb, void *X, int64_t ldx, const bsm_lsqr_params *p,
                   bsm_cg_info *info, bsm_cg_column *cols /* nrhs, may be NULL */,
                   double *history /* history_capacity x nrhs, may be NULL */, double *arnorm /* nrhs, may be NULL */,
                   double *anorm /* nrhs, may be NULL */, int memspace, void *stream);
int bsm_lsqr_destroy(struct bsm_lsqr_s *S);

/* bsm_poly_*: a POLYNOMIAL PRECONDITIONER as a handle.  bsm_poly_create returns a bsm_matrix_t whose product is z = p(A) x,
 * a fixed polynomial in an operator handle A and an optional inner preconditioner handle D (e.g. the block-Jacobi handle
 * of A; NULL: the identity).  Because it is a bsm_matrix_t, bsm_mul and bsm_mul_multi apply it and every bsm_*_create above
 * takes it as (M, opM): a solver trades outer iterations -- where its dot products, Gram-Schmidt passes and decisions are
 * paid -- for multi-column products, the matrix streamed once for up to BSM_CG_MAX_RHS columns.
 * (No counterpart in the reference: its operators are LinearMaps handed to a Julia solver package.)
 *   The recurrence, with REAL coefficients a[0 .. steps), b[0 .. steps) (a[0] is ignored), on the operand x:
 *     r_0 = x;  d_0 = b_0 D r_0
 *     k = 0 .. steps - 2:   r_{k+1} = r_k - A d_k;   d_{k+1} = a_{k+1} d_k + b_{k+1} D r_{k+1}
 *     p(A) x = d_0 + d_1 + .. + d_{steps-1};   y = alpha p(A) x + beta y   (beta_strong_zero as in bsm_mul)
 *   steps - 1 products with A and steps with D per product of the composed handle.  The host computes the coefficients; two
 *   families matter.  Chebyshev for a spectrum of D A inside [lmin, lmax], 0 < lmin < lmax (Saad, Iterative Methods for
 *   Sparse Linear Systems, Alg. 12.1):  theta = (lmax + lmin) / 2, delta = (lmax - lmin) / 2, sigma = theta / delta,
 *   rho_0 = 1 / sigma, b_0 = 1 / theta;  rho_{k+1} = 1 / (2 sigma - rho_k), a_{k+1} = rho_{k+1} rho_k, b_{k+1} = 2 rho_{k+1} /
 *   delta.  Neumann / Richardson: a_k = 0, b_k = omega, which converges as steps grows iff rho(I - omega D A) < 1.
 *   op: BSM_OP_T / BSM_OP_C on the composed handle run the same recurrence with op composed onto opA and opD -- right because
 *   the coefficients are real.  A composition that needs conj(A) or conj(D) of a COMPLEX handle (BSM_OP_T onto BSM_OP_C or
 *   the reverse) is BSM_ERR_UNSUPPORTED, as in bsm_lsqr_create.
 * create: vdtype is the type of the vectors the composed handle takes; the (handle, vector) pairings of A and D are those
 *   of bsm_cg_create (a real handle serves a complex vdtype of its precision, a mixed-storage one its vector type).  ONE
 *   device allocation on A's device (bsm_poly_info, bsm_stats.device_bytes): R, d, acc, Q (and T = D R with D) as
 *   column-major matrices of nrhs_max columns, the leading dimension rounded up to whole 16-byte groups, the padding zero.
 *   Refused, before anything is allocated and in this order: null A / out, a bad op, a vdtype that is no vector type;
 *   steps outside 1 .. BSM_POLY_MAX_STEPS, null a / b, a coefficient that is not finite; nrhs_max outside 1 ..
 *   BSM_CG_MAX_RHS; op(A) not square, D of another order; a pairing bsm_cg_create refuses (all BSM_ERR_INVALID); a
 *   multi-device handle (BSM_ERR_UNSUPPORTED), an analysis-only handle (BSM_ERR_DEVICE), a handle that owns a row range only
 *   (BSM_ERR_UNSUPPORTED), A and D on different devices (BSM_ERR_INVALID); a composed handle as A or D (BSM_ERR_UNSUPPORTED).
 *   A and D must outlive the composed handle, which bsm_destroy frees.  It holds HANDLES, not values: the next product sees
 *   a bsm_update_blocks of A or D.
 * product: bsm_mul / bsm_mul_multi with vectors of vdtype in device memory; any ldx, ldy >= max(n, 1), any element
 *   alignment; X is read and n rows of nrhs columns of Y are written element by element, nothing else is touched.  nrhs >
 *   nrhs_max runs in batches of nrhs_max columns.  After create a product allocates nothing and synchronises nothing: it
 *   only enqueues on the caller's stream.  Refused: the _cvec entries (BSM_ERR_UNSUPPORTED: to precondition complex vectors
 *   over real handles, create with a complex vdtype), BSM_MEM_HOST (BSM_ERR_UNSUPPORTED), a stream that is being captured
 *   (BSM_ERR_UNSUPPORTED).  ONE product may be in flight per composed handle -- it has one workspace; products on other
 *   streams or threads are the caller's to order, as for bsm_update_blocks.  Run to run the result is bit-identical
 *   wherever the products of A and D are (the kernels between them, csrc/bsm_poly.hip, have no reduction).
 * every other entry point that takes a bsm_matrix_t -- bsm_rowcolvals, bsm_submatrices, bsm_diag, bsm_update_blocks,
 *   bsm_value_passes, bsm_get_bookkeeping, bsm_get_image, bsm_part_info, bsm_mul_parts -- answers BSM_ERR_UNSUPPORTED for a
 *   composed handle; bsm_stats reports nnz = 0 and the workspace as device_bytes.
 * bsm_poly_info: steps, the coefficients as held (a, b: capacity BSM_POLY_MAX_STEPS, may be NULL) and the bytes of the
 *   workspace; BSM_ERR_INVALID for a handle that is not a composed one. */
#define BSM_POLY_MAX_STEPS 64
int bsm_poly_create(bsm_matrix_t A, int opA, bsm_matrix_t D /* may be NULL */, int opD, int vdtype,
                    int32_t nrhs_max /* 1 .. BSM_CG_MAX_RHS */, int32_t steps, const double *a, const double *b,
                    bsm_matrix_t *out);
int bsm_poly_info(bsm_matrix_t M, int32_t *steps, double *a, double *b /* capacity BSM_POLY_MAX_STEPS, may be NULL */,
                  int64_t *workspace_bytes);

/* bsm_krylov_combine: the compression of a tall basis by a small REAL matrix, beside bsm_krylov_orth the second building
 * block of a caller's Krylov method -- the thick restart of a Lanczos run, and the way Ritz vectors leave it:
 *     Out[:, c] = sum_{j < m} V[:, j] S[j, c]   for c < k;      carry >= 0:  Out[:, k] = V[:, carry]
 * V: n x >= max(m, carry + 1), Out: n x (k, or k + 1 with a carry), column-major device matrices of dtype (BSM_F32 ..
 * BSM_C128), ldv, ldo >= max(n, 1), ANY element alignment.  S: m x k, column-major with lds >= m, in device memory, of the REAL
 * type of dtype (float for BSM_F32 / BSM_C64, double for BSM_F64 / BSM_C128): the projected matrix of a Hermitian operator is
 * real symmetric, so its eigenvectors are real, and a complex column of n entries is walked as 2 n reals.
 * The sum runs over j ascending with one fused multiply-add per term, in the precision of dtype: the result is fixed to the
 * bit, run to run and whatever the launch geometry.  Out == V with ldo == ldv works IN PLACE (a row of the output depends on
 * the same row of V only): a workgroup stages a tile of rows x m in LDS, V is read once, nothing is allocated, and m + 1
 * columns serve a whole restarted solve.  bsm_krylov_combine_tile(dtype, m): the rows (elements) of that tile -- as many
 * whole waves of real rows as fit into 128 KiB of LDS beside each other, at most 1024 reals:
 * min(1024, floor(131072 / (m * sizeof(real)) / 64) * 64) reals, half as many complex elements.
 * The call only enqueues on `stream`; it synchronises nothing and may be graph-captured.
 * Refused (BSM_ERR_INVALID): a dtype that is no vector type; n < 0; m outside 1 .. BSM_GMRES_MAX_RESTART; k outside 0 .. m;
 * carry outside -1 .. m; ldv or ldo < max(n, 1); lds < m; a null pointer that is needed (S with k > 0; V, Out with n > 0);
 * Out overlapping V in any way other than Out == V with ldo == ldv; S overlapping Out (in place: V).  k == 0 with a carry
 * moves one column; n == 0 is legal. */
int64_t bsm_krylov_combine_tile(int dtype, int64_t m);
int bsm_krylov_combine(int dtype, int64_t n, int64_t m, int64_t k, const void *V, int64_t ldv, const void *S, int64_t lds, void *Out,
                       int64_t ldo, int64_t carry, void *stream);

/* bsm_eigsh_*: `nev` EXTREME EIGENPAIRS of op(A) for an A the caller asserts to be real symmetric / complex Hermitian (nothing
 * checks that, as for bsm_cg), by thick-restart Lanczos -- the Hermitian Krylov-Schur method (Stewart; Wu and Simon), what
 * KrylovKit's eigsolve runs on a Hermitian LinearMap --, the basis, the products, the orthogonalisation and the restart on
 * the device.  (No counterpart in the reference: its operators are LinearMaps handed to a Julia eigensolver package.)
 *   Recurrence.  V holds ncv + 1 columns.  v_0 = v0 / ||v0||.  Step j of a cycle (j = start .. ncv - 1; start = 0 in the first
 *   cycle, `keep` after a restart):
 *       w = op(A) v_j                      one bsm_mul, written straight into column j + 1
 *       h = V[:, 0:j+1]^H w;  w -= V[:, 0:j+1] h      TWICE (classical Gram-Schmidt with one reorthogonalisation, the fused pass
 *                                          of bsm_krylov_orth); the coefficients of both passes add up in column j of H
 *       alpha_j = Re H[j, j];  beta_j = ||w||;  v_{j+1} = w / beta_j    (beta_j zero or not finite: v_{j+1} = 0, nothing divided)
 *   No host read happens inside a cycle; it ends with ONE device-to-host copy (diag(H), beta, ||v0||) and one synchronisation.
 *   The host keeps the real symmetric projected matrix T (ncv x ncv, double): after a restart its leading keep x keep part is
 *   diag(theta kept) with the arrow row T[keep, i] = beta_m S[m - 1, i] (taken analytically, m = ncv), the new columns take
 *   alpha_j on and beta_j beside the diagonal.  T = S diag(theta) S^T by a cyclic Jacobi method with a fixed sweep order
 *   (csrc/bsm_eig.h), theta ascending.  The rotations leave S orthonormal to about ncv eps only; the columns that go to the
 *   device (the kept ones of a restart, the wanted ones at the end) are made orthonormal to working precision on the host
 *   first, by two modified Gram-Schmidt passes in the order of the selection.
 *   Selection (`which`) of `count` Ritz values, and the order they are reported in:  BSM_EIGSH_LA the largest, largest first;
 *   BSM_EIGSH_SA the smallest, smallest first;  BSM_EIGSH_BE ceil(count / 2) from the top, largest first, then the rest from the
 *   bottom, smallest first;  BSM_EIGSH_LM the largest |theta|, largest first (of two equal magnitudes the positive one first).
 *   Estimate and tolerance.  The residual estimate of Ritz pair i is |beta_m S[m - 1, i]|.  anorm = the largest |theta| seen in
 *   the solve, a lower bound of ||op(A)||_2.  Converged: every wanted pair has estimate <= max(rtol anorm, atol).
 *   Restart.  keep = min(ncv - 1, nev + (ncv - nev) / 2); the keep pairs are selected by the same rule as the wanted ones; S is
 *   uploaded, V[:, 0:keep] = V[:, 0:ncv] S[:, kept] by bsm_krylov_combine IN PLACE with the residual vector v_m carried to column
 *   keep; the next cycle starts at step keep.  The basis is never duplicated.
 *   End.  X[:, i] = V S[:, wanted_i] through the same kernel into the caller's matrix, every column scaled to norm one (a kept
 *   column's norm drifts by a rounding error per restart), then the TRUE residuals
 *   ||op(A) x_i - theta_i x_i||: Q = op(A) X by bsm_mul_multi in batches of at most 16 columns, one partial per workgroup and
 *   column, one wave per column adds them in a fixed order.  No floating-point atomic in the unit's own kernels, nobody waits.
 * create: vdtype must be the handle's own vector type (a mixed-storage handle solves in double; a real handle under a complex
 *   vdtype has no use here: BSM_ERR_INVALID).  1 <= nev, nev + 2 <= ncv <= min(n, BSM_GMRES_MAX_RESTART).  ONE device allocation,
 *   reported in info: V (ncv + 1 columns), a block Q of min(nev, 16) columns, H (ncv x ncv), beta, S, theta and the partials;
 *   leading dimensions rounded up to whole 16-byte groups.  Refused, before anything is allocated: null A / out, a bad op, a
 *   vdtype that is no vector type (BSM_ERR_INVALID); a composed handle (BSM_ERR_UNSUPPORTED); op(A) not square, a vdtype other
 *   than the handle's own (BSM_ERR_INVALID); a multi-device handle (BSM_ERR_UNSUPPORTED), an analysis-only handle
 *   (BSM_ERR_DEVICE), a handle that owns a row range only (BSM_ERR_UNSUPPORTED); nev / ncv outside their ranges
 *   (BSM_ERR_INVALID).  The handle must outlive the solver.
 * solve: v0 (n entries) and X (n x nev, ldx >= max(n, 1), column-major), any element alignment; BSM_MEM_HOST operands are
 *   staged through device buffers the solver keeps.  pairs: nev entries.  Synchronous.
 *   info.status:  0 converged;  1 maxcycles reached (X and pairs hold all nev Ritz pairs as they stand, nconv = nev);  2 a norm,
 *   a coefficient or a Ritz value is not finite (nconv = 0, X is not written);  3 the Krylov space ended before nev pairs
 *   existed: beta_j was exactly zero with j + 1 < nev (nconv = j + 1, the pairs of that invariant subspace, exact; a zero v0
 *   gives nconv = 0).  A space that ends with j + 1 >= nev is convergence: its Ritz pairs are exact.
 *   pairs[i], i < nconv, in the order of `which`: value, estimate, residual (the true one; with vectors = 0 neither X nor
 *   the residual pass is produced and residual = estimate).  Entries i >= nconv are NaN; columns i >= nconv of X are untouched.
 *   X is orthonormal to working precision.  a_products = Lanczos steps + residual columns.
 *   Refused (BSM_ERR_INVALID): null S, p, info, pairs, v0; a struct_size mismatch; a bad memspace or which; rtol or atol negative
 *   or NaN; maxcycles < 1; with vectors: null X, ldx < max(n, 1), X overlapping v0; a stream that is being captured.
 *   Run to run, value, X, cycles and the residuals are bit-identical wherever the product of the handle is (the forward
 *   product of a conflict-free or gather / coloured operator; see bsm_lsqr above for the transposed product).
 * Not in it: interior eigenvalues / shift-invert, the generalised problem or a preconditioner, multiplicities (a single-vector
 *   Krylov space sees one vector of an eigenspace), singular values (bsm_svds below), block Lanczos / LOBPCG, locking beyond what the thick
 *   restart keeps. */
typedef enum { BSM_EIGSH_LA = 0, BSM_EIGSH_SA = 1, BSM_EIGSH_BE = 2, BSM_EIGSH_LM = 3 } bsm_eigsh_which;
typedef struct {
    int32_t struct_size; /* = sizeof(bsm_eigsh_params) */
    int32_t which;       /* bsm_eigsh_which */
    double rtol, atol;   /* estimate <= max(rtol anorm, atol) */
    int32_t maxcycles;
    int32_t vectors;     /* 0: values and estimates only */
} bsm_eigsh_params;
typedef struct {
    int32_t status, nconv, cycles, reserved;
    int64_t a_products;
    double anorm;
    int64_t workspace_bytes;
    uint64_t workspace; /* device address of the allocation */
} bsm_eigsh_info;
typedef struct {
    double value, estimate, residual;
} bsm_eigsh_pair;
BSM_LAYOUT_ASSERT(sizeof(bsm_eigsh_params) == 32 && offsetof(bsm_eigsh_params, rtol) == 8 && offsetof(bsm_eigsh_params, maxcycles) == 24,
                  "bsm_eigsh_params layout");
BSM_LAYOUT_ASSERT(sizeof(bsm_eigsh_info) == 48 && offsetof(bsm_eigsh_info, a_products) == 16 && sizeof(bsm_eigsh_pair) == 24,
                  "bsm_eigsh_info layout");
struct bsm_eigsh_s;
int bsm_eigsh_create(bsm_matrix_t A, int opA, int vdtype, int32_t nev, int32_t ncv, struct bsm_eigsh_s **out);
int bsm_eigsh_solve(struct bsm_eigsh_s *S, const void *v0, void *X /* may be NULL with vectors = 0 */, int64_t ldx,
                    const bsm_eigsh_params *p, bsm_eigsh_info *info, bsm_eigsh_pair *pairs /* nev */, int memspace, void *stream);
int bsm_eigsh_destroy(struct bsm_eigsh_s *S);

/* bsm_svds_*: the `nsv` LARGEST or SMALLEST SINGULAR TRIPLETS (sigma_i, u_i, v_i), op(A) v_i = sigma_i u_i, op(A)^H u_i = sigma_i v_i,
 * of a rectangular or nonsymmetric op(A) (m x n), by thick-restart Golub-Kahan-Lanczos bidiagonalisation with full two-sided
 * reorthogonalisation (Baglama and Reichel; what KrylovKit's svdsolve runs on a LinearMap), the bases, the products, the
 * orthogonalisation, the restart and the true residuals on the device.  The two-sided sibling of bsm_eigsh, and the first
 * eigen-type solver that uses the transposed half of the engine: ||A||_2, sigma_min, the 2-norm condition number, a leading
 * or trailing singular subspace.  (No counterpart in the reference: its operators are LinearMaps handed to KrylovKit.)
 *   Recurrence.  It always starts in the SHORT space: with l = max(m, n), s = min(m, n) it runs on B = op(A) if m >= n and on
 *   B = op(A)^H otherwise, U and V exchanged on the way out.  (Started in the long space of a 400 x 600 operator it never converges
 *   for the smallest values: it sees the 200-dimensional null space.)  P (s x (ncv + 1)) holds the right vectors of B, Q (l x
 *   ncv) the left ones; p_0 = v0 / ||v0||, v0 of s entries.  Step j of a cycle (j = start .. ncv - 1; start = 0 in the first
 *   cycle, `keep` after a restart):
 *       q = B p_j                          one bsm_mul, written straight into Q[:, j]
 *       h = Q[:, 0:j]^H q;  q -= Q[:, 0:j] h          TWICE (the fused pass of bsm_krylov_orth)
 *       alpha_j = ||q||;  q_j = q / alpha_j          (alpha_j zero or not finite: q_j = 0, nothing divided)
 *       r = B^H q_j                        one bsm_mul, written straight into P[:, j + 1]
 *       h = P[:, 0:j+1]^H r;  r -= P[:, 0:j+1] h      TWICE
 *       beta_j = ||r||;  p_{j+1} = r / beta_j        (the same guard)
 *   No host read happens inside a cycle; it ends with ONE device-to-host copy (the alpha, the beta, ||v0||) and one
 *   synchronisation.  The host keeps the real upper-triangular projected matrix Bp (ncv x ncv, double), B P = Q Bp: alpha_j on
 *   the diagonal, beta_j beside it (row j, column j + 1); after a restart its leading keep x keep part is diag(sigma kept) and
 *   column keep holds the arrow rho_i = beta_m X[m - 1, i] (taken analytically, m = ncv).  Bp Y = X diag(sigma) by a one-sided
 *   (Hestenes) Jacobi method in double with a fixed sweep order (csrc/bsm_svds.h): a column pair is skipped when its inner
 *   product is within sqrt(ncv) eps of the product of its norms, at most 60 sweeps, sigma descending, deterministic; a column of
 *   Bp Y that is zero to ncv eps sigma_max gets its X column completed by Gram-Schmidt from the unit vectors in index order.  The
 *   columns of X and Y that go to the device are made orthonormal to working precision on the host first, by two modified
 *   Gram-Schmidt passes in the order of the selection.
 *   Selection (`which`): BSM_SVDS_LM the largest, largest first; BSM_SVDS_SM the smallest, smallest first.
 *   Estimate and tolerance.  The estimate of triplet i is |beta_m X[m - 1, i]| = ||B^H u_i - sigma_i v_i|| in exact arithmetic (B
 *   v_i = sigma_i u_i holds by construction).  anorm = the largest sigma seen in the solve, a lower bound of ||op(A)||_2.
 *   Converged: every wanted triplet has estimate <= max(rtol anorm, atol).
 *   Restart.  keep = min(ncv - 1, nsv + (ncv - nsv) / 2), selected by the same rule as the wanted ones; P[:, 0:keep] = P[:, 0:ncv]
 *   Y[:, kept] IN PLACE with p_m carried to column keep, Q[:, 0:keep] = Q X[:, kept] in place with no carry: two
 *   bsm_krylov_combine launches.  The bases are never duplicated.
 *   End.  V and U leave through the same kernel into the caller's matrices, every column scaled to norm one, then the TRUE
 *   residuals r_av = ||op(A) v_i - sigma_i u_i|| and r_ahu = ||op(A)^H u_i - sigma_i v_i||: two bsm_mul_multi per batch of at most
 *   16 columns, ONE launch pair per batch that leaves one partial per workgroup and column for both residuals, over the m-row
 *   grid and the n-row grid, and adds them in a fixed order, one wave per column.  No floating-point atomic in the unit's own
 *   kernels, nobody waits.
 * create: vdtype must be the handle's own vector type (a mixed-storage handle solves in double).  1 <= nsv, nsv + 2 <= ncv <=
 *   min(m, n, BSM_GMRES_MAX_RESTART).  ONE device allocation, reported in info: P (ncv + 1 columns of s rows), Q (ncv columns of l
 *   rows), two residual blocks of min(nsv, 16) columns, one on each grid, and the small arrays; leading dimensions rounded up to
 *   whole 16-byte groups.  Refused, before anything is allocated: what bsm_eigsh_create refuses except a non-square op(A); opA =
 *   BSM_OP_T on a complex handle (BSM_ERR_UNSUPPORTED: op(A)^H would be conj(A), as in bsm_lsqr_create).  The handle must
 *   outlive the solver; it holds the HANDLE, not values: the next solve sees a bsm_update_blocks.
 * solve: v0 (min(m, n) entries), U (m x nsv, ldu >= max(m, 1)), V (n x nsv, ldv >= max(n, 1)), column-major, any element
 *   alignment; BSM_MEM_HOST operands are staged through device buffers the solver keeps.  triplets: nsv entries.  Synchronous.
 *   info.status:  0 converged;  1 maxcycles reached (all nsv triplets are returned as they stand, nconv = nsv);  2 a norm or a
 *   singular value is not finite, or the Jacobi method hit its sweep cap (nconv = 0, U and V are not written);  3 the space
 *   ended before nsv triplets existed: a beta_j -- or an alpha_j, which gives q_j = 0 and beta_j = 0 with it -- was exactly zero
 *   with j + 1 < nsv (nconv = j + 1 triplets of that invariant pair of subspaces, exact; a zero v0 gives nconv = 0).  A space that
 *   ends with j + 1 >= nsv is convergence.  A triplet whose alpha_j was exactly zero has sigma = 0 and the ZERO vector on the long
 *   side (the recurrence offers no left null vector; both residuals are zero all the same).  Where that alpha_j is rounding
 *   noise instead of zero -- a singular SQUARE operator whose space is exhausted, ncv = n -- u_i is a unit vector of noise: the
 *   estimate is tiny, and residual_ahu, the TRUE one, is what shows it.
 *   triplets[i], i < nconv, in the order of `which`: value, estimate, residual_av, residual_ahu (the true ones; with vectors = 0
 *   neither U, V nor the residual pass is produced, and the estimate stands for the residual of the product with B^H, zero for
 *   the other one).  Entries i >= nconv are NaN; columns i >= nconv of U and V are untouched.  U and V are orthonormal to
 *   working precision.  a_products = 2 * steps + 2 * nconv, steps = ncv + (cycles - 1)(ncv - keep); with vectors = 0: 2 * steps.
 *   Refused (BSM_ERR_INVALID): null S, p, info, triplets, v0; a struct_size mismatch; a bad memspace or which; rtol or atol
 *   negative or NaN; maxcycles < 1; with vectors: null U or V, ldu < max(m, 1), ldv < max(n, 1), U or V overlapping v0 or each
 *   other; a stream that is being captured.
 *   Run to run.  One product per step is a transposed one: sigma, U, V, cycles and the residuals are bit-identical only where
 *   BOTH products of the handle are -- a handle created with transpose_image = 1 on a conflict-free operator, or a gather /
 *   coloured one (see bsm_lsqr above); elsewhere the last bits may differ and a cycle count may move by one.
 * NOT in it: one-sided reorthogonalisation; harmonic / refined Ritz values or shift-invert for interior and tiny values (the
 *   smallest values converge as the extreme Ritz values of the bidiagonalisation do); a block method; multi-device and own-range
 *   handles; graph capture. */
typedef enum { BSM_SVDS_LM = 0, BSM_SVDS_SM = 1 } bsm_svds_which;
typedef struct {
    int32_t struct_size; /* = sizeof(bsm_svds_params) */
    int32_t which;       /* bsm_svds_which */
    double rtol, atol;   /* estimate <= max(rtol anorm, atol) */
    int32_t maxcycles;
    int32_t vectors;     /* 0: values and estimates only */
} bsm_svds_params;
typedef struct {
    int32_t status, nconv, cycles, reserved;
    int64_t a_products;
    double anorm;
    int64_t workspace_bytes;
    uint64_t workspace; /* device address of the allocation */
} bsm_svds_info;
typedef struct {
    double value, estimate, residual_av, residual_ahu;
} bsm_svds_triplet;
BSM_LAYOUT_ASSERT(sizeof(bsm_svds_params) == 32 && offsetof(bsm_svds_params, rtol) == 8 && offsetof(bsm_svds_params, maxcycles) == 24,
                  "bsm_svds_params layout");
BSM_LAYOUT_ASSERT(sizeof(bsm_svds_info) == 48 && offsetof(bsm_svds_info, a_products) == 16 && sizeof(bsm_svds_triplet) == 32,
                  "bsm_svds_info layout");
struct bsm_svds_s;
int bsm_svds_create(bsm_matrix_t A, int opA, int vdtype, int32_t nsv, int32_t ncv, struct bsm_svds_s **out);
int bsm_svds_solve(struct bsm_svds_s *S, const void *v0 /* min(m, n) */, void *U /* may be NULL with vectors = 0 */, int64_t ldu,
                   void *V /* may be NULL with vectors = 0 */, int64_t ldv, const bsm_svds_params *p, bsm_svds_info *info,
                   bsm_svds_triplet *triplets /* nsv */, int memspace, void *stream);
int bsm_svds_destroy(struct bsm_svds_s *S);

/* bsm_block_gram, bsm_block_combine: the two tall-skinny products of a caller's BLOCK method, beside bsm_krylov_orth (one w per
 * call) and bsm_krylov_combine (a REAL S).  Both only enqueue on `stream`, synchronise nothing and may be graph-captured.
 *
 * bsm_block_gram:  G = U^H W.  U: n x p, 1 <= p <= 48; W: n x q, 1 <= q <= 96; column-major device matrices of dtype (BSM_F32 ..
 * BSM_C128), ldu, ldw >= max(n, 1), ANY element alignment; U is conjugated for complex types; W may alias or contain U.
 * G: p x q, column-major with ldg >= p, in device memory, of the WIDE type (double for real types, complex double for complex
 * ones).  work: bsm_block_gram_work(dtype, n, p, q) bytes of device memory, 16-byte aligned.  Two launches.  Launch 1:
 * bsm_block_gram_grid(dtype, n) workgroups (one per 8192 bytes of a column, at most 256, at least 1), each owns one row range,
 * stages chunks of its rows through LDS with coalesced loads and feeds v_mfma_{f64,f32}_16x16x4 with the rows as the K
 * dimension, 16 columns of U by 16 of W per tile -- complex types as four real products of split real and imaginary parts --
 * and leaves ONE partial p x q matrix in the precision of dtype (a chunk of rows is one chain of MFMAs in that precision; the
 * chunks' sums are added in double in registers and rounded once).  Launch 2 adds the partials in a fixed order in double.  No
 * floating-point atomic, nobody waits: the result is fixed to the bit run to run.  U and W are each read once from memory
 * (columns of U that W contains are read twice).
 * Refused (BSM_ERR_INVALID): a dtype that is no vector type; n < 0; p or q out of range; ldu or ldw < max(n, 1); ldg < p; a null
 * G or work (U, W with n > 0); a work that is not 16-byte aligned; G or work overlapping U, W or each other.  n == 0 is legal:
 * G = 0.
 *
 * bsm_block_combine:  Out[:, c] = sum_{j < p} V[:, j] C[j, c] for c < q, with C of dtype ITSELF -- complex for complex types --,
 * p x q column-major in device memory, ldc >= p.  1 <= p <= 48, 0 <= q <= p.  V: n x p, Out: n x q, ldv, ldo >= max(n, 1), any
 * element alignment.  Out == V with ldo == ldv works IN PLACE on columns 0 .. q - 1 (a tile of rows goes through LDS, all reads
 * of a tile in front of the barrier).  The sum runs over j ascending with fused multiply-adds -- a complex term as
 * re = fma(vr, cr, re), re = fma(-vi, ci, re), im = fma(vr, ci, im), im = fma(vi, cr, im), 2 p fmas per part --: the result is
 * fixed to the bit and independent of the launch geometry.  Real types run the kernel of bsm_krylov_combine.
 * bsm_block_combine_tile(dtype, p): the rows (elements) of the tile: bsm_krylov_combine_tile for real types,
 * min(512, floor(131072 / (p * sizeof(element)) / 64) * 64) for complex ones.
 * Refused (BSM_ERR_INVALID): those of bsm_krylov_combine without the carry: a dtype that is no vector type; n < 0; p outside
 * 1 .. 48; q outside 0 .. p; ldv or ldo < max(n, 1); ldc < p; a null pointer that is needed (C with q > 0; V, Out with n > 0); Out
 * overlapping V other than Out == V with ldo == ldv; C overlapping Out. */
int64_t bsm_block_gram_grid(int dtype, int64_t n);
int64_t bsm_block_gram_work(int dtype, int64_t n, int64_t p, int64_t q);
int bsm_block_gram(int dtype, int64_t n, int64_t p, const void *U, int64_t ldu, int64_t q, const void *W, int64_t ldw, void *G,
                   int64_t ldg, void *work, void *stream);
int64_t bsm_block_combine_tile(int dtype, int64_t p);
int bsm_block_combine(int dtype, int64_t n, int64_t p, int64_t q, const void *V, int64_t ldv, const void *C, int64_t ldc, void *Out,
                      int64_t ldo, void *stream);

/* bsm_lobpcg_*: the `nev` smallest (BSM_EIGSH_SA) or largest (BSM_EIGSH_LA) EIGENPAIRS of op(A), A asserted real symmetric /
 * complex Hermitian by the caller, by LOBPCG (Knyazev) on a block of `block` vectors with an optional preconditioner M, which
 * the caller asserts to be Hermitian positive definite, ~ inv(A) on the wanted end.  A block method sees every copy of a
 * multiple eigenvalue, streams A once per iteration for the whole block (bsm_mul_multi), and takes the preconditioners the
 * linear solvers take.  (No counterpart in the reference.)
 *   Write k = block, p = 3 k, eps that of vdtype, tau = 64 p eps.  The workspace holds Z = [S | AS], S = [X | P | W],
 *   AS = [AX | AP | AW], 6 k columns (and T, k columns, with M).
 *   Start.  Z = 0; X = X0; AX = op(A) X (one bsm_mul_multi); the Gram matrix below, one copy, one synchronisation; the
 *   Rayleigh-Ritz step on X alone; the combination below.
 *   Iteration i (X_i the block it starts with):
 *     1. R[:, c] = AX[:, c] - theta_c X[:, c] into W (with M: into T) on a (row ranges, k) grid; one partial of ||R_c||^2 per
 *        workgroup and column, added by one wave per column in a fixed order: the CARRIED residual norms of X_i.
 *     2. with M:  W = op(M) T (bsm_mul_multi).      3. AW = op(A) W (bsm_mul_multi), straight into the workspace.
 *     4. ONE bsm_block_gram with U = S (p columns) and W = Z:  [G_B | G_A] = [S^H S | S^H AS].
 *     5. ONE device-to-host copy (G, the k norms) and one synchronisation.
 *     6. anorm = the largest |Ritz value| of any projected problem so far.  Column c is LIVE while ||R_c|| > max(rtol anorm,
 *        atol).  The block has CONVERGED when the first nev columns (in the order of `which`) are not live.
 *     7. Rayleigh-Ritz on the host, in double / complex double (csrc/bsm_lobpcg.h), deterministic.  Basis columns in use: X,
 *        the W columns of live columns, the P columns of the columns whose W the previous iteration used (none in the first):
 *        soft locking on the host only, the device always works on 3 k columns.  G_A, G_B are symmetrised and scaled by
 *        d_i = 1 / sqrt(G_B[i, i]); the scaled G_B = Q Lambda Q^H by a cyclic Hermitian Jacobi method with a fixed sweep order;
 *        directions with lambda <= tau lambda_max are dropped (counted in info.drops); L = Q_kept Lambda^{-1/2};
 *        L^H G_A L = Z Mu Z^H by the same method; the k extreme Ritz values of `which` are theta, C = diag(d) L Z_sel (p x k,
 *        zero rows for columns not in use), C_P = C with its X rows zeroed.
 *     8. CC = [C | C_P] and theta are uploaded.     9. [X | P] = S CC and [AX | AP] = AS CC by two in-place bsm_block_combine.
 *   Every iteration runs all nine steps.  The one that found the block converged (or was number maxiter) is followed by step 1
 *   alone and a copy of the k norms: the carried norms of the X it left.  If they confirm the convergence the solve ends with
 *   status 0 -- status 0 therefore means that the carried residuals of the RETURNED pairs are within the tolerance --,
 *   otherwise (and below maxiter) it goes on with step 2.  Hence ONE synchronisation per iteration, one more per confirmation,
 *   a_products = iterations + 2 multi-column products (start, one per iteration, the true-residual pass), m_products =
 *   iterations, and a history of iterations + 1 rows.
 *   End.  X[:, :nev], every column scaled to norm one, goes to the caller's matrix; then the TRUE residuals
 *   ||op(A) x_i - theta_i x_i|| as in bsm_eigsh_solve.  AX is never recomputed: the true residual reports what the drift left.
 * create: vdtype must be A's own vector type, as for bsm_eigsh_create; 1 <= nev <= block <= BSM_CG_MAX_RHS = 16, 3 block <= n.
 *   M (may be NULL) with opM: paired with vdtype as for bsm_cg_create (its own vector type, or real and unmixed of the same
 *   precision under a complex vdtype); a composed handle (bsm_poly_create) is accepted as M, not as A.  ONE device allocation,
 *   leading dimensions rounded up to whole 16-byte groups: Z, T, the partials of the Gram, G (p x 2 p wide) with the norms, CC,
 *   theta, the partials of the residual pass.  Refused: those of bsm_eigsh_create for A, those of bsm_cg_create for M (another
 *   order, a bad pairing, multi-device, analysis-only, own-range, another device), nev or block out of range (BSM_ERR_INVALID).
 *   Both handles must outlive the solver.
 * solve: X0 (n x block, ldx0 >= max(n, 1)) and X (n x nev, ldx >= max(n, 1)), column-major, any element alignment;
 *   BSM_MEM_HOST operands are staged through device buffers the solver keeps.  pairs: nev entries of bsm_eigsh_pair in the order
 *   of `which`: value, estimate = the carried residual norm, residual = the true one.  history (may be NULL with capacity 0):
 *   row r < history_capacity takes the nev carried norms of X_r, history[r * nev + c].  Synchronous.
 *   info.status:  0 converged;  1 maxiter reached (X and pairs hold the pairs as they stand; nconv counts those within the
 *   tolerance);  2 a norm, a Gram entry or a Ritz value is not finite, or Jacobi hit its sweep cap (X is not written, pairs are
 *   NaN);  3 fewer than `block` directions kept: a rank-deficient or zero X0 at the start, or a G_B[i, i] that is not positive
 *   (X is not written, pairs are NaN).
 *   Refused (BSM_ERR_INVALID): null S, p, info, pairs, X0, X; a struct_size mismatch; a bad memspace; a `which` other than
 *   BSM_EIGSH_SA / _LA; rtol or atol negative or NaN; maxiter < 1; ldx or ldx0 < max(n, 1); X overlapping X0; a negative
 *   history_capacity, or a positive one without an array; a stream that is being captured.
 *   Run to run, the values, X, the counts and the history are bit-identical wherever the products of the handles are.
 * Not in it: the generalised problem, hard locking, a periodic recompute of AX, interior eigenvalues, block > 16, multi-device or
 *   own-range handles, graph capture of a solve, the small eigenproblem on the device. */
typedef struct {
    int32_t struct_size; /* = sizeof(bsm_lobpcg_params) */
    int32_t which;       /* BSM_EIGSH_SA or BSM_EIGSH_LA */
    double rtol, atol;   /* carried residual <= max(rtol anorm, atol) */
    int32_t maxiter;
    int32_t reserved;
} bsm_lobpcg_params;
typedef struct {
    int32_t status, nconv, iterations, drops;
    int64_t a_products, m_products;
    double anorm;
    int64_t workspace_bytes;
} bsm_lobpcg_info;
BSM_LAYOUT_ASSERT(sizeof(bsm_lobpcg_params) == 32 && offsetof(bsm_lobpcg_params, rtol) == 8 && offsetof(bsm_lobpcg_params, maxiter) == 24,
                  "bsm_lobpcg_params layout");
BSM_LAYOUT_ASSERT(sizeof(bsm_lobpcg_info) == 48 && offsetof(bsm_lobpcg_info, a_products) == 16 && offsetof(bsm_lobpcg_info, anorm) == 32,
                  "bsm_lobpcg_info layout");
struct bsm_lobpcg_s;
int bsm_lobpcg_create(bsm_matrix_t A, int opA, bsm_matrix_t M /* may be NULL */, int opM, int vdtype, int32_t nev, int32_t block,
                      struct bsm_lobpcg_s **out);
int bsm_lobpcg_solve(struct bsm_lobpcg_s *S, const void *X0, int64_t ldx0, void *X, int64_t ldx, const bsm_lobpcg_params *p,
                     bsm_lobpcg_info *info, bsm_eigsh_pair *pairs /* nev */, double *history, int64_t history_capacity, int memspace,
                     void *stream);
int bsm_lobpcg_destroy(struct bsm_lobpcg_s *S);

/* Statistics of a handle. */
typedef struct {
    int64_t nnz;            /* SparseArrays.nnz as the reference defines it (off-diagonal
                               blocks of a SymmetricBlockMatrix count twice,
                               src/symmetricblockmatrix.jl:367-384) */
    int64_t stored_entries; /* matrix entries held on the device (each stored once) */
    int64_t alg_bytes;      /* algorithmic bytes of one mul with beta = 0; mixed-precision handles count
                               the stored type's bytes for the values, the vector type's for x and y */
    int64_t device_bytes;   /* bytes of the packed device image (values in the stored type + metadata) */
    int64_t npanels, ntasks, nworkgroups;
    int64_t exclusive;      /* 1: forward product needs no atomics and no pre-scale pass */
    /* SymmetricBlockMatrix, op N: y contributions the fused launch produces (forward rows + transposed
     * columns of every wave), how many of them are added up in a workgroup's LDS window first, and how
     * many entries those windows then add to y -- global atomics per product =
     * win_emissions - win_inside + win_flushed */
    int64_t win_emissions, win_inside, win_flushed;
    int64_t reserved[5];
} bsm_stats_t;
BSM_LAYOUT_ASSERT(sizeof(bsm_stats_t) == 128 && offsetof(bsm_stats_t, win_emissions) == 64, "bsm_stats_t layout");
int bsm_stats(bsm_matrix_t A, bsm_stats_t *out);

/* Debug / test hook: copies one array of the packed device image (host copy) out.
 * which: 0 values (bytes), 1 rows (int32), 2 cols (int32), 3 waves (64-byte records;
 * layout in blocksparsematrices.jl_amd/csrc/bsm_layout.h); gather handles also 4 / 5 = row
 * pointers (int64) / workspace slots (int32) of the op-N inverted index and 6 / 7 for op T;
 * 8 = the coarser wave records bsm_mul_multi walks (empty when the records of 3 serve both).
 * Add 16 to `which` for the arrays of the transposed image (bsm_options.transpose_image).
 * Only available on analysis-only handles (BSM_DEVICE_NONE), which keep the host copy.
 * Call with out == NULL to obtain the size in bytes. */
int bsm_get_image(bsm_matrix_t A, int which, void *out, int64_t *nbytes);

/* color(conflictgraph(ColorInfo(lists)); algorithm).colors -- reference src/coloring.jl:15-61 +
 * GraphsColoring.jl (compat 0.2.0, NOT in the reference tree; the reference's default algorithm is its
 * WorkstreamDSATUR, src/BlockSparseMatrices.jl:10).  Two lists conflict iff they share an index.
 * algorithm: BSM_COLOR_WORKSTREAM_DSATUR -- the published WorkStream colouring (Turcksin, Kronbichler,
 * Bangerth, ACM TOMS 43, 2016, section 3.2: zones = breadth-first layers of the conflict graph, DSATUR
 * inside every zone, classes of the even and of the odd zones gathered largest-to-smallest) -- or
 * BSM_COLOR_DSATUR (plain DSATUR on the whole graph).
 * CONTRACT: the classes returned here (and by BSM_BK_COLORS / _TRANSPOSECOLORS / _DIAGONALCOLORS) are
 * VALID -- they partition 1..nlists and no two lists of a class share an index, which is all the
 * reference's mul! relies on (src/blockmatrix.jl:233-245) -- and DETERMINISTIC (every tie-break is
 * specified in oracle/bsm_oracle.c and compared bit-exactly in tests/test_host_logic.py).  They follow
 * the published algorithm, but are NOT claimed to be identical to GraphsColoring's output: its source
 * and version are not available here and no reference test inspects colour classes.  The serial
 * scheduler's single class [1:nblocks] (src/blockmatrix.jl:91-92) IS reproduced exactly.  The GPU
 * product does not depend on the classes (BSM_ACC_COLORED colours row GROUPS itself, with DSATUR).
 * lists[b] has lens[b] 1-based entries; color_out[b] receives the 0-based colour of list b;
 * *ncolors the number of colours. */
int bsm_color(int64_t nlists, const int64_t *const *lists, const int64_t *lens, int algorithm,
              int64_t *color_out, int64_t *ncolors);

int bsm_destroy(bsm_matrix_t A);

/* thread-local message of the last failing call in this thread ("" if none) */
const char *bsm_last_error(void);

/* library / build identification, e.g. "bsmrocm 0.3 gfx950 build 1a2b3c4d5e6f": the build id is a hash of the
 * kernel and schedule sources, so that a measurement can be tied to what actually ran */
const char *bsm_version(void);

#ifdef __cplusplus
}
#endif
#endif /* BSM_ROCM_H */
