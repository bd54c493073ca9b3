// bsm_internal.h -- what bsm_capi.cpp (the C ABI; single-device handles), bsm_dist.cpp / bsm_fanout.cpp (handles spread
// over the devices of a bsm_ctx_t: building them / issuing their products; their own types are in bsm_dist.h),
// bsm_operator.cpp (the packed operator on one device that both are made of) and the units that hold a feature's own
// entry points (bsm_entries.cpp, bsm_invert.cpp, bsm_krylov.cpp) share.  Not part of the C ABI.
#pragma once
#include <hip/hip_runtime_api.h>

#include <memory>
#include <mutex>
#include <new>
#include <string>
#include <vector>

#include "../../include/bsm_rocm.h"
#include "bsm_analysis.h"
#include "bsm_kernels.h"
#include "bsm_refill.h"
#include "bsm_types.h"

struct bsm_ctx_s {
    std::vector<int> devices;  // HIP ordinals; the same ordinal may appear several times (virtual devices)
    // peer access was ENABLED (hipSuccess or hipErrorPeerAccessAlreadyEnabled) for every ordered pair of distinct
    // devices: the condition of the fused fan-out kernels, which dereference peer pointers directly
    bool peer_ok = false;
};

namespace bsm {
struct DistState;  // bsm_dist.h
struct PolyState;  // bsm_poly.h

// bsm_update_blocks on one device: the device copy of the refill plans of its images (uploaded at the first update,
// kept until the handle is destroyed) and the per-call table of source blocks (RefillSrc by input block id) with the
// item list of a subset update.  The table is written from a pinned host mirror, and only when it differs from what
// the last update wrote: an update that names the same arrays as the previous one enqueues nothing but the kernels.
struct RefillDevice {
    void *d_chunks = nullptr, *d_colpos = nullptr, *d_segs = nullptr, *d_items_all = nullptr, *d_items_id = nullptr;
    bool ready = false;
};
// what *_create analysed, kept for bsm_update_blocks: the block list (index lists copied, `data` = a token naming the
// input block id instead of an address) and the options of the image(s)
struct UpdateInputs {
    int mtype = 0, dtype = 0;
    int64_t nrows = 0, ncols = 0;
    int64_t nids = 0;          // blocks of the whole *_create call (a part of a multi-device handle holds some)
    AnalysisOptions ao, ao_t;  // forward image, transposed image
    std::vector<BlockIn> in;
    std::vector<std::vector<int64_t>> lists;
};
struct UpdateState {
    RefillPlan plan[2];   // host plans (built at the first update)
    RefillDevice img[2];  // forward image, transposed image
    RefillSrc *d_src = nullptr, *h_src = nullptr;
    int32_t *d_list = nullptr, *h_list = nullptr;
    int64_t nids = 0, list_cap = 0;
    hipEvent_t ev_done = nullptr;  // end of the last update's kernels: the table may be rewritten from then on
    bool pending = false;
    bool table_valid = false;  // d_src / d_list hold h_src / h_list as of the last update (false after a host update:
                               // its entries named staging windows that are gone)
    int64_t list_len = -1;     // length of that list (-1: full update, no list)
    // graph-captured updates: the graph carries its own copy of the table -- a captured H2D copy from a pinned snapshot
    // into a device table only captured updates use.  Written once, by the first captured update; eager updates never
    // touch either, so a replay reads what its capture saw.
    RefillSrc *d_cap_src = nullptr, *h_cap_src = nullptr;
    int32_t *d_cap_list = nullptr, *h_cap_list = nullptr;
    bool cap_valid = false;
    int64_t cap_list_len = -1;
};

// A packed operator on one device: what a single-device handle is, and what every part of a multi-device handle is
// (bsm_operator.cpp).  Built once, refilled by bsm_update_blocks, released with its device current.
struct LocalOperator {
    // HIP ordinal of the images, set before build(); BSM_DEVICE_NONE: analysis only (the packed values stay in
    // Analysis::values).  A part that holds no block keeps its ordinal and is never built.
    int device = BSM_DEVICE_NONE;
    Analysis an;
    DeviceImage img;
    // optional second ordering (bsm_options.transpose_image): the transposed operator as its own forward image
    bool has_t = false;
    Analysis an_t;
    DeviceImage img_t;
    // bsm_update_blocks: the kept block list and the refill state on `device`
    std::unique_ptr<UpdateInputs> upd_in;
    UpdateState upd;
    // work arrays of the interleaved multi-RHS pass (bsm_kernels.h: ILWork), allocated at the first product that takes it
    ILWork il;

    // Analysis, packing and upload of `in` (the block list in its final order; ids[b]: input block id of in[b], of nids
    // in the whole *_create call) on `device`, which must be current.  Host blocks are streamed to the device while they
    // are packed, device blocks (o.blocks_memspace) are packed there by a kernel.  colors: compute the reference
    // colourings; prefix: put in front of an analysis error ("device part 3: ").  BSM_OK, or the code of the error set;
    // whatever a failed build leaves behind goes with release().
    int build(int mtype, int dtype, int64_t nrows, int64_t ncols, const std::vector<BlockIn> &in, const std::vector<int64_t> &ids,
              int64_t nids, const bsm_options &o, bool colors, const std::string &prefix);
    // Frees both images, the refill state and the work arrays; `device` must be current.
    void release();
    // Replaces the values of the blocks with the 0-based input ids ids[k] by blocks[k] / ld[k] (full: every id 0..nids-1
    // in order).  bm / bn: stored shape of every input block.
    // BSM_MEM_DEVICE: enqueued on `st`; BSM_MEM_HOST: staged, synchronous; analysis-only operators: host blocks only,
    // Analysis::values is rewritten.
    int refill(int64_t nupd, const int64_t *ids, bool full, const void *const *blocks, const int64_t *ld, int memspace, hipStream_t st,
               const std::vector<int64_t> &bm, const std::vector<int64_t> &bn);
    // builds upd.plan[] from the kept inputs at the first update (refill() calls it; dist_update reads plan[0] first)
    int ensure_plans();
};
}

namespace bsm {
// a resource of the handle that admits one product in flight (bsm_capi.cpp: Claim)
struct ClaimState {
    std::mutex mu;
    hipStream_t stream = nullptr;  // stream of the last product that held the claim
    bool pending = false;          // ... which may still be running
};
}  // namespace bsm

// The operator of a single-device handle is the handle's base.  Multi-device handles: `an` holds the bookkeeping /
// statistics of the WHOLE operator, there is no image (device == BSM_DEVICE_NONE) and every part is an operator of
// its own (bsm_dist.h: Part).
struct bsm_matrix_s : bsm::LocalOperator {
    bool on_device = false;
    // one product in flight per handle on the gather workspace of the images (one-column products) and on the work
    // arrays of the interleaved multi-RHS pass (bsm_kernels.h: ILWork, allocated at the first product that takes it):
    // bsm_capi.cpp: Claim
    bsm::ClaimState ws_claim, il_claim;
    // device staging buffers of the BSM_MEM_HOST path, kept between calls (grow-only); a second
    // concurrent host call on the same handle falls back to temporary buffers
    std::mutex host_mu;
    void *stage_x = nullptr, *stage_y = nullptr;
    size_t stage_x_bytes = 0, stage_y_bytes = 0;
    // handle spread over the devices of a context (bsm_options.ctx)
    std::unique_ptr<bsm::DistState> dist;
    // composed handle (bsm_poly_create): a polynomial in other handles; it has no image, its product is poly_mul
    std::unique_ptr<bsm::PolyState> poly;
    // bsm_update_blocks: stored shape of every input block (constructor order); one update at a time
    std::vector<int64_t> blk_m, blk_n;
    std::mutex upd_mu;
    bsm_matrix_s();
    ~bsm_matrix_s();
};

namespace bsm {

int fail(int code, const std::string &msg);
int hip_fail(hipError_t e, const char *what);
int build_error(const std::string &err);  // analysis error -> BSM_ERR_INVALID, value sink error -> BSM_ERR_DEVICE

struct DeviceGuard {
    int prev = -1;
    bool active = false;
    hipError_t enter(int dev);
    ~DeviceGuard();
};
// a scratch allocation on the current device, freed with its scope
struct DevBuf {
    void *p = nullptr;
    ~DevBuf() {
        if (p) (void)hipFree(p);
    }
    hipError_t alloc(size_t bytes) { return hipMalloc(&p, bytes ? bytes : 16); }
};

// the body of an extern "C" entry point that allocates on the host: nothing is thrown across the ABI
#define BSM_GUARDED(...)                                         \
    try {                                                        \
        __VA_ARGS__                                              \
    } catch (const std::bad_alloc &) {                           \
        return fail(BSM_ERR_ALLOC, "out of host memory");        \
    } catch (const std::exception &e) {                          \
        return fail(BSM_ERR_INVALID, e.what());                  \
    }

AnalysisOptions to_aopt(const bsm_options &o, ValueSink *sink);
// whether `st` is being captured into a graph (a failed query counts as "no")
bool capturing(hipStream_t st);
// the work arrays of the interleaved multi-RHS pass hold `need` vector entries (Xr, W: 128 bytes per entry each); a
// regrow frees the old arrays, so no product may still use them.  false: no memory (the arrays are left empty)
bool il_reserve(ILWork &il, long long need);

// ---- bsm_fanout.cpp: the products of a multi-device handle ---------------------------------------
int dist_mul_multi(bsm_matrix_s *A, int op, long long nrhs, const void *X, long long ldx, void *Y, long long ldy,
                   const void *alpha, const void *beta, int beta_strong_zero, int memspace, hipStream_t stream);
int dist_mul_parts(bsm_matrix_s *A, int op, const void *const *x_parts, void *const *y_parts, const void *alpha,
                   const void *beta, int beta_strong_zero, void *const *streams);

// ---- bsm_poly.cpp: composed handles (bsm_poly_create) ------------------------------------------
// the product behind the four product entry points (arguments as mul_entry of bsm_capi.cpp takes them)
int poly_mul(bsm_matrix_s *M, int op, bool cplx, bool multi, int64_t nrhs, const void *X, int64_t ldx, void *Y, int64_t ldy,
             const void *alpha, const void *beta, int beta_strong_zero, int memspace, hipStream_t stream);
// BSM_OK, or the BSM_ERR_UNSUPPORTED of entry point `what`, which reads or writes entries, for a composed handle
int poly_refusal(const bsm_matrix_s *A, const char *what);
// frees the workspace of a composed handle (no-op on any other); its device must be current
void poly_release(bsm_matrix_s *M);

// ---- bsm_dist.cpp -------------------------------------------------------------------------------
// Row partition of `in` (already in its final order) over the context's devices; fills A->dist.
// A->an must already hold the whole operator's bookkeeping (meta-only analysis).
// ids[b]: input block id of in[b] (bsm_update_blocks)
int dist_create(bsm_matrix_s *A, bsm_ctx_s *ctx, int mtype, int dtype, int64_t nrows, int64_t ncols,
                const std::vector<BlockIn> &in, const std::vector<int64_t> &ids, const bsm_options &o);
void dist_destroy(bsm_matrix_s *A);
int dist_part_info(bsm_matrix_s *A, int32_t part, bsm_part_info_t *out);
// bsm_update_blocks of a multi-device handle (arguments checked by the caller; ids 0-based)
int dist_update(bsm_matrix_s *A, int64_t nupd, const int64_t *ids, bool full, const void *const *blocks, const int64_t *ld,
                int memspace, hipStream_t stream);
int64_t dist_device_bytes(const bsm_matrix_s *A);
// (analysis, image) of every part that holds blocks
using ImageRef = std::pair<const Analysis *, const DeviceImage *>;
std::vector<ImageRef> dist_images(bsm_matrix_s *A);

// smallest row index of every block (its partition key) and its weight (stored entries)
void block_row_keys(const std::vector<BlockIn> &in, std::vector<int64_t> &key, std::vector<int64_t> &weight);
// see bsm_partition_rows in include/bsm_rocm.h
void partition_rows(int64_t nrows, const std::vector<int64_t> &key, const std::vector<int64_t> &weight,
                    int nparts, std::vector<int32_t> &part_of_block, std::vector<int64_t> &own_lo,
                    std::vector<int64_t> &own_hi);

}  // namespace bsm
