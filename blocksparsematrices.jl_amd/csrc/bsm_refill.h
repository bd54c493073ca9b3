// bsm_refill.h -- bsm_update_blocks: the replayable value placement of an image and the kernel that replays it.
//
// The placement is what the pack plan of a device-block create (Analysis::pack_plan) records, with the source named by
// input block id (position in the *_create call) instead of an address, so that the same plan refills the image from
// whatever arrays hold the new values.  It is derived at the first update of a handle by re-running the value-blind
// analysis on the block list kept from creation (bsm_operator.cpp: make_refill_plan) and checked against the image.
#pragma once
#include <hip/hip_runtime_api.h>

#include <cstdint>
#include <vector>

namespace bsm {

// one chunk (<= 64 rows of one block): placement as PackChunk
struct RefillChunk {
    uint64_t dst_unit;  // first 16-byte unit of the row group's panel in the value stream
    int32_t id;         // input block id (0-based)
    int32_t ra;         // first row of the chunk inside the block
    int32_t n, woff;    // columns of the block, first merged panel column (identity placement)
    int32_t perm_off;   // >= 0: offset into RefillPlan::colpos (scattered placement)
    int16_t mc;         // rows (<= 64)
    int16_t trans;      // 1: the logical block is the transpose of the stored array
};
static_assert(sizeof(RefillChunk) == 32, "RefillChunk must be 32 bytes");
// a strip range (identity placement) or a column range (scattered) of one chunk; units = mc * (hi - lo)
struct RefillSeg {
    int32_t chunk, lo, hi, units;
};
// what one wave of refill_kernel refills: up to 64 consecutive segments, at most kRefillItemUnits units in all
struct RefillItem {
    int32_t seg_first, seg_count;
};
constexpr int kRefillItemUnits = 1024;  // 16 KB of values per wave

struct RefillPlan {
    std::vector<RefillChunk> chunks;    // sorted by id
    std::vector<int32_t> colpos;        // scattered column placements (empty when no chunk is scattered)
    std::vector<int64_t> cptr;          // nids + 1: chunks[cptr[id] .. cptr[id + 1]) belong to block id
    std::vector<RefillSeg> segs;        // in chunk order
    std::vector<RefillItem> items_all;  // a full refill: items may span block ids
    std::vector<RefillItem> items_id;   // items of ONE block id each: items_id[iptr[id] .. iptr[id + 1])
    std::vector<int64_t> iptr;
    int64_t nids = 0;
    bool built = false;
    size_t host_bytes() const {
        return chunks.size() * sizeof(RefillChunk) + colpos.size() * 4 + (cptr.size() + iptr.size()) * 8 +
               segs.size() * sizeof(RefillSeg) + (items_all.size() + items_id.size()) * sizeof(RefillItem);
    }
};

// per-call source table entry: device address and leading dimension of input block id
struct RefillSrc {
    uint64_t ptr;
    int64_t ld;
};

// Refills the value stream through a plan already in device memory.  A wave per item; items = d_items[d_list[k]]
// for k < nitems (d_list null: d_items[k]).  es = element bytes.  No allocation, no synchronisation.
hipError_t launch_refill(int es, const void *d_chunks, const void *d_colpos, const void *d_segs, const void *d_items,
                         const int32_t *d_list, long long nitems, const RefillSrc *d_src, void *d_values, hipStream_t stream);

}  // namespace bsm
