// bsm_invert.cpp -- bsm_invert_blocks (include/bsm_rocm.h): batched in-place inverse of dense blocks.  Host blocks go
// through the elimination of bsm_invert.h, device blocks through invert_kernel (bsm_invert.hip), which runs the same one.
#include <hip/hip_runtime_api.h>

#include <algorithm>
#include <string>
#include <vector>

#include "bsm_internal.h"
#include "bsm_invert.h"

using namespace bsm;

namespace {
// the device leg: the non-empty blocks sorted by descending order (the large ones start first), cut into launches of
// one regime whose blocks need more than half the LDS of the launch's first -- a 16 x 16 block does not reserve the
// LDS of the 128 x 128 one that came in the same call
int invert_device(int dtype, int64_t nblocks, void *const *blocks, const int64_t *n, const int64_t *ld, int64_t *info,
                  hipStream_t stream) {
    const int es = elem_bytes(dtype);
    std::vector<InvertBlock> table;
    for (int64_t b = 0; b < nblocks; b++)
        if (n[b] > 0) table.push_back(InvertBlock{(uint64_t)(uintptr_t)blocks[b], (long long)ld[b], (int)n[b], (int)table.size()});
    if (table.empty()) return BSM_OK;
    std::stable_sort(table.begin(), table.end(), [](const InvertBlock &a, const InvertBlock &b) { return a.n > b.n; });
    int dev = 0;
    hipError_t e = hipGetDevice(&dev);
    if (e == hipSuccess && stream && hipStreamGetDevice(stream, &dev) != hipSuccess) {
        (void)hipGetLastError();
        e = hipGetDevice(&dev);
    }
    if (e != hipSuccess) return hip_fail(e, "hipGetDevice");
    DeviceGuard g;
    e = g.enter(dev);
    if (e != hipSuccess) return hip_fail(e, "hipSetDevice");
    DevBuf db;  // the table, behind it one int32 of info per table entry
    const size_t tb = (table.size() * sizeof(InvertBlock) + 15) / 16 * 16;
    e = db.alloc(tb + table.size() * 4);
    if (e == hipSuccess) e = hipMemcpyAsync(db.p, table.data(), table.size() * sizeof(InvertBlock), hipMemcpyHostToDevice, stream);
    int *d_info = (int *)((char *)db.p + tb);
    auto resident = [&](const InvertBlock &t) { return (long long)t.n * t.n * es <= (long long)BSM_INVERT_LDS_BYTES; };
    for (size_t i = 0; i < table.size() && e == hipSuccess;) {
        const bool res = resident(table[i]);
        const int head = invert_lds(table[i].n, es, res).total;
        size_t j = i + 1;
        while (j < table.size() && resident(table[j]) == res && 2 * invert_lds(table[j].n, es, res).total > head) j++;
        e = launch_invert(dtype, (const InvertBlock *)db.p + i, (long long)(j - i), table[i].n, res, d_info, stream);
        i = j;
    }
    std::vector<int> hinfo(table.size(), 0);
    if (e == hipSuccess) e = hipMemcpyAsync(hinfo.data(), d_info, table.size() * 4, hipMemcpyDeviceToHost, stream);
    if (e == hipSuccess) e = hipStreamSynchronize(stream);
    if (e != hipSuccess) return hip_fail(e, "invert");
    if (info) {
        int64_t k = 0;  // table ids count the non-empty blocks in the caller's order
        for (int64_t b = 0; b < nblocks; b++)
            if (n[b] > 0) info[b] = hinfo[(size_t)k++];
    }
    return BSM_OK;
}
}  // namespace

extern "C" int bsm_invert_blocks(int dtype, int64_t nblocks, void *const *blocks, const int64_t *n, const int64_t *ld,
                                 int64_t *info, int memspace, void *stream) {
    BSM_GUARDED(
        const std::string why = vec_type_refusal("bsm_invert_blocks", dtype);
        if (!why.empty()) return fail(BSM_ERR_INVALID, why);
        if (memspace != BSM_MEM_HOST && memspace != BSM_MEM_DEVICE) return fail(BSM_ERR_INVALID, "bad memspace");
        if (nblocks < 0 || nblocks > INT32_MAX) return fail(BSM_ERR_INVALID, "bad number of blocks");
        if (nblocks > 0 && (!blocks || !n || !ld)) return fail(BSM_ERR_INVALID, "null argument");
        for (int64_t b = 0; b < nblocks; b++) {
            const std::string blk = "block " + std::to_string(b + 1) + ": ";
            if (n[b] < 0) return fail(BSM_ERR_INVALID, blk + "negative size");
            if (ld[b] < std::max<int64_t>(n[b], 1)) return fail(BSM_ERR_INVALID, blk + "ld < max(n, 1)");
            if (n[b] > 0 && !blocks[b]) return fail(BSM_ERR_INVALID, blk + "null block");
        }
        for (int64_t b = 0; b < nblocks; b++)
            if (n[b] > BSM_INVERT_MAX_N)
                return fail(BSM_ERR_UNSUPPORTED, "block " + std::to_string(b + 1) + ": n = " + std::to_string(n[b]) +
                                                     " > 1024 (one workgroup eliminates one block)");
        if (info) std::fill(info, info + nblocks, (int64_t)0);
        if (memspace == BSM_MEM_DEVICE) return invert_device(dtype, nblocks, blocks, n, ld, info, (hipStream_t)stream);
        with_types(dtype, [&](auto r, auto, auto nc) {
            for (int64_t b = 0; b < nblocks; b++) {
                const int rc = invert_block_host<decltype(r), decltype(nc)::value>((decltype(r) *)blocks[b], n[b], ld[b]);
                if (info) info[b] = rc;
            }
        });
        return BSM_OK;)
}
