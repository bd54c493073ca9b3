// bsm_eigh.cpp -- bsm_eigh_blocks and bsm_spectral_blocks (include/bsm_rocm.h): batched Hermitian eigendecomposition of dense
// blocks, and V f(w) V^H from such a decomposition.  Host blocks go through the plain C++ of bsm_eigh.h, device blocks
// through eigh_kernel / spectral_kernel (bsm_eigh.hip), which run the same arithmetic.
#include <hip/hip_runtime_api.h>

#include <algorithm>
#include <cmath>
#include <string>
#include <vector>

#include "bsm_internal.h"
#define BSM_EIGH_LAUNCH
#include "bsm_eigh.h"

using namespace bsm;

namespace {
// the checks both entries share, in the order of bsm_invert_blocks: BSM_OK, or the refusal (nothing has been written)
int check_blocks(const char *fn, int dtype, int64_t nblocks, const void *const *blocks, const int64_t *n, const int64_t *ld, int memspace) {
    const std::string why = vec_type_refusal(fn, dtype);
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
    return BSM_OK;
}
int check_order(int64_t nblocks, const int64_t *n) {
    for (int64_t b = 0; b < nblocks; b++)
        if (n[b] > BSM_EIGH_MAX_N)
            return fail(BSM_ERR_UNSUPPORTED, "block " + std::to_string(b + 1) + ": n = " + std::to_string(n[b]) +
                                                 " > 512 (one workgroup decomposes one block)");
    return BSM_OK;
}

// the device leg of both entries: the records sorted by descending order (the large ones start first), uploaded, cut into
// launches of one regime whose blocks need more than half the LDS of the launch's first, `words` int32 of info per record
// read back into hinfo.  scratch: the records outside the LDS regime get n x n elements of one allocation as their aux.
template <typename Regime, typename Lds, typename Launch>
int run_device(std::vector<EighBlock> &table, int es, int words, hipStream_t stream, Regime regime, Lds lds, Launch launch,
               bool scratch, std::vector<int> &hinfo) {
    if (table.empty()) return BSM_OK;
    std::stable_sort(table.begin(), table.end(), [](const EighBlock &a, const EighBlock &b) { return a.n > b.n; });
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
    DevBuf db, sb;  // the table, behind it the info words; the scratch of the larger blocks
    if (scratch) {
        size_t elems = 0;
        for (const EighBlock &t : table)
            if (!regime(t)) elems += (size_t)t.n * t.n;
        if (elems) {
            e = sb.alloc(elems * es);
            if (e != hipSuccess) return hip_fail(e, "eigh scratch");
            size_t at = 0;
            for (EighBlock &t : table)
                if (!regime(t)) t.aux = (uint64_t)(uintptr_t)sb.p + at * es, at += (size_t)t.n * t.n;
        }
    }
    const size_t tb = (table.size() * sizeof(EighBlock) + 15) / 16 * 16;
    e = db.alloc(tb + table.size() * 4 * words);
    if (e == hipSuccess) e = hipMemcpyAsync(db.p, table.data(), table.size() * sizeof(EighBlock), hipMemcpyHostToDevice, stream);
    int *d_info = (int *)((char *)db.p + tb);
    for (size_t i = 0; i < table.size() && e == hipSuccess;) {
        const bool res = regime(table[i]);
        const int head = lds(table[i].n, res);
        size_t j = i + 1;
        while (j < table.size() && regime(table[j]) == res && 2 * lds(table[j].n, res) > head) j++;
        e = launch((const EighBlock *)db.p + i, (long long)(j - i), table[i].n, res, d_info);
        i = j;
    }
    hinfo.assign(table.size() * words, 0);
    if (e == hipSuccess) e = hipMemcpyAsync(hinfo.data(), d_info, hinfo.size() * 4, hipMemcpyDeviceToHost, stream);
    if (e == hipSuccess) e = hipStreamSynchronize(stream);
    if (e != hipSuccess) return hip_fail(e, "eigh");
    return BSM_OK;
}
}  // namespace

extern "C" int bsm_eigh_blocks(int dtype, int64_t nblocks, void *const *blocks, const int64_t *n, const int64_t *ld, void *const *w,
                               int32_t vectors, int64_t *info, int32_t *sweeps, int memspace, void *stream) {
    BSM_GUARDED(
        int rc = check_blocks("bsm_eigh_blocks", dtype, nblocks, blocks, n, ld, memspace);
        if (rc != BSM_OK) return rc;
        if (nblocks > 0 && !w) return fail(BSM_ERR_INVALID, "null argument");
        for (int64_t b = 0; b < nblocks; b++)
            if (n[b] > 0 && !w[b]) return fail(BSM_ERR_INVALID, "block " + std::to_string(b + 1) + ": null w");
        rc = check_order(nblocks, n);
        if (rc != BSM_OK) return rc;
        if (info) std::fill(info, info + nblocks, (int64_t)0);
        if (sweeps) std::fill(sweeps, sweeps + nblocks, (int32_t)0);
        if (memspace == BSM_MEM_HOST) {
            with_types(dtype, [&](auto r, auto, auto nc) {
                using R = decltype(r);
                for (int64_t b = 0; b < nblocks; b++) {
                    int32_t sw = 0;
                    const int st = eigh_block_host<R, decltype(nc)::value>((R *)blocks[b], n[b], ld[b], (R *)w[b], vectors != 0, sw);
                    if (info) info[b] = st;
                    if (sweeps) sweeps[b] = sw;
                }
            });
            return BSM_OK;
        }
        const int es = elem_bytes(dtype), rs = real_bytes(dtype);
        std::vector<EighBlock> table;
        for (int64_t b = 0; b < nblocks; b++)
            if (n[b] > 0)
                table.push_back(EighBlock{(uint64_t)(uintptr_t)blocks[b], (uint64_t)(uintptr_t)w[b], 0, (long long)ld[b], 0, (int)n[b],
                                          (int)table.size()});
        std::vector<int> hinfo;
        rc = run_device(
            table, es, 2, (hipStream_t)stream, [&](const EighBlock &t) { return eigh_resident(t.n, es); },
            [&](int nn, bool res) { return eigh_lds(nn, es, rs, res).total; },
            [&](const EighBlock *d, long long count, int nmax, bool res, int *d_info) {
                return launch_eigh(dtype, d, count, nmax, res, vectors != 0, d_info, (hipStream_t)stream);
            },
            vectors != 0, hinfo);
        if (rc != BSM_OK) return rc;
        int64_t k = 0;  // record ids count the non-empty blocks in the caller's order
        for (int64_t b = 0; b < nblocks; b++)
            if (n[b] > 0) {
                if (info) info[b] = hinfo[(size_t)(2 * k)];
                if (sweeps) sweeps[b] = hinfo[(size_t)(2 * k + 1)];
                k++;
            }
        return BSM_OK;)
}

extern "C" int bsm_spectral_blocks(int dtype, int64_t nblocks, const void *const *V, const int64_t *n, const int64_t *ldv,
                                   const void *const *w, int32_t func, double rcond, void *const *out, const int64_t *ldo, int64_t *info,
                                   int memspace, void *stream) {
    BSM_GUARDED(
        int rc = check_blocks("bsm_spectral_blocks", dtype, nblocks, V, n, ldv, memspace);
        if (rc != BSM_OK) return rc;
        if (func < BSM_SPEC_VALUES || func > BSM_SPEC_PINV) return fail(BSM_ERR_INVALID, "bad func");
        if (!(rcond >= 0)) return fail(BSM_ERR_INVALID, "rcond is negative or NaN");
        if (nblocks > 0 && (!w || !out || !ldo)) return fail(BSM_ERR_INVALID, "null argument");
        for (int64_t b = 0; b < nblocks; b++) {
            const std::string blk = "block " + std::to_string(b + 1) + ": ";
            if (ldo[b] < std::max<int64_t>(n[b], 1)) return fail(BSM_ERR_INVALID, blk + "ldo < max(n, 1)");
            if (n[b] > 0 && (!w[b] || !out[b])) return fail(BSM_ERR_INVALID, blk + "null w or out");
        }
        rc = check_order(nblocks, n);
        if (rc != BSM_OK) return rc;
        if (info) std::fill(info, info + nblocks, (int64_t)0);
        if (memspace == BSM_MEM_HOST) {
            with_types(dtype, [&](auto r, auto, auto nc) {
                using R = decltype(r);
                for (int64_t b = 0; b < nblocks; b++) {
                    const int64_t st = spectral_block_host<R, decltype(nc)::value>((const R *)V[b], n[b], ldv[b], (const R *)w[b], func, rcond,
                                                                          (R *)out[b], ldo[b]);
                    if (info) info[b] = st;
                }
            });
            return BSM_OK;
        }
        const int es = elem_bytes(dtype), rs = real_bytes(dtype);
        std::vector<EighBlock> table;
        for (int64_t b = 0; b < nblocks; b++)
            if (n[b] > 0)
                table.push_back(EighBlock{(uint64_t)(uintptr_t)V[b], (uint64_t)(uintptr_t)w[b], (uint64_t)(uintptr_t)out[b], (long long)ldv[b],
                                          (long long)ldo[b], (int)n[b], (int)table.size()});
        std::vector<int> hinfo;
        rc = run_device(
            table, es, 1, (hipStream_t)stream, [&](const EighBlock &t) { return spectral_staged(t.n, es); },
            [&](int nn, bool staged) { return spectral_lds(nn, es, rs, staged); },
            [&](const EighBlock *d, long long count, int nmax, bool staged, int *d_info) {
                return launch_spectral(dtype, d, count, nmax, staged, func, rcond, d_info, (hipStream_t)stream);
            },
            false, hinfo);
        if (rc != BSM_OK) return rc;
        int64_t k = 0;
        for (int64_t b = 0; b < nblocks; b++)
            if (n[b] > 0) {
                if (info) info[b] = hinfo[(size_t)k];
                k++;
            }
        return BSM_OK;)
}
