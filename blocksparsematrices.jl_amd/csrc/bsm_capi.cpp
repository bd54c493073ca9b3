// bsm_capi.cpp -- the extern "C" surface of libbsmrocm.so (include/bsm_rocm.h), but for the features whose unit holds
// its own entry points: reading entries (bsm_entries.cpp), the block inverse (bsm_invert.cpp), the Gram-Schmidt pass
// (bsm_krylov.cpp), the solvers (bsm_cg.cpp, ...), composed handles (bsm_poly.cpp).
// Plain pointers and sizes only; checks and converts arguments, has the operator built, refilled and
// released (bsm_operator.cpp: LocalOperator; bsm_dist.cpp for handles over several devices) and
// forwards bsm_mul to the HIP launchers.  Never throws across the ABI.
#include <hip/hip_runtime_api.h>

#include <algorithm>
#include <climits>
#include <cstdlib>
#include <cstring>
#include <mutex>
#include <new>
#include <string>
#include <vector>

#include "bsm_internal.h"

using namespace bsm;

namespace {
// RAII staging buffers: cached in the handle when uncontended, temporary otherwise
struct Staging {
    // the handle's buffer p (capacity `cap` bytes) holds at least `bytes`
    static hipError_t grow(void *&p, size_t &cap, size_t bytes) {
        if (cap >= bytes) return hipSuccess;
        if (p) (void)hipFree(p);
        p = nullptr;
        cap = 0;
        const hipError_t e = hipMalloc(&p, bytes + 16);
        if (e == hipSuccess) cap = bytes;
        return e;
    }
    bsm_matrix_s *A;
    bool locked = false;
    void *dx = nullptr, *dy = nullptr;
    bool own = false;
    hipError_t acquire(bsm_matrix_s *a, size_t xbytes, size_t ybytes) {
        A = a;
        locked = A->host_mu.try_lock();
        hipError_t e = hipSuccess;
        if (locked) {
            e = grow(A->stage_x, A->stage_x_bytes, xbytes);
            if (e == hipSuccess) e = grow(A->stage_y, A->stage_y_bytes, ybytes);
            if (e != hipSuccess) return e;
            dx = A->stage_x;
            dy = A->stage_y;
        } else {
            own = true;
            e = hipMalloc(&dx, xbytes + 16);
            if (e == hipSuccess) e = hipMalloc(&dy, ybytes + 16);
        }
        return e;
    }
    ~Staging() {
        if (own) {
            if (dx) (void)hipFree(dx);
            if (dy) (void)hipFree(dy);
        }
        if (locked) A->host_mu.unlock();
    }
};
}  // namespace

static thread_local std::string g_err;

namespace bsm {
int fail(int code, const std::string &msg) {
    g_err = msg;
    return code;
}

int hip_fail(hipError_t e, const char *what) {
    return fail(BSM_ERR_DEVICE, std::string(what) + ": " + hipGetErrorString(e));
}

hipError_t DeviceGuard::enter(int dev) {
    hipError_t e = hipGetDevice(&prev);
    if (e != hipSuccess) return e;
    if (prev != dev) {
        e = hipSetDevice(dev);
        if (e != hipSuccess) return e;
        active = true;
    }
    return hipSuccess;
}
DeviceGuard::~DeviceGuard() {
    if (active) (void)hipSetDevice(prev);
}
}  // namespace bsm

extern "C" const char *bsm_last_error(void) { return g_err.c_str(); }

#ifndef BSM_BUILD_ID
#define BSM_BUILD_ID "unknown"
#endif
extern "C" const char *bsm_version(void) { return "bsmrocm 0.3 gfx950 build " BSM_BUILD_ID; }

extern "C" void bsm_options_default(bsm_options *o) {
    if (!o) return;
    std::memset(o, 0, sizeof *o);
    o->struct_size = (int32_t)sizeof(bsm_options);
    o->device = BSM_DEVICE_CURRENT;
    o->scheduler = BSM_SCHED_SERIAL;
    o->accumulate = BSM_ACC_AUTO;
    o->validate = 1;
}

namespace bsm {

int read_options(const bsm_options *opts, bsm_options &o) {
    bsm_options_default(&o);
    if (opts) {
        if (opts->struct_size != (int32_t)sizeof(bsm_options))
            return fail(BSM_ERR_INVALID, "bsm_options.struct_size mismatch (call bsm_options_default)");
        o = *opts;
    }
    if (o.accumulate != BSM_ACC_AUTO && o.accumulate != BSM_ACC_ATOMIC && o.accumulate != BSM_ACC_COLORED &&
        o.accumulate != BSM_ACC_GATHER && o.accumulate != BSM_ACC_DIRECT)
        return fail(BSM_ERR_INVALID, "unknown accumulate mode");
    if (o.own_lo < 0 || o.own_hi < 0 || (o.own_hi > 0 && o.own_hi < o.own_lo))
        return fail(BSM_ERR_INVALID, "bad own_lo/own_hi");
    if (o.transpose_image < 0 || o.transpose_image > 2) return fail(BSM_ERR_INVALID, "bad transpose_image");
    if (o.coloring != BSM_COLOR_WORKSTREAM_DSATUR && o.coloring != BSM_COLOR_DSATUR)
        return fail(BSM_ERR_INVALID, "unknown colouring algorithm");
    if (o.blocks_memspace != BSM_MEM_HOST && o.blocks_memspace != BSM_MEM_DEVICE)
        return fail(BSM_ERR_INVALID, "bad blocks_memspace");
    return BSM_OK;
}

// analysis errors are the caller's (bad arguments); the value sink reports device failures
int build_error(const std::string &err) {
    const bool device = err.compare(0, 3, "hip") == 0 || err.find("upload") != std::string::npos ||
                        err.find("value sink") != std::string::npos;
    return fail(device ? BSM_ERR_DEVICE : BSM_ERR_INVALID, err);
}

}  // namespace bsm

namespace {

// A *_create call owns its half-built handle until release(): any early return or exception destroys it, device side
// included.  The target device is made current BEFORE the operator is built, so that the packer can stream the values
// to it instead of building a host copy first.
struct CreateCtx {
    bsm_matrix_s *A = new bsm_matrix_s();
    DeviceGuard guard;
    CreateCtx() = default;
    CreateCtx(const CreateCtx &) = delete;
    ~CreateCtx() { (void)bsm_destroy(A); }
    bsm_matrix_s *release() {
        bsm_matrix_s *p = A;
        A = nullptr;
        return p;
    }
    int open(const bsm_options &o) {
        if (o.device == BSM_DEVICE_NONE) return BSM_OK;
        int dev = o.device;
        if (dev == BSM_DEVICE_CURRENT) {
            hipError_t e = hipGetDevice(&dev);
            if (e != hipSuccess) return hip_fail(e, "hipGetDevice");
        }
        hipError_t e = guard.enter(dev);
        if (e != hipSuccess) return hip_fail(e, "hipSetDevice");
        A->device = dev;
        return BSM_OK;
    }
};

// one block of a *_create call: contiguous rows / columns from (r0, c0), or on index lists (all 1-based)
BlockIn block_at(const void *data, int64_t m, int64_t n, int64_t ld, int64_t r0, int64_t c0, int kind) {
    return BlockIn{(const char *)data, m, n, ld, nullptr, nullptr, r0, c0, kind};
}
BlockIn block_on(const void *data, int64_t m, int64_t n, int64_t ld, const int64_t *ridx, const int64_t *cidx, int kind) {
    return BlockIn{(const char *)data, m, n, ld, ridx, cidx, 0, 0, kind};
}

std::vector<int64_t> iota_ids(size_t n) {  // input block ids of a list kept in the caller's order
    std::vector<int64_t> v(n);
    for (size_t b = 0; b < n; b++) v[b] = (int64_t)b;
    return v;
}

// Common tail of every *_create: `in` is the block list in its final order (VBCRS: sorted, with
// A->an's perm / rowptr / ... already filled).  Single device: analysis + packing + upload; with
// bsm_options.ctx: whole-operator bookkeeping, then one image per device of the context.
int create_handle(int mtype, int dtype, int64_t nrows, int64_t ncols, const std::vector<BlockIn> &in,
                  const std::vector<int64_t> &ids, const bsm_options &o, CreateCtx &cx, bsm_matrix_t *out) {
    bsm_matrix_s *A = cx.A;
    // stored shape of every input block (bsm_update_blocks checks the new ones against it)
    A->blk_m.assign(in.size(), 0);
    A->blk_n.assign(in.size(), 0);
    for (size_t b = 0; b < in.size(); b++) {
        A->blk_m[(size_t)ids[b]] = in[b].m;
        A->blk_n[(size_t)ids[b]] = in[b].n;
    }
    if (o.ctx && is_mixed(dtype))
        return fail(BSM_ERR_UNSUPPORTED, "mixed-precision storage (BSM_F64_F32 / BSM_C128_C64) is single-device only: "
                                         "create without bsm_options.ctx");
    if (o.ctx) {
        AnalysisOptions ao = to_aopt(o, nullptr);
        ao.meta_only = true;
        ao.own_lo = ao.own_hi = 0;
        std::string err = A->an.build(mtype, dtype, nrows, ncols, in, ao);
        if (!err.empty()) return build_error(err);
        int rc = dist_create(A, (bsm_ctx_s *)o.ctx, mtype, dtype, nrows, ncols, in, ids, o);
        if (rc != BSM_OK) return rc;  // ~CreateCtx releases whatever the parts already hold
        A->on_device = true;
        *out = cx.release();
        return BSM_OK;
    }
    int rc = cx.open(o);
    if (rc != BSM_OK) return rc;
    rc = A->build(mtype, dtype, nrows, ncols, in, ids, (int64_t)in.size(), o, true, "");
    if (rc != BSM_OK) return rc;
    A->on_device = A->device != BSM_DEVICE_NONE;
    *out = cx.release();
    return BSM_OK;
}

// VBCRS front end (reference src/vbcrs.jl:84-117): stable sort by (rowstart, colstart), rowptr, ...
int create_vbcrs(int dtype, int64_t nrows, int64_t ncols, const std::vector<BlockIn> &unsorted,
                 const bsm_options &o, bsm_matrix_t *out) {
    const int64_t nb = (int64_t)unsorted.size();
    std::vector<int64_t> rs(nb), cs(nb);
    for (int64_t b = 0; b < nb; b++) {
        rs[b] = unsorted[b].r0;
        cs[b] = unsorted[b].c0;
    }
    CreateCtx cx;
    const std::vector<int64_t> p = cx.A->an.vbcrs_bookkeeping(nb, rs.data(), cs.data());
    std::vector<BlockIn> in(nb);
    for (int64_t k = 0; k < nb; k++) in[k] = unsorted[p[k]];
    return create_handle(MT_VBCRS, dtype, nrows, ncols, in, p, o, cx, out);  // block k of the image is input p[k]
}

}  // namespace

extern "C" int bsm_vbcrs_create(int dtype, int64_t nrows, int64_t ncols, int64_t nblocks,
                                const void *const *blocks, const int64_t *m, const int64_t *n,
                                const int64_t *ld, const int64_t *rowstart, const int64_t *colstart,
                                const bsm_options *opts, bsm_matrix_t *out) {
    BSM_GUARDED(
        if (!out) return fail(BSM_ERR_INVALID, "out is null");
        *out = nullptr;
        if (nblocks < 1) return fail(BSM_ERR_INVALID, "VBCRS needs at least one block (reference src/vbcrs.jl:81)");
        if (!blocks || !m || !n || !ld || !rowstart || !colstart) return fail(BSM_ERR_INVALID, "null argument");
        bsm_options o;
        int rc = read_options(opts, o);
        if (rc) return rc;
        std::vector<BlockIn> in((size_t)nblocks);
        for (int64_t b = 0; b < nblocks; b++) in[b] = block_at(blocks[b], m[b], n[b], ld[b], rowstart[b], colstart[b], KIND_PLAIN);
        return create_vbcrs(dtype, nrows, ncols, in, o, out);)
}

extern "C" int bsm_vbcrs_create_from_blocksparse(int dtype, int64_t nrows, int64_t ncols, int64_t nblocks,
                                                 const void *const *blocks, const int64_t *m,
                                                 const int64_t *n, const int64_t *ld,
                                                 const int64_t *const *rowidx, const int64_t *const *colidx,
                                                 const bsm_options *opts, bsm_matrix_t *out) {
    BSM_GUARDED(
        if (!out) return fail(BSM_ERR_INVALID, "out is null");
        *out = nullptr;
        if (nblocks < 1) return fail(BSM_ERR_INVALID, "VBCRS needs at least one block (reference src/vbcrs.jl:81)");
        if (!blocks || !m || !n || !ld || !rowidx || !colidx) return fail(BSM_ERR_INVALID, "null argument");
        bsm_options o;
        int rc = read_options(opts, o);
        if (rc) return rc;
        std::vector<BlockIn> in((size_t)nblocks);
        for (int64_t b = 0; b < nblocks; b++) {
            // first(rowindices(bsm, i)), first(colindices(bsm, i)): reference src/vbcrs.jl:201-215
            if (m[b] < 1 || n[b] < 1 || !rowidx[b] || !colidx[b])
                return fail(BSM_ERR_INVALID, "block " + std::to_string(b + 1) + ": empty index list (first() of it is undefined)");
            in[b] = block_at(blocks[b], m[b], n[b], ld[b], rowidx[b][0], colidx[b][0], KIND_PLAIN);
        }
        return create_vbcrs(dtype, nrows, ncols, in, o, out);)
}

extern "C" int bsm_vbcrs_create_from_symmetric(int dtype, int64_t nrows, int64_t ncols, int64_t ndiag,
                                               const void *const *diag, const int64_t *dsize,
                                               const int64_t *dld, const int64_t *diagstart,
                                               int64_t noff, const void *const *off, const int64_t *m,
                                               const int64_t *n, const int64_t *ld,
                                               const int64_t *rowstart, const int64_t *colstart,
                                               const bsm_options *opts, bsm_matrix_t *out) {
    BSM_GUARDED(
        if (!out) return fail(BSM_ERR_INVALID, "out is null");
        *out = nullptr;
        if (ndiag < 0 || noff < 0 || ndiag + noff < 1) return fail(BSM_ERR_INVALID, "VBCRS needs at least one block");
        if (ndiag > 0 && (!diag || !dsize || !dld || !diagstart)) return fail(BSM_ERR_INVALID, "null argument");
        if (noff > 0 && (!off || !m || !n || !ld || !rowstart || !colstart)) return fail(BSM_ERR_INVALID, "null argument");
        bsm_options o;
        int rc = read_options(opts, o);
        if (rc) return rc;
        // bookkeeping over the virtual block list of the reference's functors (src/vbcrs.jl:222-262):
        // [diagonals..., offdiagonals..., transpose(offdiagonals)...]
        const int64_t nv = ndiag + 2 * noff;
        std::vector<int64_t> rs(nv), cs(nv);
        for (int64_t d = 0; d < ndiag; d++) rs[d] = cs[d] = diagstart[d];
        for (int64_t b = 0; b < noff; b++) {
            rs[ndiag + b] = rowstart[b];
            cs[ndiag + b] = colstart[b];
            rs[ndiag + noff + b] = colstart[b];
            cs[ndiag + noff + b] = rowstart[b];
        }
        CreateCtx cx;
        cx.A->an.vbcrs_bookkeeping(nv, rs.data(), cs.data());
        // ... the image keeps every off-diagonal block once (the symmetric one)
        std::vector<BlockIn> in;
        in.reserve((size_t)(ndiag + noff));
        for (int64_t d = 0; d < ndiag; d++) in.push_back(block_at(diag[d], dsize[d], dsize[d], dld[d], diagstart[d], diagstart[d], KIND_DIAG));
        for (int64_t b = 0; b < noff; b++) in.push_back(block_at(off[b], m[b], n[b], ld[b], rowstart[b], colstart[b], KIND_OFF));
        return create_handle(MT_VBCRS, dtype, nrows, ncols, in, iota_ids(in.size()), o, cx, out);)
}

extern "C" int bsm_blocksparse_create(int dtype, int64_t nrows, int64_t ncols, int64_t nblocks,
                                      const void *const *blocks, const int64_t *m, const int64_t *n,
                                      const int64_t *ld, const int64_t *const *rowidx,
                                      const int64_t *const *colidx, const bsm_options *opts,
                                      bsm_matrix_t *out) {
    BSM_GUARDED(
        if (!out) return fail(BSM_ERR_INVALID, "out is null");
        *out = nullptr;
        if (nblocks < 0) return fail(BSM_ERR_INVALID, "negative block count");
        if (nblocks > 0 && (!blocks || !m || !n || !ld || !rowidx || !colidx)) return fail(BSM_ERR_INVALID, "null argument");
        bsm_options o;
        int rc = read_options(opts, o);
        if (rc) return rc;
        std::vector<BlockIn> in((size_t)nblocks);
        for (int64_t b = 0; b < nblocks; b++) {
            const BlockIn &B = in[b] = block_on(blocks[b], m[b], n[b], ld[b], rowidx[b], colidx[b], KIND_PLAIN);
            if ((B.m > 0 && !B.ridx) || (B.n > 0 && !B.cidx))
                return fail(BSM_ERR_INVALID, "block " + std::to_string(b + 1) + ": null index list");
        }
        CreateCtx cx;
        return create_handle(MT_BLOCKSPARSE, dtype, nrows, ncols, in, iota_ids(in.size()), o, cx, out);)
}

extern "C" int bsm_symmetric_create(int dtype, int64_t nrows, int64_t ncols, int64_t ndiag,
                                    const void *const *diag, const int64_t *dsize, const int64_t *dld,
                                    const int64_t *const *diagidx, int64_t noff,
                                    const void *const *off, const int64_t *m, const int64_t *n,
                                    const int64_t *ld, const int64_t *const *rowidx,
                                    const int64_t *const *colidx, const bsm_options *opts,
                                    bsm_matrix_t *out) {
    BSM_GUARDED(
        if (!out) return fail(BSM_ERR_INVALID, "out is null");
        *out = nullptr;
        if (ndiag < 0 || noff < 0) return fail(BSM_ERR_INVALID, "negative block count");
        if (ndiag > 0 && (!diag || !dsize || !dld || !diagidx)) return fail(BSM_ERR_INVALID, "null argument");
        if (noff > 0 && (!off || !m || !n || !ld || !rowidx || !colidx)) return fail(BSM_ERR_INVALID, "null argument");
        bsm_options o;
        int rc = read_options(opts, o);
        if (rc) return rc;
        std::vector<BlockIn> in;
        in.reserve((size_t)(ndiag + noff));
        for (int64_t d = 0; d < ndiag; d++) {
            const BlockIn B = block_on(diag[d], dsize[d], dsize[d], dld[d], diagidx[d], diagidx[d], KIND_DIAG);
            if (B.m > 0 && !B.ridx)
                return fail(BSM_ERR_INVALID, "diagonal block " + std::to_string(d + 1) + ": null index list");
            in.push_back(B);
        }
        for (int64_t b = 0; b < noff; b++) {
            const BlockIn B = block_on(off[b], m[b], n[b], ld[b], rowidx[b], colidx[b], KIND_OFF);
            if ((B.m > 0 && !B.ridx) || (B.n > 0 && !B.cidx))
                return fail(BSM_ERR_INVALID, "off-diagonal block " + std::to_string(b + 1) + ": null index list");
            in.push_back(B);
        }
        CreateCtx cx;
        return create_handle(MT_SYMMETRIC, dtype, nrows, ncols, in, iota_ids(in.size()), o, cx, out);)
}

// ---- contexts of devices (multi-GPU handles) -----------------------------------------------------
extern "C" int bsm_ctx_create(const int32_t *device_ids, int32_t ndevices, bsm_ctx_t *out) {
    BSM_GUARDED(
        if (!out) return fail(BSM_ERR_INVALID, "out is null");
        *out = nullptr;
        if (ndevices < 1 || ndevices > 64 || !device_ids) return fail(BSM_ERR_INVALID, "a context needs 1..64 devices");
        int count = 0;
        hipError_t e = hipGetDeviceCount(&count);
        if (e != hipSuccess) return hip_fail(e, "hipGetDeviceCount");
        std::unique_ptr<bsm_ctx_s> ctx(new bsm_ctx_s());
        for (int32_t i = 0; i < ndevices; i++) {
            if (device_ids[i] < 0 || device_ids[i] >= count)
                return fail(BSM_ERR_INVALID, "device ordinal " + std::to_string(device_ids[i]) + " does not exist");
            ctx->devices.push_back(device_ids[i]);
        }
        // direct xGMI access between every pair of distinct devices (the halo copies then run device
        // to device; without it the runtime stages them through host memory, still correct)
        // (what the fused fan-out kernels of bsm_fanout.cpp rely on is that the access was ENABLED, not that it is
        // possible: only hipSuccess / "already enabled" count, anything else leaves the context on the copy path)
        ctx->peer_ok = true;
        for (int a : ctx->devices)
            for (int b : ctx->devices) {
                if (a == b) continue;
                int can = 0;
                if (hipDeviceCanAccessPeer(&can, a, b) != hipSuccess || !can) {
                    (void)hipGetLastError();
                    ctx->peer_ok = false;
                    continue;
                }
                DeviceGuard g;
                if (g.enter(a) != hipSuccess) {
                    (void)hipGetLastError();
                    ctx->peer_ok = false;
                    continue;
                }
                const hipError_t pe = hipDeviceEnablePeerAccess(b, 0);
                if (pe != hipSuccess) {
                    (void)hipGetLastError();
                    if (pe != hipErrorPeerAccessAlreadyEnabled) ctx->peer_ok = false;
                }
            }
        *out = ctx.release();
        return BSM_OK;)
}

extern "C" int bsm_ctx_destroy(bsm_ctx_t ctx) {
    delete ctx;
    return BSM_OK;
}

extern "C" int bsm_ctx_devices(bsm_ctx_t ctx, int32_t *ndevices, int32_t *device_ids, int32_t capacity) {
    if (!ctx || !ndevices) return fail(BSM_ERR_INVALID, "null argument");
    *ndevices = (int32_t)ctx->devices.size();
    if (device_ids) {
        if (capacity < *ndevices) return fail(BSM_ERR_INVALID, "output buffer too small");
        for (size_t i = 0; i < ctx->devices.size(); i++) device_ids[i] = ctx->devices[i];
    }
    return BSM_OK;
}

extern "C" int bsm_partition_rows(int64_t nrows, int64_t nblocks, const int64_t *rowkey, const int64_t *weight,
                                  int32_t nparts, int32_t *part_of_block, int64_t *own_lo, int64_t *own_hi) {
    BSM_GUARDED(
        if (nparts < 1 || nblocks < 0 || nrows < 0 || !own_lo || !own_hi || (nblocks > 0 && (!rowkey || !weight || !part_of_block)))
            return fail(BSM_ERR_INVALID, "bad argument");
        std::vector<int64_t> key(rowkey, rowkey + nblocks), w(weight, weight + nblocks), lo, hi;
        for (int64_t b = 0; b < nblocks; b++)
            if (key[b] < 1 || key[b] > std::max<int64_t>(nrows, 1)) return fail(BSM_ERR_INVALID, "row key outside the matrix");
        std::vector<int32_t> part;
        partition_rows(nrows, key, w, nparts, part, lo, hi);
        for (int64_t b = 0; b < nblocks; b++) part_of_block[b] = part[b];
        for (int32_t p = 0; p < nparts; p++) {
            own_lo[p] = lo[p];
            own_hi[p] = hi[p];
        }
        return BSM_OK;)
}

extern "C" int bsm_host_register(void *ptr, int64_t bytes) {
    if (!ptr || bytes <= 0) return fail(BSM_ERR_INVALID, "bad argument");
    hipError_t e = hipHostRegister(ptr, (size_t)bytes, hipHostRegisterDefault);
    if (e != hipSuccess) return hip_fail(e, "hipHostRegister");
    return BSM_OK;
}

extern "C" int bsm_host_unregister(void *ptr) {
    if (!ptr) return BSM_OK;
    hipError_t e = hipHostUnregister(ptr);
    if (e != hipSuccess) return hip_fail(e, "hipHostUnregister");
    return BSM_OK;
}

// A compute stream that leaves CUs to the collective layer.  Measured with the one-rank RCCL loopback of the C5 step
// (tools/loopback_trace.py, profiles/r05_loopback_*.txt): beside a product launch that fills every CU, RCCL's send /
// recv kernel (one large workgroup per channel) found no CU with enough free registers and LDS at once -- 8 us alone,
// 470 us beside the interior launch, i.e. the "overlapped" exchange finished when the product did.  With the product
// on a stream whose CU mask leaves one CU per XCD free the exchange runs beside it (87-137 us, hidden) and the step
// shrinks from 698 to 656 us at 1 % cost for the product.  Mask bit i is CU i / 8 of XCD i % 8 on this part: clearing
// bits in groups of 8 keeps the XCDs equal -- masks that do not (4 CUs of one XCD: 917 instead of 615 us) slow every
// launch, which is why `reserved_cus` is rounded up to a multiple of 8.
extern "C" int bsm_stream_create_reserved(int device, int reserved_cus, void **stream) {
    if (!stream || reserved_cus < 0) return fail(BSM_ERR_INVALID, "bad argument");
    DeviceGuard g;
    hipError_t e = g.enter(device);
    if (e != hipSuccess) return hip_fail(e, "hipSetDevice");
    int ncu = 0;
    e = hipDeviceGetAttribute(&ncu, hipDeviceAttributeMultiprocessorCount, device);
    if (e != hipSuccess) return hip_fail(e, "hipDeviceGetAttribute");
    const int r = std::min((reserved_cus + 7) / 8 * 8, std::max(ncu - 8, 0));
    hipStream_t st = nullptr;
    if (r == 0) {
        e = hipStreamCreateWithFlags(&st, hipStreamNonBlocking);
    } else {
        std::vector<uint32_t> mask((size_t)(ncu + 31) / 32, 0u);
        for (int i = r; i < ncu; i++) mask[(size_t)i / 32] |= 1u << (i % 32);
        e = hipExtStreamCreateWithCUMask(&st, (uint32_t)mask.size(), mask.data());
    }
    if (e != hipSuccess) return hip_fail(e, "stream creation");
    *stream = (void *)st;
    return BSM_OK;
}

extern "C" int bsm_stream_destroy(void *stream) {
    if (!stream) return BSM_OK;
    hipError_t e = hipStreamDestroy((hipStream_t)stream);
    if (e != hipSuccess) return hip_fail(e, "hipStreamDestroy");
    return BSM_OK;
}

extern "C" int bsm_vec_add_segments(int dtype, void *y, int32_t nseg, const int64_t *offset, const void *const *src,
                                    const int64_t *len, void *stream) {
    const std::string why = vec_type_refusal("bsm_vec_add_segments", dtype);
    if (!why.empty()) return fail(BSM_ERR_INVALID, why);
    if (nseg < 0 || (nseg > 0 && (!y || !offset || !src || !len))) return fail(BSM_ERR_INVALID, "null argument");
    // disjoint segments only: the launch adds without atomics
    for (int32_t a = 0; a < nseg; a++) {
        if (offset[a] < 0 || len[a] < 0 || (len[a] > 0 && !src[a])) return fail(BSM_ERR_INVALID, "bad segment");
        for (int32_t b = a + 1; b < nseg; b++)
            if (len[a] > 0 && len[b] > 0 && offset[a] < offset[b] + len[b] && offset[b] < offset[a] + len[a])
                return fail(BSM_ERR_INVALID, "segments overlap");
    }
    for (int32_t c = 0; c < nseg;) {  // kMaxVecPieces non-empty segments per launch
        VecPieces pc;
        int np = 0;
        for (; c < nseg && np < kMaxVecPieces; c++) {
            if (len[c] == 0) continue;
            pc.base[np] = src[c];
            pc.lo[np] = offset[c];
            pc.hi[np] = offset[c] + len[c];
            pc.strided[np] = 0;
            np++;
        }
        if (np == 0) break;
        hipError_t e = launch_vec_add_segments(dtype, y, pc, np, (hipStream_t)stream);
        if (e != hipSuccess) return hip_fail(e, "segment add launch");
    }
    return BSM_OK;
}

extern "C" int bsm_part_info(bsm_matrix_t A, int32_t part, bsm_part_info_t *out) {
    if (!A || !out) return fail(BSM_ERR_INVALID, "null argument");
    if (int rc = poly_refusal(A, "bsm_part_info")) return rc;
    if (!A->dist) return fail(BSM_ERR_INVALID, "not a multi-device handle");
    return dist_part_info(A, part, out);
}

// The gather workspace of an image (column sums + inverted indices) and the work arrays of the interleaved multi-RHS pass
// (Xr, W: 128 bytes per vector entry each) belong to the handle and admit ONE product in flight each.  The enqueue is
// serialised; a caller that races on the same handle from another thread, or whose predecessor may still be running on
// ANOTHER stream (same stream: stream order protects it), does not get the claim and its product takes the kernels that
// need neither (atomic path, ordinary multi-RHS kernels).  Nothing is enqueued for the bookkeeping (an event recorded
// per product costs 3 us between two 9 us launches): the previous stream is queried only when the stream changes.  A
// product enqueued while the stream is being captured into a graph never gets the claim: a replay would use the
// resource on whatever stream, beside eager products nobody can order against.
struct Claim {
    ClaimState &c;
    hipStream_t st;
    std::unique_lock<std::mutex> lock;
    bool held = false;
    Claim(ClaimState &c_, bool wanted, hipStream_t st_) : c(c_), st(st_), lock(c_.mu, std::defer_lock) {
        if (!wanted || !lock.try_lock() || capturing(st)) return;
        if (c.pending && c.stream != st) {  // the stream changed: is the previous one idle?
            const hipError_t q = hipStreamQuery(c.stream);
            if (q != hipSuccess) {
                (void)hipGetLastError();  // hipErrorNotReady is not a failure
                // (any other answer -- the stream may be gone -- is treated the same way once, then
                // forgotten: work of a destroyed stream does not outlive a whole product by much)
                if (q != hipErrorNotReady) c.pending = false;
                return;
            }
            c.pending = false;
        }
        held = true;
    }
    // before the resource is freed (a regrow): wait for the product that may still use it
    void drain() {
        if (c.pending && hipStreamSynchronize(c.stream) != hipSuccess) (void)hipGetLastError();
        c.pending = false;
    }
    void mark() {  // after the product has been enqueued
        if (!held) return;
        c.stream = st;
        c.pending = true;
    }
};

// the complex gather workspace of a real image (bsm_mul_cvec), allocated at the first complex gather product -- under
// the claim, so no product uses it yet; never regrown.  false: no memory (the product takes the atomic path)
static bool wsc_reserve(const Analysis &an, DeviceImage &img, hipStream_t st) {
    if (img.d_wsc) return true;
    const size_t bytes = (size_t)(an.ws_slots + 8) * (size_t)an.vs * 2;
    void *p = nullptr;
    if (hipMalloc(&p, bytes) != hipSuccess || hipMemsetAsync(p, 0, bytes, st) != hipSuccess) {
        (void)hipGetLastError();
        if (p) (void)hipFree(p);
        return false;
    }
    img.d_wsc = p;
    return true;
}

// the product after its argument checks (one column: K = 1, ld = max(length, 1)); vt: the dtype code of the vectors
static int mul_k(bsm_matrix_s *A, int op, long long K, const void *X, long long ldx, void *Y, long long ldy,
                 const void *alpha, const void *beta, int beta_strong_zero, int memspace, hipStream_t st, int vt) {
    if (A->dist)  // multi-device handles: every device streams its part once per batch of <= 16 columns
        return dist_mul_multi(A, op, K, X, ldx, Y, ldy, alpha, beta, beta_strong_zero, memspace, st);
    // transposed products run forward on the second ordering when the handle has one
    const bool use_t = (op != BSM_OP_N) && A->has_t;
    DeviceImage &img = use_t ? A->img_t : A->img;
    const bool opT = (op != BSM_OP_N) && !use_t;
    const bool conj = (op == BSM_OP_C);
    DeviceGuard guard;
    hipError_t e = guard.enter(img.device);
    if (e != hipSuccess) return hip_fail(e, "hipSetDevice");
    // one column: the gather workspace (if the image has one); more: the interleaved pass's work arrays (if it applies)
    Claim claim(K == 1 ? A->ws_claim : A->il_claim, K == 1 ? img.d_ws != nullptr : wants_il_arrays(plan_input(img, opT, vt, K, false)), st);
    // (complex vectors under a real image gather into the complex workspace)
    if (claim.held && K == 1 && vt != img.dtype && img.dtype <= BSM_F64 && !wsc_reserve(use_t ? A->an_t : A->an, img, st))
        claim.held = false;  // no memory for the complex workspace: the atomic path needs none
    ILWork *il = nullptr;
    if (claim.held && K > 1) {  // allocated (and grown) here, at the first product that uses them
        const long long need = std::max(img.nrows, img.ncols);
        if (A->il.rows < need) claim.drain();  // a regrow frees the arrays the previous claim's product may still read
        if (il_reserve(A->il, need))
            il = &A->il;
        else
            claim.held = false;  // no memory for the work arrays: the ordinary kernels need none
    }
    const bool gather = K == 1 && claim.held;
    if (memspace == BSM_MEM_DEVICE) {
        e = launch_mul(img, opT, conj, K, X, ldx, Y, ldy, alpha, beta, beta_strong_zero, st, gather, nullptr, il, vt);
        if (e != hipSuccess) return hip_fail(e, "kernel launch");
        claim.mark();
        return BSM_OK;
    }
    if (memspace != BSM_MEM_HOST) return fail(BSM_ERR_INVALID, "bad memspace");
    // host vectors: stage through device buffers (PCIe), synchronous
    const size_t es = (size_t)elem_bytes(vt);
    const long long xlen = (op == 0 ? A->an.ncols : A->an.nrows);
    const long long ylen = (op == 0 ? A->an.nrows : A->an.ncols);
    Staging sg;
    e = sg.acquire(A, (size_t)xlen * K * es, (size_t)ylen * K * es);
    void *dx = sg.dx, *dy = sg.dy;
    // K columns between host (ld) and staging (len, packed); one column: a plain copy
    auto copy = [&](void *dst, long long ldd, const void *src, long long lds, long long len, hipMemcpyKind kind) {
        if (K == 1) return hipMemcpyAsync(dst, src, (size_t)len * es, kind, st);
        return hipMemcpy2DAsync(dst, (size_t)ldd * es, src, (size_t)lds * es, (size_t)len * es, (size_t)K, kind, st);
    };
    // the incoming y travels when beta uses it -- and whenever the handle owns only a row range: rows
    // outside it that no block reaches are left untouched by the product and must come back unchanged
    const bool partial = (op == BSM_OP_N) && (img.own_lo > 0 || img.own_hi < img.nrows);
    const bool y_in = !beta_strong_zero || partial;
    // (page-locked vectors -- bsm_host_register -- make both copies true DMA; pageable ones are staged
    // by the runtime: 74 vs 118 us per C2-sized product)
    if (e == hipSuccess) e = copy(dx, xlen, X, ldx, xlen, hipMemcpyHostToDevice);
    if (e == hipSuccess && y_in) e = copy(dy, ylen, Y, ldy, ylen, hipMemcpyHostToDevice);
    if (e == hipSuccess) e = launch_mul(img, opT, conj, K, dx, xlen, dy, ylen, alpha, beta, beta_strong_zero, st, gather, nullptr, il, vt);
    claim.mark();
    if (e == hipSuccess) e = copy(Y, ldy, dy, ylen, ylen, hipMemcpyDeviceToHost);
    if (e == hipSuccess) e = hipStreamSynchronize(st);
    if (e != hipSuccess) return hip_fail(e, K == 1 ? "host-staged mul" : "host-staged multi mul");
    return BSM_OK;
}

// The four product entry points: bsm_mul / bsm_mul_multi (multi: X and Y hold nrhs columns at ldx / ldy; else one
// packed column) and their _cvec forms (cplx: complex vectors under a real handle).  What a handle refuses complex
// vectors for is answered before anything that needs a device, so that analysis-only handles reach every answer.
static int mul_entry(bsm_matrix_s *A, int op, bool cplx, bool multi, int64_t nrhs, const void *X, int64_t ldx, void *Y,
                     int64_t ldy, const void *alpha, const void *beta, int beta_strong_zero, int memspace, void *stream) {
    if (!A) return fail(BSM_ERR_INVALID, "null handle");
    if (A->poly) return poly_mul(A, op, cplx, multi, nrhs, X, ldx, Y, ldy, alpha, beta, beta_strong_zero, memspace, (hipStream_t)stream);
    const int dt = A->an.dtype;
    if (cplx && (dt == BSM_C64 || dt == BSM_C128))
        return fail(BSM_ERR_INVALID, "complex handle: bsm_mul / bsm_mul_multi take its complex vectors");
    if (cplx && dt != BSM_F32 && dt != BSM_F64)
        return fail(BSM_ERR_UNSUPPORTED, "complex vectors under a mixed-storage handle are not supported");
    if (cplx && A->dist) return fail(BSM_ERR_UNSUPPORTED, "complex vectors under a multi-device handle are not supported");
    if (op < 0 || op > 2) return fail(BSM_ERR_INVALID, "bad op");
    if (cplx && memspace != BSM_MEM_HOST && memspace != BSM_MEM_DEVICE) return fail(BSM_ERR_INVALID, "bad memspace");
    if (nrhs < 0) return fail(BSM_ERR_INVALID, "negative nrhs");
    if (nrhs == 0) return BSM_OK;
    if (!X || !Y) return fail(BSM_ERR_INVALID, multi ? "null matrix" : "null vector");
    if (!A->on_device)
        return fail(BSM_ERR_DEVICE, "handle has no device image (created with BSM_DEVICE_NONE)");
    // (the whole operator's size: a multi-device handle has no image of its own)
    const long long xlen = (op == 0 ? A->an.ncols : A->an.nrows);
    const long long ylen = (op == 0 ? A->an.nrows : A->an.ncols);
    if (!multi) ldx = std::max<long long>(xlen, 1), ldy = std::max<long long>(ylen, 1);
    if (ldx < std::max<long long>(xlen, 1) || ldy < std::max<long long>(ylen, 1))
        return fail(BSM_ERR_INVALID, "leading dimension smaller than the vector length");
    // the vector type: the complex one of the handle's precision, or the handle's own (double / complex double under the
    // mixed storage codes)
    const int vt = cplx ? (dt == BSM_F32 ? BSM_C64 : BSM_C128) : vec_type(dt);
    return mul_k(A, op, nrhs, X, ldx, Y, ldy, alpha, beta, beta_strong_zero, memspace, (hipStream_t)stream, vt);
}

extern "C" int bsm_mul(bsm_matrix_t A, int op, const void *x, void *y, const void *alpha,
                       const void *beta, int beta_strong_zero, int memspace, void *stream) {
    return mul_entry(A, op, false, false, 1, x, 0, y, 0, alpha, beta, beta_strong_zero, memspace, stream);
}

extern "C" int bsm_mul_multi(bsm_matrix_t A, int op, int64_t nrhs, const void *X, int64_t ldx, void *Y,
                             int64_t ldy, const void *alpha, const void *beta, int beta_strong_zero,
                             int memspace, void *stream) {
    return mul_entry(A, op, false, true, nrhs, X, ldx, Y, ldy, alpha, beta, beta_strong_zero, memspace, stream);
}

extern "C" int bsm_mul_cvec(bsm_matrix_t A, int op, const void *x, void *y, const void *alpha, const void *beta,
                            int beta_strong_zero, int memspace, void *stream) {
    return mul_entry(A, op, true, false, 1, x, 0, y, 0, alpha, beta, beta_strong_zero, memspace, stream);
}

extern "C" int bsm_mul_multi_cvec(bsm_matrix_t A, int op, int64_t nrhs, const void *X, int64_t ldx, void *Y, int64_t ldy,
                                  const void *alpha, const void *beta, int beta_strong_zero, int memspace, void *stream) {
    return mul_entry(A, op, true, true, nrhs, X, ldx, Y, ldy, alpha, beta, beta_strong_zero, memspace, stream);
}

extern "C" int bsm_value_passes(bsm_matrix_t A, int64_t *count) {
    if (!A) return fail(BSM_ERR_INVALID, "null handle");
    if (!count) return fail(BSM_ERR_INVALID, "null count");
    if (int rc = poly_refusal(A, "bsm_value_passes")) return rc;
    if (A->dist) return fail(BSM_ERR_UNSUPPORTED, "bsm_value_passes: single-device handles only");
    *count = __atomic_load_n(&A->img.value_passes, __ATOMIC_RELAXED) + __atomic_load_n(&A->img_t.value_passes, __ATOMIC_RELAXED);
    return BSM_OK;
}

extern "C" int bsm_mul_parts(bsm_matrix_t A, int op, const void *const *x_parts, void *const *y_parts,
                             const void *alpha, const void *beta, int beta_strong_zero, void *const *streams) {
    if (!A) return fail(BSM_ERR_INVALID, "null handle");
    if (op < 0 || op > 2) return fail(BSM_ERR_INVALID, "bad op");
    if (!x_parts || !y_parts) return fail(BSM_ERR_INVALID, "null vector parts");
    if (int rc = poly_refusal(A, "bsm_mul_parts")) return rc;
    if (!A->dist) return fail(BSM_ERR_INVALID, "bsm_mul_parts needs a multi-device handle (bsm_options.ctx)");
    return dist_mul_parts(A, op, x_parts, y_parts, alpha, beta, beta_strong_zero, streams);
}

extern "C" int bsm_update_blocks(bsm_matrix_t A, int64_t nupd, const int64_t *ids, const void *const *blocks,
                                 const int64_t *ld, int memspace, void *stream) {
    BSM_GUARDED(
        if (!A) return fail(BSM_ERR_INVALID, "null handle");
        if (int rc = poly_refusal(A, "bsm_update_blocks")) return rc;
        if (is_mixed(A->an.dtype))
            return fail(BSM_ERR_UNSUPPORTED, "bsm_update_blocks: not available on a mixed-precision handle (BSM_F64_F32 / "
                                             "BSM_C128_C64); create a new handle from the new blocks");
        if (memspace != BSM_MEM_HOST && memspace != BSM_MEM_DEVICE) return fail(BSM_ERR_INVALID, "bad memspace");
        const int64_t nb = (int64_t)A->blk_m.size();
        if (nupd < 0 || nupd > nb) return fail(BSM_ERR_INVALID, "nupd out of range");
        if (!ids && nupd != nb) return fail(BSM_ERR_INVALID, "ids == NULL needs nupd == the number of blocks");
        if (nupd > 0 && (!blocks || !ld)) return fail(BSM_ERR_INVALID, "null argument");
        // every argument is checked before anything is written
        std::vector<int64_t> id0((size_t)nupd);
        std::vector<uint8_t> seen((size_t)nb, 0);
        bool in_order = true;
        for (int64_t k = 0; k < nupd; k++) {
            const int64_t id = ids ? ids[k] - 1 : k;
            if (id < 0 || id >= nb) return fail(BSM_ERR_INVALID, "update " + std::to_string(k + 1) + ": block id out of range");
            if (seen[id]) return fail(BSM_ERR_INVALID, "update " + std::to_string(k + 1) + ": duplicate block id");
            seen[id] = 1;
            in_order &= (id == k);
            id0[k] = id;
            const int64_t m = A->blk_m[id], n = A->blk_n[id];
            if (ld[k] < m || ld[k] < 1) return fail(BSM_ERR_INVALID, "update " + std::to_string(k + 1) + ": ld < m");
            if (!blocks[k] && m > 0 && n > 0) return fail(BSM_ERR_INVALID, "update " + std::to_string(k + 1) + ": null block");
        }
        if (nupd == 0) return BSM_OK;
        const bool full = in_order && nupd == nb;
        hipStream_t st = (hipStream_t)stream;
        std::lock_guard<std::mutex> lk(A->upd_mu);
        if (A->dist) return dist_update(A, nupd, id0.data(), full, blocks, ld, memspace, st);
        return A->refill(nupd, id0.data(), full, blocks, ld, memspace, st, A->blk_m, A->blk_n);)
}

static int copy_out(const std::vector<int64_t> &v, int64_t *out, int64_t *len) {
    if (!len) return fail(BSM_ERR_INVALID, "len is null");
    if (out) {
        if (*len < (int64_t)v.size()) return fail(BSM_ERR_INVALID, "output buffer too small");
        std::memcpy(out, v.data(), v.size() * sizeof(int64_t));
    }
    *len = (int64_t)v.size();
    return BSM_OK;
}

extern "C" int bsm_get_bookkeeping(bsm_matrix_t A, int which, int64_t *out, int64_t *len) {
    if (!A) return fail(BSM_ERR_INVALID, "null handle");
    if (int rc = poly_refusal(A, "bsm_get_bookkeeping")) return rc;
    const Analysis &an = A->an;
    switch (which) {
        case BSM_BK_VBCRS_PERM:
        case BSM_BK_VBCRS_ROWPTR:
        case BSM_BK_VBCRS_COLINDICES:
        case BSM_BK_VBCRS_ROWINDICES: {
            if (an.mtype != MT_VBCRS) return fail(BSM_ERR_INVALID, "not a VBCRS handle");
            const std::vector<int64_t> *v = which == BSM_BK_VBCRS_PERM         ? &an.perm
                                            : which == BSM_BK_VBCRS_ROWPTR     ? &an.rowptr
                                            : which == BSM_BK_VBCRS_COLINDICES ? &an.colindices
                                                                               : &an.rowindices;
            return copy_out(*v, out, len);
        }
        case BSM_BK_COLORS:
        case BSM_BK_TRANSPOSECOLORS:
        case BSM_BK_DIAGONALCOLORS: {
            if (an.mtype == MT_VBCRS) return fail(BSM_ERR_INVALID, "VBCRS has no colours");
            if (which == BSM_BK_DIAGONALCOLORS && an.mtype != MT_SYMMETRIC)
                return fail(BSM_ERR_INVALID, "not a symmetric handle");
            const auto &cs = an.colors[which - BSM_BK_COLORS];
            std::vector<int64_t> flat;
            flat.push_back((int64_t)cs.size());
            for (const auto &c : cs) {
                flat.push_back((int64_t)c.size());
                flat.insert(flat.end(), c.begin(), c.end());
            }
            return copy_out(flat, out, len);
        }
    }
    return fail(BSM_ERR_INVALID, "unknown bookkeeping id");
}

extern "C" int bsm_get_image(bsm_matrix_t A, int which, void *out, int64_t *nbytes) {
    if (!A || !nbytes) return fail(BSM_ERR_INVALID, "null argument");
    if (int rc = poly_refusal(A, "bsm_get_image")) return rc;
    if (A->on_device || A->dist) return fail(BSM_ERR_UNSUPPORTED, "image dump needs an analysis-only handle");
    if (which >= 16 && !A->has_t) return fail(BSM_ERR_INVALID, "handle has no transposed image");
    const Analysis &an = (which >= 16) ? A->an_t : A->an;
    which &= 15;
    const void *src = nullptr;
    size_t bytes = 0;
    switch (which) {
        case 0: src = an.values.data(); bytes = an.values.size(); break;
        case 1: src = an.rows.data(); bytes = an.rows.size() * 4; break;
        case 2: src = an.cols.data(); bytes = an.cols.size() * 4; break;
        case 3: src = an.waves.data(); bytes = an.waves.size() * sizeof(WaveWork); break;
        case 4: src = an.inv_ptr[0].data(); bytes = an.inv_ptr[0].size() * 8; break;
        case 5: src = an.inv_idx[0].data(); bytes = an.inv_idx[0].size() * 4; break;
        case 6: src = an.inv_ptr[1].data(); bytes = an.inv_ptr[1].size() * 8; break;
        case 7: src = an.inv_idx[1].data(); bytes = an.inv_idx[1].size() * 4; break;
        case 8: src = an.waves_multi.data(); bytes = an.waves_multi.size() * sizeof(WaveWork); break;
        default: return fail(BSM_ERR_INVALID, "unknown image array");
    }
    if (out) {
        if (*nbytes < (int64_t)bytes) return fail(BSM_ERR_INVALID, "output buffer too small");
        std::memcpy(out, src, bytes);
    }
    *nbytes = (int64_t)bytes;
    return BSM_OK;
}

// Developer probe (tools/placement_move.py; not declared in the public header): moves one array of a device image
// to a fresh allocation -- which = 0 values, 1 rows, 2 cols, 3 wave records -- to find out which one a handle's
// "placement level" depends on.
extern "C" int bsm_debug_move_image_array(bsm_matrix_t A, int which) {
    if (!A || !A->on_device || A->dist || A->poly) return fail(BSM_ERR_INVALID, "needs a single-device handle");
    DeviceGuard guard;
    hipError_t e = guard.enter(A->img.device);
    if (e != hipSuccess) return hip_fail(e, "hipSetDevice");
    void **slot = which == 0 ? &A->img.d_values : which == 1 ? &A->img.d_rows : which == 2 ? &A->img.d_cols : &A->img.d_waves;
    const size_t bytes = which == 0 ? (size_t)A->an.value_bytes
                         : which == 1 ? A->an.rows.size() * 4
                         : which == 2 ? A->an.cols.size() * 4
                                      : A->an.waves.size() * sizeof(WaveWork);
    if (!*slot || bytes == 0) return BSM_OK;
    void *fresh = nullptr;
    if ((e = hipDeviceSynchronize()) != hipSuccess) return hip_fail(e, "sync");
    if ((e = hipMalloc(&fresh, bytes)) != hipSuccess) return hip_fail(e, "hipMalloc");
    if ((e = hipMemcpy(fresh, *slot, bytes, hipMemcpyDeviceToDevice)) != hipSuccess) return hip_fail(e, "copy");
    (void)hipFree(*slot);
    *slot = fresh;
    if (std::getenv("BSM_PLACEMENT_DEBUG")) std::fprintf(stderr, "[bsm image] array %d now at %p (%zu B)\n", which, fresh, bytes);
    return BSM_OK;
}

extern "C" int bsm_stats(bsm_matrix_t A, bsm_stats_t *out) {
    if (!A || !out) return fail(BSM_ERR_INVALID, "null argument");
    std::memset(out, 0, sizeof *out);
    out->nnz = A->an.nnz;
    out->stored_entries = A->an.stored_entries;
    out->alg_bytes = A->an.alg_bytes;
    out->device_bytes = A->dist ? dist_device_bytes(A) : A->img.device_bytes + (A->has_t ? A->img_t.device_bytes : 0);
    out->npanels = A->an.ngroups;
    out->ntasks = (int64_t)A->an.waves.size();
    out->nworkgroups = A->img.nwg_total ? A->img.nwg_total : A->an.nwg_total;
    out->exclusive = A->img.exclusive_fwd ? 1 : 0;
    out->win_emissions = A->an.win_emissions;
    out->win_inside = A->an.win_inside;
    out->win_flushed = A->an.win_flushed;
    return BSM_OK;
}

extern "C" int bsm_color(int64_t nlists, const int64_t *const *lists, const int64_t *lens, int algorithm,
                         int64_t *color_out, int64_t *ncolors) {
    try {
        if (nlists < 0 || (nlists > 0 && (!lists || !lens || !color_out)) || !ncolors)
            return fail(BSM_ERR_INVALID, "null argument");
        std::vector<const int64_t *> lp((size_t)nlists);
        std::vector<int64_t> ln((size_t)nlists);
        for (int64_t b = 0; b < nlists; b++) {
            if (lens[b] < 0 || (lens[b] > 0 && !lists[b])) return fail(BSM_ERR_INVALID, "bad list");
            for (int64_t k = 0; k < lens[b]; k++)
                if (lists[b][k] < 1) return fail(BSM_ERR_INVALID, "indices are 1-based");
            lp[b] = lists[b];
            ln[b] = lens[b];
        }
        if (algorithm != BSM_COLOR_WORKSTREAM_DSATUR && algorithm != BSM_COLOR_DSATUR)
            return fail(BSM_ERR_INVALID, "unknown colouring algorithm");
        auto classes = algorithm == BSM_COLOR_DSATUR ? color_dsatur(lp, ln) : color_workstream_dsatur(lp, ln);
        for (size_t c = 0; c < classes.size(); c++)
            for (int64_t id : classes[c]) color_out[id - 1] = (int64_t)c;
        *ncolors = (int64_t)classes.size();
        return BSM_OK;
    } catch (const std::bad_alloc &) {
        return fail(BSM_ERR_ALLOC, "out of host memory");
    }
}

extern "C" int bsm_destroy(bsm_matrix_t A) {
    if (!A) return BSM_OK;
    dist_destroy(A);  // the parts of a multi-device handle, each on its device
    DeviceGuard guard;
    if (A->device != BSM_DEVICE_NONE) {
        (void)guard.enter(A->device);
        if (A->stage_x) (void)hipFree(A->stage_x);
        if (A->stage_y) (void)hipFree(A->stage_y);
        poly_release(A);  // a composed handle's workspace
    }
    A->release();
    delete A;
    return BSM_OK;
}
