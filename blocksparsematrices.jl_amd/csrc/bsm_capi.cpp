// bsm_capi.cpp -- the extern "C" surface of libbsmrocm.so (include/bsm_rocm.h).
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
#include "bsm_invert.h"

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
    if (o.ctx && (dtype == BSM_F64_F32 || dtype == BSM_C128_C64))
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

#define BSM_GUARDED(...)                                         \
    try {                                                        \
        __VA_ARGS__                                              \
    } catch (const std::bad_alloc &) {                           \
        return fail(BSM_ERR_ALLOC, "out of host memory");        \
    } catch (const std::exception &e) {                          \
        return fail(BSM_ERR_INVALID, e.what());                  \
    }

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
        // (what the fused fan-out kernels of bsm_dist.cpp rely on is that the access was ENABLED, not that it is
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

namespace {
// triples of one packed image -> device buffers of its device (orow / ocol int64, oval element type)
int export_image(const Analysis &an, const DeviceImage &img, void *orow, void *ocol, void *oval, hipStream_t st) {
    const long long nw = (long long)an.waves.size();
    std::vector<long long> off((size_t)nw + 1, 0);
    for (long long w = 0; w < nw; w++) {
        const WaveWork &W = an.waves[w];
        long long cnt = 0;
        if (W.work == WORK_PANEL && W.npieces > 0) {
            const Piece &P = W.first;
            long long noff = 0;
            if (P.xbase < 0) {
                if ((P.kind & 3) == KIND_OFF)
                    for (int32_t k = 0; k < P.ncols; k++) noff += an.cols[(size_t)P.col_off + k] >= 0;
            } else {
                const long long w1 = std::min<long long>(W.seg1_w, P.ncols), w2 = std::min<long long>(W.seg2_w, P.ncols);
                if ((P.kind & 3) == KIND_OFF) noff += w1;
                if (((P.kind >> 2) & 3) == KIND_OFF) noff += std::max<long long>(0, w2 - w1);
                if (((P.kind >> 4) & 3) == KIND_OFF) noff += std::max<long long>(0, P.ncols - w2);
            }
            cnt = (long long)W.m * (P.ncols + noff);
        }
        off[w + 1] = off[w] + cnt;
    }
    if (off[nw] != an.nnz) return fail(BSM_ERR_DEVICE, "rowcolvals: image / nnz mismatch");
    if (nw == 0 || an.nnz == 0) return BSM_OK;
    void *d_off = nullptr;
    hipError_t e = hipMalloc(&d_off, off.size() * sizeof(long long));
    if (e == hipSuccess) e = hipMemcpyAsync(d_off, off.data(), off.size() * sizeof(long long), hipMemcpyHostToDevice, st);
    if (e == hipSuccess)
        e = launch_export_coo(an.dtype, img.d_waves, nw, d_off, img.d_values, img.d_rows, img.d_cols, orow, ocol, oval, st);
    if (e == hipSuccess) e = hipStreamSynchronize(st);
    if (d_off) (void)hipFree(d_off);
    if (e != hipSuccess) return hip_fail(e, "rowcolvals");
    return BSM_OK;
}
}  // namespace

extern "C" int bsm_rowcolvals(bsm_matrix_t A, int64_t *rows, int64_t *cols, void *vals, int64_t *count,
                              int memspace, void *stream) {
    BSM_GUARDED(
        if (!A || !count) return fail(BSM_ERR_INVALID, "null argument");
        if (!rows || !cols || !vals) {
            *count = A->an.nnz;
            return BSM_OK;
        }
        if (*count < A->an.nnz) return fail(BSM_ERR_INVALID, "output buffers too small");
        if (!A->on_device) return fail(BSM_ERR_DEVICE, "handle has no device image (created with BSM_DEVICE_NONE)");
        if (memspace != BSM_MEM_HOST && memspace != BSM_MEM_DEVICE) return fail(BSM_ERR_INVALID, "bad memspace");
        const size_t es = (size_t)A->an.vs;  // the stored values leave widened to the vector type
        // one image per device part (a single one for ordinary handles); parts are written one after another
        std::vector<std::pair<const Analysis *, const DeviceImage *>> imgs;
        if (A->dist)
            dist_images(A, imgs);
        else
            imgs.emplace_back(&A->an, &A->img);
        int64_t done = 0;
        for (auto &pi : imgs) {
            const Analysis &an = *pi.first;
            const DeviceImage &img = *pi.second;
            const int64_t n = an.nnz;
            if (n == 0) continue;
            DeviceGuard g;
            hipError_t e = g.enter(img.device);
            if (e != hipSuccess) return hip_fail(e, "hipSetDevice");
            // staged through buffers on the image's device unless the caller's arrays already live there
            bool direct = false;
            if (memspace == BSM_MEM_DEVICE && !A->dist) direct = true;
            void *r = nullptr; void *c = nullptr; void *v = nullptr;
            if (direct) {
                r = rows + done;
                c = cols + done;
                v = (char *)vals + (size_t)done * es;
            } else {
                e = hipMalloc(&r, (size_t)n * 8);
                if (e == hipSuccess) e = hipMalloc(&c, (size_t)n * 8);
                if (e == hipSuccess) e = hipMalloc(&v, (size_t)n * es);
                if (e != hipSuccess) {
                    for (void *q : {r, c, v}) if (q) (void)hipFree(q);
                    return hip_fail(e, "rowcolvals staging");
                }
            }
            int rc = export_image(an, img, r, c, v, direct ? (hipStream_t)stream : nullptr);
            if (rc == BSM_OK && !direct) {
                e = hipMemcpy(rows + done, r, (size_t)n * 8, hipMemcpyDefault);
                if (e == hipSuccess) e = hipMemcpy(cols + done, c, (size_t)n * 8, hipMemcpyDefault);
                if (e == hipSuccess) e = hipMemcpy((char *)vals + (size_t)done * es, v, (size_t)n * es, hipMemcpyDefault);
                if (e != hipSuccess) rc = hip_fail(e, "rowcolvals copy");
            }
            if (!direct) for (void *q : {r, c, v}) (void)hipFree(q);
            if (rc != BSM_OK) return rc;
            done += n;
        }
        *count = done;
        return BSM_OK;)
}

// ---- bsm_submatrices / bsm_diag: entries of the operator read out of its image -------------------------------------------
namespace {
// one output window: ni x nj entries of the vector type at `out`, leading dimension ld (elements).  diag(A) is one
// window of min(nrows, ncols) x 1
struct Window {
    int64_t ni, nj, ld;
    void *out;
};
struct DevBuf {
    void *p = nullptr;
    ~DevBuf() {
        if (p) (void)hipFree(p);
    }
    hipError_t alloc(size_t bytes) { return hipMalloc(&p, bytes ? bytes : 16); }
};
int vector_code(int dtype) { return dtype == BSM_F64_F32 ? BSM_F64 : dtype == BSM_C128_C64 ? BSM_C128 : dtype; }

// The host image of an analysis-only handle, by a plain loop over the wave records the kernel walks (bsm_extract.hip:
// same decode, same conditions, same addresses).  R / RS: real type of the vector / stored type, NC: 2 for complex.
// maps: rset, rpos (nrows each), cset, cpos (ncols each); null: diag(A) into win[0].  The windows are zero beforehand.
template <typename R, typename RS, int NC>
void extract_host(const Analysis &an, const int32_t *maps, const std::vector<Window> &win, bool opT, bool conj) {
    const int32_t *rset = maps, *rpos = maps ? maps + an.nrows : nullptr;
    const int32_t *cset = maps ? maps + 2 * an.nrows : nullptr, *cpos = maps ? maps + 2 * an.nrows + an.ncols : nullptr;
    auto add = [&](void *base, int64_t idx, const RS *v) {
        R *p = (R *)base + idx * NC;
        p[0] += (R)v[0];
        if (NC == 2) p[NC - 1] += conj ? -(R)v[NC - 1] : (R)v[NC - 1];
    };
    const int E = an.E;
    for (const WaveWork &W : an.waves) {
        if (W.work != WORK_PANEL || W.npieces == 0) continue;
        const Piece &P = W.first;
        const int64_t m = W.m;
        const RS *vb = (const RS *)(an.values.data() + P.val_off * 16);
        for (int32_t w = 0; w < P.ncols; w++) {
            bool off;
            int64_t ci;
            if (P.xbase < 0) {
                const int32_t raw = an.cols[(size_t)P.col_off + w];
                off = raw >= 0 && (P.kind & 3) == KIND_OFF;
                ci = raw & 0x7fffffff;
            } else {
                const int sh = w < W.seg1_w ? 0 : (w < W.seg2_w ? 2 : 4);
                off = ((P.kind >> sh) & 3) == KIND_OFF;
                ci = w < W.seg1_w ? P.xbase + w : (w < W.seg2_w ? W.seg1_x + (w - W.seg1_w) : P.seg2_x + (w - W.seg2_w));
            }
            const int64_t s = w / E, e = w % E;
            for (int64_t i = 0; i < m; i++) {
                const int64_t ri = (W.rbase >= 0) ? (int64_t)W.rbase + i : an.rows[(size_t)W.row_off + i];
                const RS *v = vb + ((s * m + i) * E + e) * NC;
                if (!maps) {
                    if (ri == ci) {
                        add(win[0].out, ri, v);
                        if (off) add(win[0].out, ri, v);
                    }
                    continue;
                }
                const int32_t fs = rset[ri];
                if (fs >= 0 && cset[ci] == fs) {
                    const Window &o = win[(size_t)fs];
                    add(o.out, opT ? cpos[ci] + o.ld * rpos[ri] : rpos[ri] + o.ld * cpos[ci], v);
                }
                if (off && ci < an.nrows && ri < an.ncols) {  // the transposed copy sits at (ci, ri)
                    const int32_t us = rset[ci];
                    if (us >= 0 && cset[ri] == us) {
                        const Window &o = win[(size_t)us];
                        add(o.out, opT ? cpos[ri] + o.ld * rpos[ci] : rpos[ci] + o.ld * cpos[ri], v);
                    }
                }
            }
        }
    }
}

// one packed image -> windows in the memory of its device (current): uploads the maps and the table of windows, zeroes
// the windows when `shape` says which they are, runs the kernel on `st` and waits for it
int extract_image(const Analysis &an, const DeviceImage &img, const std::vector<int32_t> *maps, const std::vector<ExtractOut> &table,
                  const std::vector<long long> *shape, void *d_diag, bool opT, bool conj, hipStream_t st) {
    // one allocation: the maps, behind them the table of windows and their shapes (16-byte aligned)
    DevBuf db;
    ExtractMaps mp{nullptr, nullptr, nullptr, nullptr};
    void *d_table = nullptr;
    hipError_t e = hipSuccess;
    if (maps) {
        const size_t mb = (maps->size() * 4 + 15) / 16 * 16, tb = table.size() * sizeof(ExtractOut);
        e = db.alloc(mb + tb + (shape ? shape->size() * 8 : 0));
        if (e == hipSuccess) e = hipMemcpyAsync(db.p, maps->data(), maps->size() * 4, hipMemcpyHostToDevice, st);
        d_table = (char *)db.p + mb;
        if (e == hipSuccess && !table.empty()) e = hipMemcpyAsync(d_table, table.data(), tb, hipMemcpyHostToDevice, st);
        const int *b = (const int *)db.p;
        mp = ExtractMaps{b, b + an.nrows, b + 2 * an.nrows, b + 2 * an.nrows + an.ncols};
        if (e == hipSuccess && shape) {
            long long largest = 0;
            for (size_t s = 0; s < table.size(); s++) largest = std::max(largest, (*shape)[2 * s] * (*shape)[2 * s + 1]);
            void *d_shape = (char *)d_table + tb;
            if (!shape->empty()) e = hipMemcpyAsync(d_shape, shape->data(), shape->size() * 8, hipMemcpyHostToDevice, st);
            if (e == hipSuccess)
                e = launch_zero_windows(vector_code(an.dtype), d_table, d_shape, (long long)table.size(), largest, st);
        }
    }
    if (e == hipSuccess)
        e = launch_extract(an.dtype, img.d_waves, (long long)an.waves.size(), img.d_values, img.d_rows, img.d_cols,
                           maps ? &mp : nullptr, d_table, d_diag, an.nrows, an.ncols, opT, conj, st);
    if (e == hipSuccess) e = hipStreamSynchronize(st);
    if (e != hipSuccess) return hip_fail(e, "extract");
    return BSM_OK;
}

// the checked request (maps == nullptr: diag(A), win[0] = d) on whatever the handle is made of
int extract_run(bsm_matrix_s *A, int op, const std::vector<int32_t> *maps, const std::vector<Window> &win, int memspace,
                hipStream_t stream) {
    const Analysis &an0 = A->an;
    const size_t vs = (size_t)an0.vs;
    const int vt = vector_code(an0.dtype);
    const bool opT = op != BSM_OP_N, conj = op == BSM_OP_C;
    if (!A->on_device) {  // analysis-only handle, host windows: zeroed, then summed
        for (const Window &w : win)
            for (int64_t b = 0; b < w.nj; b++) std::memset((char *)w.out + (size_t)(b * w.ld) * vs, 0, (size_t)w.ni * vs);
        const int32_t *mp = maps ? maps->data() : nullptr;
        switch (an0.dtype) {
            case BSM_F32: extract_host<float, float, 1>(an0, mp, win, opT, conj); break;
            case BSM_F64: extract_host<double, double, 1>(an0, mp, win, opT, conj); break;
            case BSM_C64: extract_host<float, float, 2>(an0, mp, win, opT, conj); break;
            case BSM_C128: extract_host<double, double, 2>(an0, mp, win, opT, conj); break;
            case BSM_F64_F32: extract_host<double, float, 1>(an0, mp, win, opT, conj); break;
            case BSM_C128_C64: extract_host<double, float, 2>(an0, mp, win, opT, conj); break;
            default: return fail(BSM_ERR_INVALID, "bad dtype");
        }
        return BSM_OK;
    }
    if (memspace == BSM_MEM_DEVICE && !A->dist) {  // straight into the caller's windows
        DeviceGuard g;
        hipError_t e = g.enter(A->img.device);
        if (e != hipSuccess) return hip_fail(e, "hipSetDevice");
        if (!maps) {
            if (win[0].ni == 0) return BSM_OK;
            e = hipMemsetAsync(win[0].out, 0, (size_t)win[0].ni * vs, stream);
            if (e != hipSuccess) return hip_fail(e, "hipMemsetAsync");
            return extract_image(A->an, A->img, nullptr, {}, nullptr, win[0].out, opT, conj, stream);
        }
        std::vector<ExtractOut> table(win.size());
        std::vector<long long> shape(2 * win.size());
        for (size_t s = 0; s < win.size(); s++) {
            table[s] = ExtractOut{(uint64_t)(uintptr_t)win[s].out, (long long)win[s].ld};
            shape[2 * s] = win[s].ni;
            shape[2 * s + 1] = win[s].nj;
        }
        return extract_image(A->an, A->img, maps, table, &shape, nullptr, opT, conj, stream);
    }
    // host windows, or a multi-device handle: every image adds into a zeroed, compact staging buffer on its own device;
    // the buffers come back to the host, are summed there (an entry lives in exactly one part) and delivered
    std::vector<size_t> off(win.size() + 1, 0);
    for (size_t s = 0; s < win.size(); s++) off[s + 1] = off[s] + (size_t)win[s].ni * (size_t)win[s].nj;
    const size_t total = off[win.size()];
    if (total == 0) return BSM_OK;
    std::vector<std::pair<const Analysis *, const DeviceImage *>> imgs;
    if (A->dist)
        dist_images(A, imgs);
    else
        imgs.emplace_back(&A->an, &A->img);
    std::vector<char> sum(total * vs, 0), part;
    bool first = true;
    for (auto &pi : imgs) {
        DeviceGuard g;
        hipError_t e = g.enter(pi.second->device);
        if (e != hipSuccess) return hip_fail(e, "hipSetDevice");
        DevBuf stg;
        e = stg.alloc(total * vs);
        if (e == hipSuccess) e = hipMemsetAsync(stg.p, 0, total * vs, nullptr);
        if (e != hipSuccess) return hip_fail(e, "extract staging");
        std::vector<ExtractOut> table(maps ? win.size() : 0);
        for (size_t s = 0; s < table.size(); s++)
            table[s] = ExtractOut{(uint64_t)(uintptr_t)((char *)stg.p + off[s] * vs), (long long)std::max<int64_t>(win[s].ni, 1)};
        const int rc = extract_image(*pi.first, *pi.second, maps, table, nullptr, stg.p, opT, conj, nullptr);
        if (rc != BSM_OK) return rc;
        std::vector<char> &dst = first ? sum : part;
        dst.resize(total * vs);
        e = hipMemcpy(dst.data(), stg.p, total * vs, hipMemcpyDeviceToHost);
        if (e != hipSuccess) return hip_fail(e, "extract copy");
        if (!first) {
            if (vt == BSM_F32 || vt == BSM_C64) {
                float *a = (float *)sum.data();
                const float *b = (const float *)part.data();
                for (size_t k = 0; k < total * vs / 4; k++) a[k] += b[k];
            } else {
                double *a = (double *)sum.data();
                const double *b = (const double *)part.data();
                for (size_t k = 0; k < total * vs / 8; k++) a[k] += b[k];
            }
        }
        first = false;
    }
    for (size_t s = 0; s < win.size(); s++) {
        const Window &w = win[s];
        if (w.ni == 0 || w.nj == 0) continue;
        const char *src = sum.data() + off[s] * vs;
        if (memspace == BSM_MEM_HOST) {
            for (int64_t b = 0; b < w.nj; b++)
                std::memcpy((char *)w.out + (size_t)(b * w.ld) * vs, src + (size_t)(b * w.ni) * vs, (size_t)w.ni * vs);
        } else {
            const hipError_t e = hipMemcpy2D(w.out, (size_t)w.ld * vs, src, (size_t)w.ni * vs, (size_t)w.ni * vs, (size_t)w.nj,
                                             hipMemcpyHostToDevice);
            if (e != hipSuccess) return hip_fail(e, "extract delivery");
        }
    }
    return BSM_OK;
}
}  // namespace

extern "C" int bsm_submatrices(bsm_matrix_t A, int op, int64_t nsets, const int64_t *const *I, const int64_t *ni,
                               const int64_t *const *J, const int64_t *nj, void *const *out, const int64_t *ldo, int memspace,
                               void *stream) {
    BSM_GUARDED(
        if (!A) return fail(BSM_ERR_INVALID, "null handle");
        if (op != BSM_OP_N && op != BSM_OP_T && op != BSM_OP_C) return fail(BSM_ERR_INVALID, "bad op");
        if (memspace != BSM_MEM_HOST && memspace != BSM_MEM_DEVICE) return fail(BSM_ERR_INVALID, "bad memspace");
        if (memspace == BSM_MEM_DEVICE && !A->on_device)
            return fail(BSM_ERR_INVALID, "BSM_MEM_DEVICE windows need a device image (handle created with BSM_DEVICE_NONE)");
        if (nsets < 0 || nsets > INT32_MAX) return fail(BSM_ERR_INVALID, "bad number of sets");
        if (nsets > 0 && (!I || !ni || !J || !nj || !out || !ldo)) return fail(BSM_ERR_INVALID, "null argument");
        const Analysis &an = A->an;
        if (an.nrows > INT32_MAX || an.ncols > INT32_MAX) return fail(BSM_ERR_UNSUPPORTED, "operator too large for int32 maps");
        // the four maps over the rows and columns of the STORED operator: I indexes the rows of op(A), i.e. the columns
        // of A for op T / C.  Filling them is the duplicate check: an index is written once.
        std::vector<int32_t> maps((size_t)(2 * an.nrows + 2 * an.ncols), 0);
        int32_t *rset = maps.data(), *rpos = rset + an.nrows, *cset = rpos + an.nrows, *cpos = cset + an.ncols;
        std::fill(rset, rset + an.nrows, -1);
        std::fill(cset, cset + an.ncols, -1);
        const bool opT = op != BSM_OP_N;
        std::vector<Window> win((size_t)nsets);
        for (int64_t s = 0; s < nsets; s++) {
            const std::string set = "set " + std::to_string(s + 1) + ": ";
            if (ni[s] < 0 || nj[s] < 0 || ni[s] > INT32_MAX || nj[s] > INT32_MAX) return fail(BSM_ERR_INVALID, set + "bad size");
            if ((ni[s] > 0 && !I[s]) || (nj[s] > 0 && !J[s])) return fail(BSM_ERR_INVALID, set + "null index list");
            if (ldo[s] < std::max<int64_t>(ni[s], 1)) return fail(BSM_ERR_INVALID, set + "ldo < max(ni, 1)");
            if (ni[s] > 0 && nj[s] > 0 && !out[s]) return fail(BSM_ERR_INVALID, set + "null output window");
            for (int side = 0; side < 2; side++) {
                const int64_t *idx = side ? J[s] : I[s];
                const int64_t cnt = side ? nj[s] : ni[s];
                const bool stored_rows = (side == 0) != opT;  // this list names rows of the stored operator
                const int64_t dim = stored_rows ? an.nrows : an.ncols;
                int32_t *sm = stored_rows ? rset : cset, *pm = stored_rows ? rpos : cpos;
                for (int64_t k = 0; k < cnt; k++) {
                    const int64_t v = idx[k];
                    if (v < 1 || v > dim)
                        return fail(BSM_ERR_INVALID, set + (side ? "column" : "row") + " index " + std::to_string(v) + " outside 1.." + std::to_string(dim));
                    if (sm[v - 1] >= 0)
                        return fail(BSM_ERR_INVALID, set + (side ? "column" : "row") + " index " + std::to_string(v) +
                                                         " is listed twice (the sets must be disjoint and free of repeats)");
                    sm[v - 1] = (int32_t)s;
                    pm[v - 1] = (int32_t)k;
                }
            }
            win[(size_t)s] = Window{ni[s], nj[s], ldo[s], out[s]};
        }
        if (nsets == 0) return BSM_OK;
        return extract_run(A, op, &maps, win, memspace, (hipStream_t)stream);)
}

extern "C" int bsm_diag(bsm_matrix_t A, void *d, int memspace, void *stream) {
    BSM_GUARDED(
        if (!A) return fail(BSM_ERR_INVALID, "null handle");
        if (memspace != BSM_MEM_HOST && memspace != BSM_MEM_DEVICE) return fail(BSM_ERR_INVALID, "bad memspace");
        if (memspace == BSM_MEM_DEVICE && !A->on_device)
            return fail(BSM_ERR_INVALID, "a BSM_MEM_DEVICE result needs a device image (handle created with BSM_DEVICE_NONE)");
        const int64_t n = std::min(A->an.nrows, A->an.ncols);
        if (n > 0 && !d) return fail(BSM_ERR_INVALID, "d is null");
        if (n == 0) return BSM_OK;
        const std::vector<Window> win{Window{n, 1, n, d}};
        return extract_run(A, BSM_OP_N, nullptr, win, memspace, (hipStream_t)stream);)
}

// ---- bsm_invert_blocks: batched in-place inverse of dense blocks ---------------------------------------------------------
namespace {
// the device leg: the non-empty blocks sorted by descending order (the large ones start first), cut into launches of
// one regime whose blocks need more than half the LDS of the launch's first -- a 16 x 16 block does not reserve the
// LDS of the 128 x 128 one that came in the same call
int invert_device(int dtype, int64_t nblocks, void *const *blocks, const int64_t *n, const int64_t *ld, int64_t *info,
                  hipStream_t stream) {
    const int es = dtype == BSM_F32 ? 4 : dtype == BSM_C128 ? 16 : 8;
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
        if (dtype == BSM_F64_F32 || dtype == BSM_C128_C64)
            return fail(BSM_ERR_INVALID, "bsm_invert_blocks takes a vector type (BSM_F32 .. BSM_C128), not a mixed storage code");
        if (dtype < 0 || dtype > 3) return fail(BSM_ERR_INVALID, "bad dtype");
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
        for (int64_t b = 0; b < nblocks; b++) {
            int rc = 0;
            switch (dtype) {
                case BSM_F32: rc = invert_block_host<float, 1>((float *)blocks[b], n[b], ld[b]); break;
                case BSM_F64: rc = invert_block_host<double, 1>((double *)blocks[b], n[b], ld[b]); break;
                case BSM_C64: rc = invert_block_host<float, 2>((float *)blocks[b], n[b], ld[b]); break;
                default: rc = invert_block_host<double, 2>((double *)blocks[b], n[b], ld[b]); break;
            }
            if (info) info[b] = rc;
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
    if (dtype == BSM_F64_F32 || dtype == BSM_C128_C64)
        return fail(BSM_ERR_INVALID, "bsm_vec_add_segments takes a vector type (BSM_F32 .. BSM_C128), not a mixed storage code");
    if (dtype < 0 || dtype > 3) return fail(BSM_ERR_INVALID, "bad dtype");
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
    const size_t es = vt == BSM_F32 ? 4 : vt == BSM_C128 ? 16 : 8;
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
    static const int kVecType[6] = {BSM_F32, BSM_F64, BSM_C64, BSM_C128, BSM_F64, BSM_C128};
    const int vt = cplx ? (dt == BSM_F32 ? BSM_C64 : BSM_C128) : kVecType[dt];
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
    if (A->dist) return fail(BSM_ERR_UNSUPPORTED, "bsm_value_passes: single-device handles only");
    *count = __atomic_load_n(&A->img.value_passes, __ATOMIC_RELAXED) + __atomic_load_n(&A->img_t.value_passes, __ATOMIC_RELAXED);
    return BSM_OK;
}

extern "C" int bsm_mul_parts(bsm_matrix_t A, int op, const void *const *x_parts, void *const *y_parts,
                             const void *alpha, const void *beta, int beta_strong_zero, void *const *streams) {
    if (!A) return fail(BSM_ERR_INVALID, "null handle");
    if (op < 0 || op > 2) return fail(BSM_ERR_INVALID, "bad op");
    if (!x_parts || !y_parts) return fail(BSM_ERR_INVALID, "null vector parts");
    if (!A->dist) return fail(BSM_ERR_INVALID, "bsm_mul_parts needs a multi-device handle (bsm_options.ctx)");
    return dist_mul_parts(A, op, x_parts, y_parts, alpha, beta, beta_strong_zero, streams);
}

extern "C" int bsm_update_blocks(bsm_matrix_t A, int64_t nupd, const int64_t *ids, const void *const *blocks,
                                 const int64_t *ld, int memspace, void *stream) {
    BSM_GUARDED(
        if (!A) return fail(BSM_ERR_INVALID, "null handle");
        if (A->an.dtype == BSM_F64_F32 || A->an.dtype == BSM_C128_C64)
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
    if (!A || !A->on_device || A->dist) return fail(BSM_ERR_INVALID, "needs a single-device handle");
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
    }
    A->release();
    delete A;
    return BSM_OK;
}
