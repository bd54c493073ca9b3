// bsm_operator.cpp -- LocalOperator (bsm_internal.h): a packed operator on one device.  Its three life-cycle steps --
// build (analysis, packing, upload), refill (bsm_update_blocks) and release -- for single-device handles (bsm_capi.cpp)
// and for every part of a multi-device handle (bsm_dist.cpp) alike.  Not part of the C ABI.
#include <hip/hip_runtime_api.h>

#include <algorithm>
#include <climits>
#include <cstdlib>
#include <cstring>
#include <mutex>
#include <string>
#include <vector>

#include "bsm_internal.h"

namespace bsm {

namespace {

template <typename V> hipError_t upload(const V &v, void **dptr, long long &total) {
    const size_t bytes = v.size() * sizeof(decltype(v[0]));
    hipError_t e = hipMalloc(dptr, bytes ? bytes : 16);
    if (e != hipSuccess) return e;
    total += (long long)bytes;
    if (bytes) e = hipMemcpy(*dptr, v.data(), bytes, hipMemcpyHostToDevice);
    return e;
}

// Streams the packed values to the device while they are being packed: two pinned staging windows
// (kept for the life of the process: pinning 2 x 64 MiB costs more than packing a C2-sized operator)
// and asynchronous copies on a private stream.  Small operators decline and take the one-shot path.
struct PinnedPool {
    std::mutex mu;  // one streamed create at a time per process
    char *buf[2] = {nullptr, nullptr};
    size_t cap[2] = {0, 0};
};
PinnedPool g_pool;
size_t stream_min_bytes() {  // BSM_STREAM_MIN_BYTES: smaller operators take the one-shot upload
    const char *e = std::getenv("BSM_STREAM_MIN_BYTES");
    return (e && *e) ? (size_t)std::strtoull(e, nullptr, 10) : ((size_t)128 << 20);
}

struct DeviceSink : ValueSink {
    void **dptr;
    std::unique_lock<std::mutex> lock;
    hipStream_t st = nullptr;
    hipEvent_t ev[2] = {nullptr, nullptr};
    bool pending[2] = {false, false};
    int k = 0;
    bool active = false;
    explicit DeviceSink(void **d) : dptr(d) {}
    static std::string msg(hipError_t e, const char *what) { return std::string(what) + ": " + hipGetErrorString(e); }
    std::string begin(size_t total, bool *use) override {
        *use = false;
        if (total == 0 || total < stream_min_bytes()) return "";
        lock = std::unique_lock<std::mutex>(g_pool.mu);
        hipError_t e = hipMalloc(dptr, total);
        if (e != hipSuccess) return msg(e, "hipMalloc(values)");
        e = hipStreamCreateWithFlags(&st, hipStreamNonBlocking);
        for (int i = 0; i < 2 && e == hipSuccess; i++) e = hipEventCreateWithFlags(&ev[i], hipEventDisableTiming);
        if (e != hipSuccess) return msg(e, "upload stream");
        active = *use = true;
        return "";
    }
    char *window(size_t bytes) override {
        const int i = k & 1;
        if (pending[i]) {
            if (hipEventSynchronize(ev[i]) != hipSuccess) return nullptr;
            pending[i] = false;
        }
        if (g_pool.cap[i] < bytes) {
            if (g_pool.buf[i]) (void)hipHostFree(g_pool.buf[i]);
            g_pool.buf[i] = nullptr;
            g_pool.cap[i] = 0;
            const size_t want = std::max<size_t>(bytes, 64u << 20);
            if (hipHostMalloc((void **)&g_pool.buf[i], want, hipHostMallocDefault) != hipSuccess) return nullptr;
            g_pool.cap[i] = want;
        }
        return g_pool.buf[i];
    }
    std::string commit(size_t offset, size_t bytes) override {
        const int i = k & 1;
        hipError_t e = hipMemcpyAsync((char *)*dptr + offset, g_pool.buf[i], bytes, hipMemcpyHostToDevice, st);
        if (e == hipSuccess) e = hipEventRecord(ev[i], st);
        if (e != hipSuccess) return msg(e, "streamed upload");
        pending[i] = true;
        k++;
        return "";
    }
    std::string end() override {
        hipError_t e = hipStreamSynchronize(st);
        pending[0] = pending[1] = false;
        if (lock.owns_lock()) lock.unlock();  // the staging windows are free for the next create
        return e == hipSuccess ? "" : msg(e, "streamed upload");
    }
    ~DeviceSink() override {
        if (st) {
            (void)hipStreamSynchronize(st);  // the staging buffers go back to the pool idle
            (void)hipStreamDestroy(st);
        }
        for (auto &e : ev)
            if (e) (void)hipEventDestroy(e);
    }
};

void free_image(DeviceImage &img) {
    for (void **p : {&img.d_values, &img.d_rows, &img.d_cols, &img.d_waves, &img.d_waves_multi, &img.d_ws, &img.d_wsc, &img.d_inv_ptr[0],
                     &img.d_inv_ptr[1], &img.d_inv_idx[0], &img.d_inv_idx[1]}) {
        if (*p) (void)hipFree(*p);
        *p = nullptr;
    }
}

void fill_image(const Analysis &an, const bsm_options &o, bool use_own, DeviceImage &img) {
    img.dtype = an.dtype;
    img.nrows = an.nrows;
    img.ncols = an.ncols;
    img.own_lo = (use_own && o.own_lo > 0) ? o.own_lo - 1 : 0;
    img.own_hi = (use_own && o.own_hi > 0) ? std::min<long long>(o.own_hi, an.nrows) : an.nrows;
    img.value_bytes = an.value_bytes;
    img.nwg_main = an.nwg_main;
    img.nwg_total = an.nwg_total;
    img.nwg_multi = an.nwg_multi;
    img.lane_fill = (float)an.lane_fill;
    img.mean_rows = (float)an.mean_rows;
    img.exclusive_fwd = an.exclusive_fwd && (o.accumulate == BSM_ACC_AUTO || o.accumulate == BSM_ACC_DIRECT);
    img.has_off = false;
    img.max_rows = 1;
    for (const WaveWork &w : an.waves)
        if (w.work == WORK_PANEL && w.npieces > 0) {
            if (w.first.kind & kKindHasOff) img.has_off = true;
            img.max_rows = std::max(img.max_rows, (int)w.m);
        }
    if (!img.exclusive_fwd) img.nwg_total = img.nwg_main;
    img.color_wg_ptr.assign(an.color_wg_ptr.begin(), an.color_wg_ptr.end());
    img.device_bytes = (long long)((size_t)an.value_bytes + an.rows.size() * 4 + an.cols.size() * 4 +
                                   (an.waves.size() + an.waves_multi.size()) * sizeof(WaveWork));
    if (an.gather)
        img.device_bytes += (long long)((an.ws_slots + 8) * an.vs + (an.inv_ptr[0].size() + an.inv_ptr[1].size()) * 8 +
                                        (an.inv_idx[0].size() + an.inv_idx[1].size()) * 4);
}

hipError_t upload_image(Analysis &an, DeviceImage &img, int dev) {
    img.device = dev;
    long long total = 0;
    hipError_t e = hipSuccess;
    if (img.d_values)  // the packer streamed them (DeviceSink)
        total += an.value_bytes;
    else
        e = upload(an.values, &img.d_values, total);
    if (e == hipSuccess) e = upload(an.rows, &img.d_rows, total);
    if (e == hipSuccess) e = upload(an.cols, &img.d_cols, total);
    if (e == hipSuccess) e = upload(an.waves, &img.d_waves, total);
    if (e == hipSuccess && !an.waves_multi.empty()) e = upload(an.waves_multi, &img.d_waves_multi, total);
    if (e == hipSuccess && an.gather) {
        img.ws_fbase = an.ws_fbase;
        for (int k = 0; k < 2 && e == hipSuccess; k++) {
            e = upload(an.inv_ptr[k], &img.d_inv_ptr[k], total);
            if (e == hipSuccess) e = upload(an.inv_idx[k], &img.d_inv_idx[k], total);
        }
        if (e == hipSuccess) {
            const size_t wsb = (size_t)(an.ws_slots + 8) * (size_t)an.vs;  // sums: vector type
            e = hipMalloc(&img.d_ws, wsb);
            if (e == hipSuccess) e = hipMemset(img.d_ws, 0, wsb);
            total += (long long)wsb;
        }
    }
    if (e == hipSuccess) an.values.release();  // packed host copy no longer needed
    if (std::getenv("BSM_PLACEMENT_DEBUG") && e == hipSuccess && an.value_bytes >= (64 << 20)) {
        // developer probe (tools/placement_which.py): where the image landed, and what a BARE streaming read of its
        // value stream takes there
        void *sink = nullptr;
        hipEvent_t a, b;
        float ms = 0.f;
        if (hipMalloc(&sink, 8192) == hipSuccess && hipEventCreate(&a) == hipSuccess && hipEventCreate(&b) == hipSuccess) {
            for (int r = 0; r < 3; r++) (void)launch_stream_floor(img.d_values, an.value_bytes / 16 * 16, sink, nullptr, nullptr);
            (void)hipEventRecord(a, nullptr);
            for (int r = 0; r < 10; r++) (void)launch_stream_floor(img.d_values, an.value_bytes / 16 * 16, sink, nullptr, nullptr);
            (void)hipEventRecord(b, nullptr);
            (void)hipEventSynchronize(b);
            (void)hipEventElapsedTime(&ms, a, b);
            (void)hipEventDestroy(a);
            (void)hipEventDestroy(b);
            (void)hipFree(sink);
        }
        std::fprintf(stderr, "[bsm image] values %p (%lld B) bare stream %.1f us | rows %p cols %p waves %p (%zu)\n", img.d_values,
                     (long long)an.value_bytes, ms * 100.f, img.d_rows, img.d_cols, img.d_waves, an.waves.size());
    }
    return e;
}

// Second ordering: the transposed operator as a forward image (rows <-> columns, blocks read
// transposed by the packer).  Built from the same caller arrays, before they are released.
std::vector<BlockIn> transposed_blocks(const std::vector<BlockIn> &in) {
    std::vector<BlockIn> t(in.size());
    for (size_t b = 0; b < in.size(); b++) {
        const BlockIn &B = in[b];
        BlockIn &Tb = t[b];
        Tb.data = B.data;
        Tb.m = B.n;
        Tb.n = B.m;
        Tb.ld = B.ld;
        Tb.ridx = B.cidx;
        Tb.cidx = B.ridx;
        Tb.r0 = B.c0;
        Tb.c0 = B.r0;
        Tb.kind = KIND_PLAIN;
        Tb.trans = !B.trans;
    }
    return t;
}

AnalysisOptions transpose_aopt(const bsm_options &o) {
    AnalysisOptions a;
    a.scheduler = 0;
    a.accumulate = o.accumulate;
    a.blocks_on_device = (o.blocks_memspace == BSM_MEM_DEVICE);
    return a;
}

// Executes the pack plan of an analysis built with blocks_on_device on the CURRENT device: the
// strip-packed value stream is written by a kernel straight from the caller's device blocks.
hipError_t device_pack(Analysis &an, void **d_values) {
    hipError_t e = hipMalloc(d_values, (size_t)std::max<int64_t>(an.value_bytes, 16));
    if (e == hipSuccess && std::getenv("BSM_TIMING"))
        std::fprintf(stderr, "[bsm] values at %p (%lld bytes)\n", *d_values, (long long)an.value_bytes);
    if (e != hipSuccess) return e;
    e = hipMemsetAsync(*d_values, 0, (size_t)std::max<int64_t>(an.value_bytes, 16), nullptr);  // strip tails
    void *d_plan = nullptr, *d_cp = nullptr;
    if (e == hipSuccess && !an.pack_plan.empty()) {
        e = hipMalloc(&d_plan, an.pack_plan.size() * sizeof(PackChunk));
        if (e == hipSuccess)
            e = hipMemcpyAsync(d_plan, an.pack_plan.data(), an.pack_plan.size() * sizeof(PackChunk),
                               hipMemcpyHostToDevice, nullptr);
        if (e == hipSuccess && !an.pack_colpos.empty()) {
            e = hipMalloc(&d_cp, an.pack_colpos.size() * 4);
            if (e == hipSuccess)
                e = hipMemcpyAsync(d_cp, an.pack_colpos.data(), an.pack_colpos.size() * 4, hipMemcpyHostToDevice, nullptr);
        }
        if (e == hipSuccess) e = launch_pack(an.es, an.vs, d_plan, (long long)an.pack_plan.size(), d_cp, *d_values, nullptr);
    }
    if (e == hipSuccess) e = hipStreamSynchronize(nullptr);
    if (d_plan) (void)hipFree(d_plan);
    if (d_cp) (void)hipFree(d_cp);
    an.pack_plan.clear();
    an.pack_plan.shrink_to_fit();
    an.pack_colpos.clear();
    an.pack_colpos.shrink_to_fit();
    return e;
}

// ---- bsm_update_blocks ------------------------------------------------------------------------------------------
void il_free(ILWork &il) {
    if (il.xr) (void)hipFree(il.xr);
    if (il.w) (void)hipFree(il.w);
    il = ILWork{};
}

void update_free(UpdateState &U) {
    if (U.pending && U.ev_done) (void)hipEventSynchronize(U.ev_done);
    for (RefillDevice &R : U.img)
        for (void **p : {&R.d_chunks, &R.d_colpos, &R.d_segs, &R.d_items_all, &R.d_items_id}) {
            if (*p) (void)hipFree(*p);
            *p = nullptr;
        }
    for (void *p : {(void *)U.d_src, (void *)U.d_list, (void *)U.d_cap_src, (void *)U.d_cap_list})
        if (p) (void)hipFree(p);
    for (void *p : {(void *)U.h_src, (void *)U.h_list, (void *)U.h_cap_src, (void *)U.h_cap_list})
        if (p) (void)hipHostFree(p);
    if (U.ev_done) (void)hipEventDestroy(U.ev_done);
    U = UpdateState();
}

// The block list of a create, kept for the refill plan: index lists copied (the caller may free its own), `data` = a
// token naming the input block id -- the analysis with blocks_on_device never reads it, it only records it as the
// source of every chunk of its pack plan.
std::unique_ptr<UpdateInputs> keep_inputs(int mtype, int dtype, int64_t nrows, int64_t ncols, const std::vector<BlockIn> &in,
                                          const std::vector<int64_t> &ids, int64_t nids, const AnalysisOptions &ao,
                                          const AnalysisOptions *ao_t) {
    std::unique_ptr<UpdateInputs> K(new UpdateInputs());
    K->mtype = mtype;
    K->dtype = dtype;
    K->nrows = nrows;
    K->ncols = ncols;
    K->nids = nids;
    K->ao = ao;
    if (ao_t) K->ao_t = *ao_t;
    K->in = in;
    size_t nl = 0;
    for (const BlockIn &B : in) nl += (B.ridx ? 1 : 0) + (B.cidx && B.cidx != B.ridx ? 1 : 0);
    K->lists.reserve(nl);  // the BlockIn point into these vectors: no reallocation below
    for (size_t b = 0; b < in.size(); b++) {
        BlockIn &B = K->in[b];
        const int64_t id = ids[b];
        B.data = reinterpret_cast<const char *>((uintptr_t)(id + 1) * 16);
        const bool same = B.cidx == B.ridx;
        if (B.ridx) {
            K->lists.emplace_back(B.ridx, B.ridx + B.m);
            B.ridx = K->lists.back().data();
        }
        if (same) {
            B.cidx = B.ridx;
        } else if (B.cidx) {
            K->lists.emplace_back(B.cidx, B.cidx + B.n);
            B.cidx = K->lists.back().data();
        }
    }
    return K;
}

// the pack plan of the same analysis run on the kept block list, by input block id
std::string make_refill_plan(const UpdateInputs &inp, bool transposed, const Analysis &real, RefillPlan &R) {
    Analysis probe;
    AnalysisOptions ao = transposed ? inp.ao_t : inp.ao;
    ao.sink = nullptr;
    ao.blocks_on_device = true;
    ao.skip_colors = true;
    ao.meta_only = false;
    std::string err = transposed ? probe.build(MT_BLOCKSPARSE, inp.dtype, inp.ncols, inp.nrows, transposed_blocks(inp.in), ao)
                                 : probe.build(inp.mtype, inp.dtype, inp.nrows, inp.ncols, inp.in, ao);
    if (!err.empty()) return err;
    // the placement is a function of the structure and the options only: it must reproduce the image it refills
    if (probe.value_bytes != real.value_bytes || probe.waves.size() != real.waves.size() ||
        std::memcmp(probe.waves.data(), real.waves.data(), real.waves.size() * sizeof(WaveWork)) != 0)
        return "the refill plan does not reproduce the image (BSM_* tunables changed since the create?)";
    const int E = 16 / probe.es;
    R = RefillPlan();
    const int64_t nids = inp.nids;
    R.nids = nids;
    R.cptr.assign((size_t)nids + 1, 0);
    R.chunks.reserve(probe.pack_plan.size());
    for (const PackChunk &pc : probe.pack_plan) {
        RefillChunk c;
        c.dst_unit = pc.dst_unit;
        c.id = (int32_t)(pc.src / 16 - 1);
        c.ra = pc.ra;
        c.n = pc.n;
        c.woff = pc.woff;
        c.perm_off = pc.perm_off;
        c.mc = (int16_t)pc.mc;
        c.trans = (int16_t)pc.trans;
        R.chunks.push_back(c);
        R.cptr[(size_t)c.id + 1]++;
    }
    std::stable_sort(R.chunks.begin(), R.chunks.end(), [](const RefillChunk &a, const RefillChunk &b) { return a.id < b.id; });
    for (int64_t i = 0; i < nids; i++) R.cptr[i + 1] += R.cptr[i];
    R.colpos = std::move(probe.pack_colpos);
    // segments: a chunk's strips (identity) or columns (scattered), cut into pieces of at most kRefillItemUnits units
    for (size_t k = 0; k < R.chunks.size(); k++) {
        const RefillChunk &c = R.chunks[k];
        const int32_t lo0 = c.perm_off >= 0 ? 0 : c.woff / E;
        const int32_t hi0 = c.perm_off >= 0 ? c.n : (c.woff + c.n - 1) / E + 1;
        const int32_t step = std::max(1, kRefillItemUnits / (int)c.mc);
        for (int32_t lo = lo0; lo < hi0; lo += step) {
            const int32_t hi = std::min(hi0, lo + step);
            R.segs.push_back(RefillSeg{(int32_t)k, lo, hi, (int32_t)c.mc * (hi - lo)});
        }
    }
    // items: runs of up to 64 segments / kRefillItemUnits units; items_id never cross a block id
    auto make_items = [&](bool by_id, std::vector<RefillItem> &out) {
        int32_t first = 0, count = 0, units = 0;
        for (int32_t g = 0; g < (int32_t)R.segs.size(); g++) {
            const RefillSeg &sg = R.segs[g];
            const bool new_id = count > 0 && R.chunks[sg.chunk].id != R.chunks[R.segs[first].chunk].id;
            if (count > 0 && (count == 64 || units + sg.units > kRefillItemUnits || (by_id && new_id))) {
                out.push_back(RefillItem{first, count});
                count = units = 0;
            }
            if (count == 0) first = g;
            count++;
            units += sg.units;
        }
        if (count > 0) out.push_back(RefillItem{first, count});
    };
    make_items(false, R.items_all);
    make_items(true, R.items_id);
    R.iptr.assign((size_t)nids + 1, 0);
    for (const RefillItem &it : R.items_id) R.iptr[(size_t)R.chunks[R.segs[it.seg_first].chunk].id + 1]++;
    for (int64_t i = 0; i < nids; i++) R.iptr[i + 1] += R.iptr[i];
    R.built = true;
    return "";
}

struct U16 {
    uint64_t a, b;
};
// one chunk into the panel at dst: element (i, w) of the chunk to merged column q (identity: woff + w), i.e. unit
// (q / E) * mc + i, slot q % E -- what the packer of the create path writes
template <typename U>
void refill_chunk(const RefillChunk &c, const int32_t *colpos, const U *src, int64_t ld, int E, U *dst) {
    for (int64_t w = 0; w < c.n; w++) {
        const int64_t q = c.perm_off >= 0 ? colpos[c.perm_off + w] : c.woff + w;
        U *d = dst + ((q / E) * c.mc) * E + (q % E);
        for (int i = 0; i < c.mc; i++)
            d[(int64_t)i * E] = c.trans ? src[w + (int64_t)(c.ra + i) * ld] : src[(c.ra + i) + w * ld];
    }
}

// host refill of an analysis-only image (Analysis::values) through plan P
void refill_host(Analysis &an, const RefillPlan &P, int64_t nupd, const int64_t *ids, const void *const *src, const int64_t *ld) {
    const int es = an.es, E = 16 / es;
    for (int64_t k = 0; k < nupd; k++) {
        const int64_t id = ids[k];
        if (id < 0 || id >= P.nids) continue;
        for (int64_t ci = P.cptr[id]; ci < P.cptr[id + 1]; ci++) {
            const RefillChunk &c = P.chunks[ci];
            char *dst = an.values.data() + (size_t)c.dst_unit * 16;
            if (es == 4)
                refill_chunk<uint32_t>(c, P.colpos.data(), (const uint32_t *)src[k], ld[k], E, (uint32_t *)dst);
            else if (es == 8)
                refill_chunk<uint64_t>(c, P.colpos.data(), (const uint64_t *)src[k], ld[k], E, (uint64_t *)dst);
            else
                refill_chunk<U16>(c, P.colpos.data(), (const U16 *)src[k], ld[k], E, (U16 *)dst);
        }
    }
}

template <typename V> hipError_t upload_plan(const std::vector<V> &v, void **d) {
    if (v.empty()) return hipSuccess;
    hipError_t e = hipMalloc(d, v.size() * sizeof(V));
    if (e == hipSuccess) e = hipMemcpy(*d, v.data(), v.size() * sizeof(V), hipMemcpyHostToDevice);
    return e;
}

// first update on this device: plans, table, list, event (synchronous; later updates allocate nothing)
hipError_t update_setup(LocalOperator &op) {
    UpdateState &U = op.upd;
    const int nimg = op.has_t ? 2 : 1;
    const int64_t nids = op.upd_in->nids;
    hipError_t e = hipSuccess;
    int64_t cap = 0;
    for (int k = 0; k < nimg && e == hipSuccess; k++) {
        RefillDevice &R = U.img[k];
        const RefillPlan &P = U.plan[k];
        cap += (int64_t)P.items_id.size();
        if (R.ready) continue;
        e = upload_plan(P.chunks, &R.d_chunks);
        if (e == hipSuccess) e = upload_plan(P.colpos, &R.d_colpos);
        if (e == hipSuccess) e = upload_plan(P.segs, &R.d_segs);
        if (e == hipSuccess) e = upload_plan(P.items_all, &R.d_items_all);
        if (e == hipSuccess) e = upload_plan(P.items_id, &R.d_items_id);
        if (e == hipSuccess) R.ready = true;
    }
    if (e == hipSuccess && !U.d_src) {
        U.nids = nids;
        U.list_cap = std::max<int64_t>(cap, 1);
        e = hipMalloc((void **)&U.d_src, (size_t)std::max<int64_t>(nids, 1) * sizeof(RefillSrc));
        if (e == hipSuccess) e = hipMalloc((void **)&U.d_list, (size_t)U.list_cap * 4);
        if (e == hipSuccess) e = hipHostMalloc((void **)&U.h_src, (size_t)std::max<int64_t>(nids, 1) * sizeof(RefillSrc), hipHostMallocDefault);
        if (e == hipSuccess) e = hipHostMalloc((void **)&U.h_list, (size_t)U.list_cap * 4, hipHostMallocDefault);
        const size_t tb = (size_t)std::max<int64_t>(nids, 1) * sizeof(RefillSrc);
        if (e == hipSuccess) e = hipMalloc((void **)&U.d_cap_src, tb);
        if (e == hipSuccess) e = hipMalloc((void **)&U.d_cap_list, (size_t)U.list_cap * 4);
        if (e == hipSuccess) e = hipHostMalloc((void **)&U.h_cap_src, tb, hipHostMallocDefault);
        if (e == hipSuccess) e = hipHostMalloc((void **)&U.h_cap_list, (size_t)U.list_cap * 4, hipHostMallocDefault);
        if (e == hipSuccess) e = hipEventCreateWithFlags(&U.ev_done, hipEventDisableTiming);
        if (e == hipSuccess) {
            std::memset(U.h_src, 0, tb);
            std::memset(U.h_cap_src, 0, tb);
        }
    }
    return e;
}

// item list of a subset update for image k at `out`: the items of every updated id; returns its length
int64_t subset_list(const RefillPlan &P, int64_t nupd, const int64_t *ids, int32_t *out) {
    int64_t len = 0;
    for (int64_t q = 0; q < nupd; q++) {
        const int64_t id = ids[q];
        if (id < 0 || id >= (int64_t)P.iptr.size() - 1) continue;
        for (int64_t i = P.iptr[id]; i < P.iptr[id + 1]; i++) out[len++] = (int32_t)i;
    }
    return len;
}

// Writes the table (entries src[q] for ids[q]) and the lists, unless the device already holds exactly these; then
// launches the refill of every image on st.  lists[k] / nitems[k] receive what image k runs.
int enqueue_refill(LocalOperator &op, int64_t nupd, const int64_t *ids, bool full, const RefillSrc *src, hipStream_t st) {
    UpdateState &U = op.upd;
    const int es = op.an.es, nimg = op.has_t ? 2 : 1;
    std::vector<int32_t> list;
    int64_t off[2] = {0, 0}, len[2] = {0, 0};
    if (!full) {
        list.resize((size_t)U.list_cap);
        int64_t at = 0;
        for (int k = 0; k < nimg; k++) {
            off[k] = at;
            len[k] = subset_list(U.plan[k], nupd, ids, list.data() + at);
            at += len[k];
        }
        list.resize((size_t)at);
    }
    const int64_t want_len = full ? -1 : (int64_t)list.size();
    int64_t lo = INT64_MAX, hi = -1;
    for (int64_t q = 0; q < nupd; q++) {
        lo = std::min(lo, ids[q]);
        hi = std::max(hi, ids[q]);
    }
    // does (tab, lst, lst_len) already hold this call's sources and list?
    auto holds = [&](const RefillSrc *tab, const int32_t *lst, int64_t lst_len) {
        if (lst_len != want_len || (!full && std::memcmp(lst, list.data(), list.size() * 4) != 0)) return false;
        for (int64_t q = 0; q < nupd; q++)
            if (tab[ids[q]].ptr != src[q].ptr || tab[ids[q]].ld != src[q].ld) return false;
        return true;
    };
    const RefillSrc *d_tab = U.d_src;
    const int32_t *d_lst = U.d_list;
    hipError_t e = hipSuccess;
    if (capturing(st)) {
        // captured copy: the graph copies its own snapshot into the capture table, then refills from it
        if (U.cap_valid && !holds(U.h_cap_src, U.h_cap_list, U.cap_list_len))
            return fail(BSM_ERR_UNSUPPORTED, "a handle holds one captured source table: a later captured update must name "
                                             "the same blocks, arrays and ids as the first one");
        if (!U.cap_valid) {
            for (int64_t q = 0; q < nupd; q++) U.h_cap_src[ids[q]] = src[q];
            if (!list.empty()) std::memcpy(U.h_cap_list, list.data(), list.size() * 4);
            U.cap_list_len = want_len;
            U.cap_valid = true;
        }
        e = hipMemcpyAsync(U.d_cap_src + lo, U.h_cap_src + lo, (size_t)(hi - lo + 1) * sizeof(RefillSrc), hipMemcpyHostToDevice, st);
        if (e == hipSuccess && !list.empty())
            e = hipMemcpyAsync(U.d_cap_list, U.h_cap_list, list.size() * 4, hipMemcpyHostToDevice, st);
        if (e != hipSuccess) return hip_fail(e, "update: captured source table");
        d_tab = U.d_cap_src;
        d_lst = U.d_cap_list;
    } else if (U.table_valid && holds(U.h_src, U.h_list, U.list_len)) {
        // the table of the last update serves: order this stream behind that update (its copy may be on another stream)
        if (U.pending) e = hipStreamWaitEvent(st, U.ev_done, 0);
        if (e != hipSuccess) return hip_fail(e, "update: wait for the source table");
    } else {
        if (U.pending) e = hipEventSynchronize(U.ev_done);  // the kernels of the last update have read the table
        if (e != hipSuccess) return hip_fail(e, "update: previous refill");
        U.pending = false;
        U.table_valid = false;
        for (int64_t q = 0; q < nupd; q++) U.h_src[ids[q]] = src[q];
        e = hipMemcpyAsync(U.d_src + lo, U.h_src + lo, (size_t)(hi - lo + 1) * sizeof(RefillSrc), hipMemcpyHostToDevice, st);
        if (e == hipSuccess && !list.empty()) {
            std::memcpy(U.h_list, list.data(), list.size() * 4);
            e = hipMemcpyAsync(U.d_list, U.h_list, list.size() * 4, hipMemcpyHostToDevice, st);
        }
        if (e != hipSuccess) return hip_fail(e, "update: source table");
        U.list_len = want_len;
        U.table_valid = true;
    }
    for (int k = 0; k < nimg; k++) {
        const RefillDevice &R = U.img[k];
        const RefillPlan &P = U.plan[k];
        e = full ? launch_refill(es, R.d_chunks, R.d_colpos, R.d_segs, R.d_items_all, nullptr, (long long)P.items_all.size(),
                                 d_tab, (k ? op.img_t : op.img).d_values, st)
                 : launch_refill(es, R.d_chunks, R.d_colpos, R.d_segs, R.d_items_id, d_lst + off[k], (long long)len[k], d_tab,
                                 (k ? op.img_t : op.img).d_values, st);
        if (e != hipSuccess) return hip_fail(e, "refill_kernel");
    }
    if (d_tab == U.d_cap_src) return BSM_OK;  // a captured update leaves the eager table and its event alone
    e = hipEventRecord(U.ev_done, st);
    if (e != hipSuccess) return hip_fail(e, "update: event");
    U.pending = true;
    return BSM_OK;
}
}  // namespace

int LocalOperator::ensure_plans() {
    if (!upd_in) return fail(BSM_ERR_UNSUPPORTED, "handle keeps no block list");
    for (int k = 0; k < (has_t ? 2 : 1); k++) {
        if (upd.plan[k].built) continue;
        std::string err = make_refill_plan(*upd_in, k == 1, k ? an_t : an, upd.plan[k]);
        if (!err.empty()) return fail(BSM_ERR_UNSUPPORTED, "update: " + err);
    }
    return BSM_OK;
}

int LocalOperator::refill(int64_t nupd, const int64_t *ids, bool full, const void *const *blocks, const int64_t *ld, int memspace,
                          hipStream_t st, const std::vector<int64_t> &bm, const std::vector<int64_t> &bn) {
    if (!upd_in) return fail(BSM_ERR_UNSUPPORTED, "handle keeps no block list");
    if (device == BSM_DEVICE_NONE) {  // the host images (Analysis::values)
        if (memspace != BSM_MEM_HOST) return fail(BSM_ERR_INVALID, "an analysis-only handle takes host blocks only");
        int rc = ensure_plans();
        if (rc != BSM_OK) return rc;
        refill_host(an, upd.plan[0], nupd, ids, blocks, ld);
        if (has_t) refill_host(an_t, upd.plan[1], nupd, ids, blocks, ld);
        return BSM_OK;
    }
    DeviceGuard guard;
    hipError_t e = guard.enter(device);
    if (e != hipSuccess) return hip_fail(e, "hipSetDevice");
    UpdateState &U = upd;
    if (capturing(st) && (memspace != BSM_MEM_DEVICE || !U.d_src))
        return fail(BSM_ERR_UNSUPPORTED, memspace != BSM_MEM_DEVICE
                                             ? "an update from host blocks synchronises: it cannot be graph-captured"
                                             : "the first update of a handle uploads its plan: run one before capturing");
    int rc0 = ensure_plans();
    if (rc0 != BSM_OK) return rc0;
    e = update_setup(*this);
    if (e != hipSuccess) return hip_fail(e, "update: plan upload");
    const int es = an.es;
    if (memspace == BSM_MEM_DEVICE) {
        std::vector<RefillSrc> src((size_t)nupd);
        for (int64_t q = 0; q < nupd; q++) src[q] = RefillSrc{(uint64_t)(uintptr_t)blocks[q], ld[q]};
        return enqueue_refill(*this, nupd, ids, full, src.data(), st);
    }
    // host blocks: raw copies (ld = m) into the pinned windows of the create path, one H2D copy per window, the same
    // kernel reads the staged blocks.  Windows alternate between two pinned and two device buffers.
    const size_t wcap_min = (size_t)64 << 20;
    size_t biggest = 0, total = 0;
    for (int64_t q = 0; q < nupd; q++) {
        const size_t b = (size_t)bm[ids[q]] * (size_t)bn[ids[q]] * (size_t)es;
        biggest = std::max(biggest, b);
        total += (b + 255) / 256 * 256;
    }
    const size_t wcap = std::max(biggest, std::min(wcap_min, total));
    // window of every block and its offset in it
    std::vector<int64_t> wstart(1, 0);  // first update position of every window
    std::vector<size_t> boff((size_t)nupd);
    {
        size_t at = 0;
        for (int64_t q = 0; q < nupd; q++) {
            const size_t b = ((size_t)bm[ids[q]] * (size_t)bn[ids[q]] * (size_t)es + 255) / 256 * 256;
            if (at + b > wcap && at > 0) {
                wstart.push_back(q);
                at = 0;
            }
            boff[q] = at;
            at += b;
        }
        wstart.push_back(nupd);
    }
    const int nwin = (int)wstart.size() - 1;
    std::unique_lock<std::mutex> lock(g_pool.mu);
    void *dwin[2] = {nullptr, nullptr};
    hipEvent_t ev[2] = {nullptr, nullptr};
    bool ev_pending[2] = {false, false};
    struct Cleanup {
        void **d;
        hipEvent_t *ev;
        hipStream_t st;
        UpdateState *u;
        ~Cleanup() {
            (void)hipStreamSynchronize(st);
            u->pending = false;
            u->table_valid = false;  // the eager table named the staging windows freed here
            for (int i = 0; i < 2; i++) {
                if (d[i]) (void)hipFree(d[i]);
                if (ev[i]) (void)hipEventDestroy(ev[i]);
            }
        }
    } cleanup{dwin, ev, st, &U};
    for (int i = 0; i < std::min(nwin, 2) && e == hipSuccess; i++) {
        e = hipMalloc(&dwin[i], std::max<size_t>(wcap, 16));
        if (e == hipSuccess) e = hipEventCreateWithFlags(&ev[i], hipEventDisableTiming);
        if (e == hipSuccess && g_pool.cap[i] < wcap) {
            if (g_pool.buf[i]) (void)hipHostFree(g_pool.buf[i]);
            g_pool.buf[i] = nullptr;
            g_pool.cap[i] = 0;
            const size_t want = std::max<size_t>(wcap, wcap_min);
            e = hipHostMalloc((void **)&g_pool.buf[i], want, hipHostMallocDefault);
            if (e == hipSuccess) g_pool.cap[i] = want;
        }
    }
    if (e != hipSuccess) return hip_fail(e, "update: staging windows");
    std::vector<RefillSrc> src((size_t)nupd);
    for (int64_t q = 0; q < nupd; q++) {
        const int w = (int)(std::upper_bound(wstart.begin(), wstart.end(), q) - wstart.begin()) - 1;
        src[q] = RefillSrc{(uint64_t)(uintptr_t)((char *)dwin[w & 1] + boff[q]), std::max<int64_t>(bm[ids[q]], 1)};
    }
    for (int w = 0; w < nwin; w++) {
        const int i = w & 1;
        if (ev_pending[i]) {
            e = hipEventSynchronize(ev[i]);  // the copy out of this pinned window has run
            if (e != hipSuccess) return hip_fail(e, "update: staging");
            ev_pending[i] = false;
        }
        char *pin = g_pool.buf[i];
        size_t bytes = 0;
        for (int64_t q = wstart[w]; q < wstart[w + 1]; q++) {
            const int64_t m = bm[ids[q]], n = bn[ids[q]];
            const char *b = (const char *)blocks[q];
            char *d = pin + boff[q];
            if (ld[q] == m)
                std::memcpy(d, b, (size_t)(m * n) * es);
            else
                for (int64_t c = 0; c < n; c++) std::memcpy(d + (size_t)(c * m) * es, b + (size_t)(c * ld[q]) * es, (size_t)m * es);
            bytes = boff[q] + (size_t)(m * n) * es;
        }
        if (bytes) e = hipMemcpyAsync(dwin[i], pin, bytes, hipMemcpyHostToDevice, st);
        if (e == hipSuccess) e = hipEventRecord(ev[i], st);
        if (e != hipSuccess) return hip_fail(e, "update: staged copy");
        ev_pending[i] = true;
        // the whole update in one window in creation order: the items of a full refill
        const bool wfull = full && nwin == 1;
        int rc = enqueue_refill(*this, wstart[w + 1] - wstart[w], ids + wstart[w], wfull, src.data() + wstart[w], st);
        if (rc != BSM_OK) return rc;
    }
    e = hipStreamSynchronize(st);
    U.pending = false;
    U.table_valid = false;  // its entries named the staging windows, freed below (Cleanup)
    if (e != hipSuccess) return hip_fail(e, "update: refill");
    return BSM_OK;
}

bool capturing(hipStream_t st) {
    hipStreamCaptureStatus cs = hipStreamCaptureStatusNone;
    if (hipStreamIsCapturing(st, &cs) != hipSuccess) {
        (void)hipGetLastError();
        return false;
    }
    return cs != hipStreamCaptureStatusNone;
}

AnalysisOptions to_aopt(const bsm_options &o, ValueSink *sink) {
    AnalysisOptions a;
    a.sink = sink;
    a.blocks_on_device = (o.blocks_memspace == BSM_MEM_DEVICE);
    a.coloring = (int)o.coloring;
    a.scheduler = o.scheduler;
    a.validate = 1;  // indices are always range-checked: a bad index must never reach a kernel
    a.accumulate = o.accumulate;
    a.own_lo = o.own_lo;
    a.own_hi = o.own_hi;
    return a;
}

int LocalOperator::build(int mtype, int dtype, int64_t nrows, int64_t ncols, const std::vector<BlockIn> &in,
                         const std::vector<int64_t> &ids, int64_t nids, const bsm_options &o, bool colors, const std::string &prefix) {
    const bool devblocks = (o.blocks_memspace == BSM_MEM_DEVICE);
    if (devblocks && device == BSM_DEVICE_NONE) return fail(BSM_ERR_INVALID, "device-resident blocks need a device handle");
    // host blocks of a device operator are streamed to it while they are packed; device blocks are packed there, below
    const bool streamed = device != BSM_DEVICE_NONE && !devblocks;
    DeviceSink sink(&img.d_values), sink_t(&img_t.d_values);
    AnalysisOptions ao = to_aopt(o, streamed ? &sink : nullptr);
    ao.skip_colors = !colors;
    // what one resident round of the device holds decides how far outlier row groups may be cut (Analysis::plan_cuts)
    if (device != BSM_DEVICE_NONE) {
        int ncu = 0;
        if (hipDeviceGetAttribute(&ncu, hipDeviceAttributeMultiprocessorCount, device) == hipSuccess)
            ao.num_cus = ncu;
        else
            (void)hipGetLastError();
    }
    std::string err = an.build(mtype, dtype, nrows, ncols, in, ao);
    ao.sink = nullptr;
    bool want_t = o.transpose_image == 1;
    if (o.transpose_image == 2 && device != BSM_DEVICE_NONE) {  // "when it is cheap"
        size_t free_b = 0, total_b = 0;
        if (hipMemGetInfo(&free_b, &total_b) == hipSuccess)
            want_t = (size_t)an.value_bytes <= free_b / 16;
        else
            (void)hipGetLastError();
    }
    // second ordering: the transposed operator as a forward image (rows <-> columns, blocks read transposed by the
    // packer), built from the same caller arrays
    AnalysisOptions ao_t = transpose_aopt(o);
    ao_t.num_cus = ao.num_cus;
    if (err.empty() && want_t && mtype != MT_SYMMETRIC) {
        bool plain = true;
        for (const BlockIn &B : in) plain &= (B.kind == KIND_PLAIN);
        if (plain) {
            ao_t.sink = streamed ? &sink_t : nullptr;
            err = an_t.build(MT_BLOCKSPARSE, an.dtype, an.ncols, an.nrows, transposed_blocks(in), ao_t);
            ao_t.sink = nullptr;
            has_t = err.empty();
        }
    }
    if (!err.empty()) return build_error(prefix + err);
    upd_in = keep_inputs(mtype, dtype, nrows, ncols, in, ids, nids, ao, has_t ? &ao_t : nullptr);
    if (devblocks) {  // the blocks may live on another device of a context: read over xGMI
        hipError_t e = device_pack(an, &img.d_values);
        if (e == hipSuccess && has_t) e = device_pack(an_t, &img_t.d_values);
        if (e != hipSuccess) return hip_fail(e, "device-side packing");
    }
    fill_image(an, o, true, img);
    if (has_t) fill_image(an_t, o, false, img_t);
    if (device != BSM_DEVICE_NONE) {
        hipError_t e = upload_image(an, img, device);
        if (e == hipSuccess && has_t) e = upload_image(an_t, img_t, device);
        if (e != hipSuccess) return hip_fail(e, "device upload");
    }
    return BSM_OK;
}

// what a built operator owns on its device: THE list (beside free_image, which knows an image's arrays)
void LocalOperator::release() {
    free_image(img);
    free_image(img_t);
    update_free(upd);
    il_free(il);
}

bool il_reserve(ILWork &il, long long need) {
    if (il.rows >= need) return true;
    il_free(il);
    void *xr = nullptr, *w = nullptr;
    if (hipMalloc(&xr, (size_t)need * 128) != hipSuccess || hipMalloc(&w, (size_t)need * 128) != hipSuccess) {
        (void)hipGetLastError();
        if (xr) (void)hipFree(xr);
        return false;
    }
    il.xr = xr;
    il.w = w;
    il.rows = need;
    return true;
}

}  // namespace bsm
