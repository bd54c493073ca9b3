// bsm_dist.cpp -- ONE handle spread over the devices of a bsm_ctx_t (include/bsm_rocm.h).
//
// The reference fans its block rows / colour classes out as tasks of one process
// (`@tasks for ...` with the scheduler stored in the matrix: src/vbcrs.jl:275-276,
// src/blockmatrix.jl:233-245, src/symmetricblockmatrix.jl:395-432).  Here the same call fans out
// over the GPUs of one node: contiguous ranges of block rows per device (balanced by stored
// entries), one stream per device, and only the y segments a device produced for rows of ANOTHER
// device travel -- as direct peer-to-peer copies over the xGMI links followed by a local add.
// One host thread issues everything; every step is asynchronous and ordered by events.
//
// This unit builds and maintains the handle (bsm_dist.h: the types); bsm_fanout.cpp issues its products.
#include <cstdlib>
#include <cstring>

#include "bsm_dist.h"
#include "bsm_poly.h"

namespace bsm {

void Part::release_sync() {
    if (ev_prod) (void)hipEventDestroy(ev_prod);
    if (ev_done) (void)hipEventDestroy(ev_done);
    if (ev_in) (void)hipEventDestroy(ev_in);
    if (stream) (void)hipStreamDestroy(stream);
    ev_prod = ev_done = ev_in = nullptr;
    stream = nullptr;
}

hipError_t Part::alloc_buffers(size_t vec_bytes, size_t recv_bytes, int K) {
    hipError_t e = hipMalloc(&d_x, vec_bytes * K);
    if (e == hipSuccess) e = hipMalloc(&d_w, vec_bytes * K);
    if (e == hipSuccess && recv_bytes) e = hipMalloc(&d_recv, recv_bytes * K);
    return e;
}

void Part::free_buffers() {
    for (void **q : {&d_x, &d_w, &d_recv}) {
        if (*q) (void)hipFree(*q);
        *q = nullptr;
    }
}

Workers::Workers(const std::vector<int> &devices) : n_((int)devices.size()), rc_(devices.size(), BSM_OK), msg_(devices.size()) {
    for (int p = 0; p < n_; p++) th_.emplace_back([this, p, dev = devices[p]] { loop(p, dev); });
}

Workers::~Workers() {
    {
        std::lock_guard<std::mutex> l(mu_);
        stop_ = true;
        gen_++;
    }
    go_.notify_all();
    for (auto &t : th_) t.join();
}

int Workers::run_fn(Fn fn, void *arg) {
    std::unique_lock<std::mutex> l(mu_);
    fn_ = fn;
    arg_ = arg;
    pending_ = n_;
    gen_++;
    go_.notify_all();
    done_.wait(l, [&] { return pending_ == 0; });
    fn_ = nullptr;
    for (int p = 0; p < n_; p++)
        if (rc_[p] != BSM_OK) return fail(rc_[p], msg_[p]);
    return BSM_OK;
}

void Workers::loop(int p, int dev) {
    (void)hipSetDevice(dev);
    uint64_t seen = 0;
    std::unique_lock<std::mutex> l(mu_);
    for (;;) {
        go_.wait(l, [&] { return gen_ != seen; });
        seen = gen_;
        if (stop_) return;
        const Fn fn = fn_;
        void *const arg = arg_;
        l.unlock();
        int rc = BSM_ERR_DEVICE;
        std::string msg;
        try {
            rc = fn(arg, p);
            if (rc != BSM_OK) msg = bsm_last_error();  // this thread's slot
        } catch (const std::exception &e) {
            msg = e.what();
        }
        l.lock();
        rc_[p] = rc;
        msg_[p] = msg;
        if (--pending_ == 0) done_.notify_all();
    }
}

}  // namespace bsm

// (defined here: DistState and PolyState must be complete where the handle's unique_ptrs are destroyed)
bsm_matrix_s::bsm_matrix_s() = default;
bsm_matrix_s::~bsm_matrix_s() = default;

namespace bsm {

void block_row_keys(const std::vector<BlockIn> &in, std::vector<int64_t> &key, std::vector<int64_t> &weight) {
    key.resize(in.size());
    weight.resize(in.size());
    for (size_t b = 0; b < in.size(); b++) {
        const BlockIn &B = in[b];
        int64_t k = B.r0 > 0 ? B.r0 : 1;
        if (B.ridx && B.m > 0) {
            k = B.ridx[0];
            for (int64_t i = 1; i < B.m; i++) k = std::min(k, B.ridx[i]);
        }
        key[b] = k;
        weight[b] = B.m * B.n;
    }
}

void partition_rows(int64_t nrows, const std::vector<int64_t> &key, const std::vector<int64_t> &weight,
                    int nparts, std::vector<int32_t> &part_of_block, std::vector<int64_t> &own_lo,
                    std::vector<int64_t> &own_hi) {
    const size_t nb = key.size();
    std::vector<int64_t> uk(key);
    std::sort(uk.begin(), uk.end());
    uk.erase(std::unique(uk.begin(), uk.end()), uk.end());
    const size_t nk = uk.size();
    std::vector<double> csum(nk + 1, 0.0);
    std::vector<size_t> kidx(nb);
    for (size_t b = 0; b < nb; b++) {
        kidx[b] = (size_t)(std::lower_bound(uk.begin(), uk.end(), key[b]) - uk.begin());
        csum[kidx[b] + 1] += (double)std::max<int64_t>(weight[b], 0);
    }
    for (size_t k = 0; k < nk; k++) csum[k + 1] += csum[k];
    const double total = csum[nk];
    std::vector<size_t> cut((size_t)nparts + 1, 0);
    for (int p = 1; p < nparts; p++) {
        const double target = total * p / nparts;
        size_t k = (size_t)(std::lower_bound(csum.begin(), csum.end(), target) - csum.begin());
        cut[p] = std::min(std::max(k, cut[p - 1]), nk);
    }
    cut[nparts] = nk;
    part_of_block.assign(nb, 0);
    {
        std::vector<int32_t> part_of_key(nk, 0);
        for (int p = 0; p < nparts; p++)
            for (size_t k = cut[p]; k < cut[p + 1]; k++) part_of_key[k] = p;
        for (size_t b = 0; b < nb; b++) part_of_block[b] = part_of_key[kidx[b]];
    }
    own_lo.assign(nparts, 1);
    own_hi.assign(nparts, 0);
    int first = -1, last = -1;
    for (int p = 0; p < nparts; p++) {
        if (cut[p] == cut[p + 1]) {  // no key: an empty range just below the next part's first row
            own_lo[p] = cut[p] < nk ? uk[cut[p]] : nrows + 1;
            own_hi[p] = own_lo[p] - 1;
            continue;
        }
        if (first < 0) first = p;
        last = p;
        own_lo[p] = uk[cut[p]];
        own_hi[p] = cut[p + 1] < nk ? uk[cut[p + 1]] - 1 : nrows;
    }
    if (first >= 0) {  // rows in front of the first key / behind the last block row belong to somebody
        own_lo[first] = 1;
        own_hi[last] = nrows;
    } else if (nparts > 0) {  // no block at all: part 0 owns (and scales) every row
        own_lo[0] = 1;
        own_hi[0] = nrows;
    }
}

namespace {

void block_hulls(const std::vector<BlockIn> &sub, Range &rows, Range &cols) {
    rows = cols = Range{};
    for (const BlockIn &B : sub) {
        if (B.m <= 0 || B.n <= 0) continue;
        int64_t rl, rh, cl, ch;
        if (B.ridx) {
            rl = rh = B.ridx[0];
            for (int64_t i = 1; i < B.m; i++) rl = std::min(rl, B.ridx[i]), rh = std::max(rh, B.ridx[i]);
        } else {
            rl = B.r0;
            rh = B.r0 + B.m - 1;
        }
        if (B.cidx) {
            cl = ch = B.cidx[0];
            for (int64_t i = 1; i < B.n; i++) cl = std::min(cl, B.cidx[i]), ch = std::max(ch, B.cidx[i]);
        } else {
            cl = B.c0;
            ch = B.c0 + B.n - 1;
        }
        rows = hull(rows, Range{rl - 1, rh});
        cols = hull(cols, Range{cl - 1, ch});
    }
}

// transfers + receive-buffer layout of a plan whose xr / out / touched ranges are known
void finish_plan(Plan &pl, const std::vector<Range> &touched, int es) {
    const int P = (int)pl.out.size();
    pl.zr.resize(P);
    pl.recv_bytes.assign(P, 0);
    for (int p = 0; p < P; p++) pl.zr[p] = hull(touched[p], pl.out[p]);
    for (int q = 0; q < P; q++)
        for (int p = 0; p < P; p++) {
            if (p == q) continue;
            const Range o = isect(touched[p], pl.out[q]);
            if (o.empty()) continue;
            pl.transfers.push_back(Transfer{p, q, o, pl.recv_bytes[q]});
            pl.recv_bytes[q] += ((size_t)o.len() * es + 255) & ~(size_t)255;
        }
}

}  // namespace

void dist_destroy(bsm_matrix_s *A) {
    if (!A->dist) return;
    DistState &D = *A->dist;
    D.workers.reset();
    for (auto &pp : D.parts) {
        Part &p = *pp;
        DeviceGuard g;
        (void)g.enter(p.device);
        if (p.stream) (void)hipStreamSynchronize(p.stream);
        p.release();
        p.free_buffers();
        p.release_sync();
    }
    if (D.ev_tail) {
        DeviceGuard g;
        (void)g.enter(D.tail_dev);
        (void)hipEventDestroy(D.ev_tail);
    }
    for (auto &kv : D.ev_x) {
        DeviceGuard g;
        (void)g.enter(kv.first);
        (void)hipEventDestroy(kv.second);
    }
    if (D.d_res) {
        DeviceGuard g;
        (void)g.enter(D.res_dev);
        (void)hipFree(D.d_res);
    }
    if (D.flags) (void)hipHostFree(D.flags);
    A->dist.reset();
}

int dist_create(bsm_matrix_s *A, bsm_ctx_s *ctx, int mtype, int dtype, int64_t nrows, int64_t ncols,
                const std::vector<BlockIn> &in, const std::vector<int64_t> &ids, const bsm_options &o) {
    const int P = (int)ctx->devices.size();
    if (P < 1) return fail(BSM_ERR_INVALID, "context has no device");
    A->dist.reset(new DistState());
    DistState &D = *A->dist;
    D.ctx = ctx;
    D.dtype = dtype;
    D.es = A->an.es;
    D.nrows = nrows;
    D.ncols = ncols;
    D.symmetric = (mtype == MT_SYMMETRIC);
    for (const BlockIn &B : in) D.symmetric |= (B.kind != KIND_PLAIN);  // symmetric view of a VBCRS

    std::vector<int64_t> key, weight, own_lo, own_hi;
    std::vector<int32_t> part_of;
    block_row_keys(in, key, weight);
    partition_rows(nrows, key, weight, P, part_of, own_lo, own_hi);

    std::vector<Range> touched_n(P), touched_t(P);
    D.plan_n.xr.resize(P);
    D.plan_n.out.resize(P);
    D.plan_t.xr.resize(P);
    D.plan_t.out.resize(P);
    const long long chunk_t = (ncols + P - 1) / P;
    // the COLUMN partition (what a part holds of a vector of length ncols when the vectors are partitioned,
    // and what it delivers of a product across the row partition): the row partition itself for square
    // operators -- y of one product is x of the next, part by part -- else equal chunks
    const bool square = (nrows == ncols);
    D.plan_n.in.resize(P);
    D.plan_t.in.resize(P);
    std::vector<std::vector<BlockIn>> subs(P);
    std::vector<std::vector<int64_t>> sub_ids(P);
    for (size_t b = 0; b < in.size(); b++) {
        subs[part_of[b]].push_back(in[b]);
        sub_ids[part_of[b]].push_back(ids[b]);
    }
    for (int p = 0; p < P; p++) {
        D.parts.emplace_back(new Part());
        Part &pt = *D.parts.back();
        pt.device = ctx->devices[p];
        pt.nblocks = (int64_t)subs[p].size();
        pt.own = Range{own_lo[p] - 1, own_hi[p]};
        block_hulls(subs[p], pt.rows, pt.cols);
        if (D.symmetric) pt.rows = pt.cols = hull(pt.rows, pt.cols);
        pt.has_image = !pt.rows.empty();
        // products ALONG the partition (op N; every op of a symmetric operator)
        D.plan_n.xr[p] = pt.cols;
        D.plan_n.out[p] = pt.own;
        touched_n[p] = pt.rows;
        // products ACROSS it (transpose / adjoint of a row-partitioned VBCRS / BlockSparseMatrix): every
        // part holds a partial result over the columns of its blocks; reduce-scatter onto equal chunks
        pt.colpart = square ? pt.own : Range{std::min<long long>(p * chunk_t, ncols), std::min<long long>((p + 1) * chunk_t, ncols)};
        D.plan_t.xr[p] = pt.rows;
        D.plan_t.out[p] = pt.colpart;
        touched_t[p] = pt.cols;
        D.plan_n.in[p] = pt.colpart;
        D.plan_t.in[p] = pt.own;
    }
    finish_plan(D.plan_n, touched_n, D.es);
    finish_plan(D.plan_t, touched_t, D.es);

    D.vlen = (size_t)std::max<long long>(std::max(nrows, ncols), 1) + 2;
    const size_t vec_bytes = D.vlen * D.es;
    for (int p = 0; p < P; p++) {
        Part &pt = *D.parts[p];
        DeviceGuard g;
        hipError_t e = g.enter(pt.device);
        if (e != hipSuccess) return hip_fail(e, "hipSetDevice");
        if (pt.has_image) {
            bsm_options po = o;
            po.ctx = nullptr;
            po.device = pt.device;
            po.transpose_image = 0;
            // the image defines (scales / overwrites) every row it touches plus the rows it owns
            po.own_lo = D.plan_n.zr[p].lo + 1;
            po.own_hi = D.plan_n.zr[p].hi;
            int rc = pt.build(mtype, dtype, nrows, ncols, subs[p], sub_ids[p], (int64_t)in.size(), po, false,
                              "device part " + std::to_string(p) + ": ");
            if (rc != BSM_OK) return rc;
        }
        e = hipStreamCreateWithFlags(&pt.stream, hipStreamNonBlocking);
        if (e == hipSuccess) e = hipEventCreateWithFlags(&pt.ev_prod, hipEventDisableTiming);
        if (e == hipSuccess) e = hipEventCreateWithFlags(&pt.ev_done, hipEventDisableTiming);
        if (e == hipSuccess) e = hipEventCreateWithFlags(&pt.ev_in, hipEventDisableTiming);
        if (e == hipSuccess) e = pt.alloc_buffers(vec_bytes, std::max(D.plan_n.recv_bytes[p], D.plan_t.recv_bytes[p]), 1);
        if (e != hipSuccess) return hip_fail(e, "multi-device buffers");
    }
    D.all_peer = ctx->peer_ok;  // enabled for every pair when the context was created (bsm_ctx_create)
    if (const char *v = std::getenv("BSM_DIST_COPIES")) D.all_peer = D.all_peer && std::atoi(v) == 0;  // tests: force the copy path
    if (const char *v = std::getenv("BSM_DIST_ONE_STREAM")) D.one_stream = std::atoi(v) != 0;
    {
        // flags and zero-keeping: on by default where they have been exercised -- every part on ONE physical device
        // (virtual devices).  On distinct devices a flag is polled by another GPU's command processor and the finish
        // kernels write their zeros into a PEER's work vector over xGMI (visible to the owner's next atomic
        // accumulation only if those remote writes have reached its L2 at the event boundary): neither has ever run
        // on this pool, so both are opt-in there (BSM_DIST_FLAGS=1 / BSM_DIST_REZERO=1) until one 2-GPU parity run of
        // test_work_vectors_stay_zero_* / test_flag_and_event_ordering_* has passed on real devices.
        bool one_device = true;
        for (int d : ctx->devices) one_device = one_device && d == ctx->devices[0];
        D.rezero = one_device;
        if (const char *v = std::getenv("BSM_DIST_REZERO")) D.rezero = std::atoi(v) != 0;
        int can = 1;
        for (int d : ctx->devices) {
            int c = 0;
            if (hipDeviceGetAttribute(&c, hipDeviceAttributeCanUseStreamWaitValue, d) != hipSuccess) {
                (void)hipGetLastError();
                c = 0;
            }
            can = can && c;  // EVERY device of the context must be able to run the wait packets
        }
        D.use_flags = one_device && can;
        if (const char *v = std::getenv("BSM_DIST_FLAGS")) D.use_flags = std::atoi(v) != 0 && can;
        if (D.use_flags) {
            hipError_t e = hipHostMalloc((void **)&D.flags, (size_t)(3 * P + 1) * sizeof(uint64_t), hipHostMallocCoherent | hipHostMallocPortable);
            if (e != hipSuccess) {
                (void)hipGetLastError();
                D.flags = nullptr;
                D.use_flags = false;
            } else {
                std::memset(D.flags, 0, (size_t)(3 * P + 1) * sizeof(uint64_t));
            }
        }
    }
    // one persistent issuing thread per device from five parts on (BSM_DIST_WORKERS = smallest part count that
    // gets them): below, the calling thread issues everything faster than the threads can be woken twice
    int wmin = 5;
    if (const char *v = std::getenv("BSM_DIST_WORKERS")) wmin = std::atoi(v);
    if (P >= wmin) D.workers.reset(new Workers(ctx->devices));
    return BSM_OK;
}


// bsm_update_blocks: every part refills its own image on its device, on its own stream, from the blocks it holds
// (device blocks on another device are read over xGMI, as at create; host blocks are staged per part).  The fan-out
// orders a product's work by streams, events and flags that an update is not part of, so the update stands outside
// it: it waits for the caller's stream (where the new blocks were written) and for every earlier product of the
// handle, refills, and returns when every part's image holds the new values.
int dist_update(bsm_matrix_s *A, int64_t nupd, const int64_t *ids, bool full, const void *const *blocks, const int64_t *ld,
                int memspace, hipStream_t stream) {
    DistState &D = *A->dist;
    std::lock_guard<std::mutex> lock(D.mu);
    hipError_t e = hipStreamSynchronize(stream);
    if (e == hipSuccess) e = drain_handle(D);
    if (e != hipSuccess) return hip_fail(e, "update: drain");
    std::vector<int64_t> pid;
    std::vector<const void *> pblk;
    std::vector<int64_t> pld;
    for (auto &pp : D.parts) {
        Part &pt = *pp;
        if (!pt.has_image) continue;
        int rc0 = pt.ensure_plans();
        if (rc0 != BSM_OK) return rc0;
        const RefillPlan &R = pt.upd.plan[0];
        pid.clear();
        pblk.clear();
        pld.clear();
        for (int64_t k = 0; k < nupd; k++) {
            const int64_t id = ids[k];
            if (id < R.nids && R.cptr[id + 1] > R.cptr[id]) {  // the part holds chunks of block id
                pid.push_back(id);
                pblk.push_back(blocks[k]);
                pld.push_back(ld[k]);
            }
        }
        if (pid.empty()) continue;
        DeviceGuard g;
        e = g.enter(pt.device);
        if (e != hipSuccess) return hip_fail(e, "hipSetDevice");
        int rc = pt.refill((int64_t)pid.size(), pid.data(), full, pblk.data(), pld.data(), memspace, pt.stream, A->blk_m, A->blk_n);
        if (rc != BSM_OK) return rc;
        e = hipStreamSynchronize(pt.stream);
        if (e != hipSuccess) return hip_fail(e, "update: refill");
        pt.upd.pending = false;
    }
    return BSM_OK;
}

int dist_part_info(bsm_matrix_s *A, int32_t part, bsm_part_info_t *out) {
    DistState &D = *A->dist;
    if (part < 0 || part >= (int32_t)D.parts.size()) return fail(BSM_ERR_INVALID, "part index out of range");
    const Part &p = *D.parts[part];
    std::memset(out, 0, sizeof *out);
    out->device = p.device;
    out->own_lo = p.own.lo + 1;
    out->own_hi = p.own.hi;
    const Range z = D.plan_n.zr[part];
    out->touched_lo = z.lo + 1;
    out->touched_hi = z.hi;
    out->device_bytes = p.img.device_bytes;
    out->nblocks = p.nblocks;
    out->col_lo = p.colpart.lo + 1;
    out->col_hi = p.colpart.hi;
    return BSM_OK;
}

std::vector<ImageRef> dist_images(bsm_matrix_s *A) {
    std::vector<ImageRef> out;
    for (const auto &p : A->dist->parts)
        if (p->has_image) out.emplace_back(&p->an, &p->img);
    return out;
}

int64_t dist_device_bytes(const bsm_matrix_s *A) {
    int64_t s = 0;
    for (const auto &p : A->dist->parts) s += p->img.device_bytes;
    return s;
}

}  // namespace bsm
