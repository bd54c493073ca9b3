// bsm_fanout.cpp -- the products of ONE handle spread over the devices of a bsm_ctx_t (bsm_dist.h: its state; bsm_dist.cpp
// builds and maintains it).  Every product runs inside one frame (fan_out) that is handed one of two drivers:
// FusedProduct (device-resident vectors, every device peer-accessible: dist_mul_fused) or CopyProduct (host vectors,
// devices without peer access: dist_mul_copies).  How a product's steps are ordered across streams is a value of its own
// (Ordering).
#include <atomic>
#include <complex>
#include <cstring>

#include "bsm_dist.h"

namespace bsm {

namespace {

hipError_t copy_between(void *dst, int ddev, const void *src, int sdev, size_t bytes, hipStream_t st) {
    if (bytes == 0) return hipSuccess;
    if (ddev == sdev) return hipMemcpyAsync(dst, src, bytes, hipMemcpyDeviceToDevice, st);
    return hipMemcpyPeerAsync(dst, ddev, src, sdev, bytes, st);  // xGMI, device to device
}

template <typename T> void host_axpby(T *y, const T *r, long long n, T beta) {
    for (long long i = 0; i < n; i++) y[i] = beta * y[i] + r[i];
}

int pointer_device(const void *p, int fallback) {
    hipPointerAttribute_t at;
    std::memset(&at, 0, sizeof at);
    if (hipPointerGetAttributes(&at, p) != hipSuccess) {
        (void)hipGetLastError();
        return fallback;
    }
    return at.device;
}

}  // namespace

// whether part `pt` takes the interleaved multi-RHS pass for a product of K columns, given its work arrays
// (A part's image is never mixed storage: its dtype is the vector type of every product.)
static bool takes_il(const Part &pt, bool opT, int K) {
    return !pt.il_failed && wants_il_arrays(plan_input(pt.img, opT, pt.img.dtype, K, false));
}

// the part's work arrays if its image / this product take the interleaved pass (and they can be had), else null.
static ILWork *part_il(Part &pt, bool opT, int K) {
    if (!takes_il(pt, opT, K)) return nullptr;
    pt.il_failed = !il_reserve(pt.il, std::max(pt.img.nrows, pt.img.ncols));
    return pt.il_failed ? nullptr : &pt.il;
}

// Waits for everything queued on the devices of the parts: every device is drained whatever fails, the first error is
// returned.
static hipError_t drain_devices(DistState &D) {
    hipError_t first = hipSuccess;
    for (auto &pt : D.parts) {
        DeviceGuard g;
        hipError_t e = g.enter(pt->device);
        if (e == hipSuccess) e = hipDeviceSynchronize();
        if (first == hipSuccess) first = e;
    }
    return first;
}

// Waits until nothing of any earlier product of the handle can still be running (or reading a part's buffers).
hipError_t drain_handle(DistState &D) {
    const int P = (int)D.parts.size();
    hipError_t e = hipSuccess;
    for (int p = 0; p < P && e == hipSuccess; p++) {
        DeviceGuard g;
        e = g.enter(D.parts[p]->device);
        if (e == hipSuccess) e = hipStreamSynchronize(D.parts[p]->stream);
    }
    if (e == hipSuccess && D.ev_tail) e = hipEventSynchronize(D.ev_tail);
    // the fused path works on the CALLERS' streams (run[p] = the part's caller stream), and a peer's finish kernel
    // reads this part's work vector over xGMI: ev_done is recorded on run[p] after the part's last use of the
    // buffers, so every part's ev_done has to be reached too before the first buffer is freed
    if (D.produced && D.last_mode == 0)
        for (int p = 0; p < P && e == hipSuccess; p++) e = hipEventSynchronize(D.parts[p]->ev_done);
    // ordered by flags / by one stream: no event carries the last use -- drain the devices
    if (e == hipSuccess && D.produced && D.last_mode >= 1) e = drain_devices(D);
    return e;
}

// part buffers for K columns (grow-only).  EVERY part's stream is drained before ANY buffer goes: a peer may
// still be reading this part's work vector.
static hipError_t grow_buffers(DistState &D, int K) {
    if (K <= D.kcap) return hipSuccess;
    const int P = (int)D.parts.size();
    hipError_t e = drain_handle(D);
    for (int p = 0; p < P && e == hipSuccess; p++) {
        Part &pt = *D.parts[p];
        DeviceGuard g;
        e = g.enter(pt.device);
        if (e != hipSuccess) break;
        pt.free_buffers();
        e = pt.alloc_buffers(D.vlen * (size_t)D.es, std::max(D.plan_n.recv_bytes[p], D.plan_t.recv_bytes[p]), K);
    }
    if (e == hipSuccess) D.kcap = K;
    for (auto &pt : D.parts) pt->w_clean = false;
    return e;
}

// "x and y are ready" on a caller's stream on device `sdev`: one event per device, created at its first use
static hipError_t ready_event(DistState &D, int sdev, hipEvent_t *ev) {
    auto it = D.ev_x.find(sdev);
    if (it == D.ev_x.end()) {
        DeviceGuard g;
        hipError_t e = g.enter(sdev);
        hipEvent_t created = nullptr;
        if (e == hipSuccess) e = hipEventCreateWithFlags(&created, hipEventDisableTiming);
        if (e != hipSuccess) return e;
        it = D.ev_x.emplace(sdev, created).first;
    }
    *ev = it->second;
    return hipSuccess;
}

// (in a function that returns a bsm status and has `hipError_t e` in scope)
#define DCHECK(call, what)                             \
    do {                                               \
        e = (call);                                    \
        if (e != hipSuccess) return hip_fail(e, what); \
    } while (0)

// test hook (unexported in the header, like bsm_debug_move_image_array): the n-th fan-out from now fails between its two
// phases, the way a launch error would (tests/test_gpu_multidevice.py: the product after it must not hang)
static std::atomic<int> g_fail_countdown{-1};
extern "C" void bsm_debug_dist_fail_after(int n) { g_fail_countdown.store(n); }
static bool injected_failure() {
    int c = g_fail_countdown.load();
    if (c < 0) return false;
    return g_fail_countdown.fetch_sub(1) == 0;
}

namespace {

// How the steps of ONE product are ordered across streams, decided once per product: "recorded" / "waited for" is an
// event, or (flags) the product's sequence number in a counter (DistState::flags), or nothing at all.
struct Ordering {
    // 0 events, 1 flags, 2 nothing at all (every part AND the caller's vectors on one stream of one device: stream order
    // is the order).  The forms do not see each other: fan_out drains every device where the form changes.
    const int mode;
    uint64_t *const F;
    // what a wait for the PREVIOUS product's delivery / for a step of THIS product compares a counter with.
    // (the counters only ever hold numbers of products ordered by flags: a product ordered by events in between must not
    // consume one, or the next one would wait for a value nobody writes)
    const uint64_t prev_seq, seq;

    // single: everything on ONE stream of one device; several_streams: the parts' own work is spread over streams
    // (flags pay where streams wait for each other).  The copy path is the events form: (D, false, false).
    Ordering(DistState &D, bool single, bool several_streams)
        : mode(single ? 2 : (D.use_flags && several_streams ? 1 : 0)), F(D.flags), prev_seq(D.seq),
          seq(mode == 1 ? ++D.seq : D.seq) {}

    hipError_t signal(hipEvent_t ev, int flag, hipStream_t st) const {
        if (mode == 2) return hipSuccess;
        return mode == 1 ? hipStreamWriteValue64(st, F + flag, seq, 0) : hipEventRecord(ev, st);
    }
    hipError_t await(hipStream_t st, hipEvent_t ev, int flag, uint64_t value) const {
        if (mode == 2) return hipSuccess;
        return mode == 1 ? hipStreamWaitValue64(st, F + flag, value, hipStreamWaitValueGte, ~(uint64_t)0)
                         : hipStreamWaitEvent(st, ev, 0);
    }
};

// One part's share of one phase of `prod`, on the calling thread (bind: enter the part's device first; a worker thread
// is bound to it already).
template <typename Product> static int issue_part(DistState &D, Product &prod, int ph, int p, bool bind) {
    hipError_t e = hipSuccess;
    DeviceGuard g;
    if (bind) DCHECK(g.enter(D.parts[p]->device), "hipSetDevice");
    return ph == 0 ? prod.first_phase(p) : prod.second_phase(p);
}

template <typename Product> static int issue(DistState &D, int K, Product &prod) {
    const int P = (int)D.parts.size();
    const int mode = prod.order.mode;
    const hipStream_t single = prod.single_stream();
    hipError_t e = hipSuccess;
    DCHECK(grow_buffers(D, K), "multi-device buffers");
    if (D.last_mode >= 0 && (D.last_mode != mode || (mode == 2 && D.last_single_stream != single)))
        DCHECK(drain_devices(D), "hipDeviceSynchronize");
    D.last_mode = mode;
    D.last_single_stream = mode == 2 ? single : nullptr;
    int rc = prod.before();
    for (int ph = 0; ph < 2 && rc == BSM_OK; ph++) {
        if (ph == 1 && injected_failure()) return hip_fail(hipErrorUnknown, "injected failure between the phases of a fan-out");
        auto on_worker = [&D, &prod, ph](int p) { return issue_part(D, prod, ph, p, false); };
        if (D.workers)
            rc = D.workers->run(on_worker);
        else
            for (int p = 0; p < P && rc == BSM_OK; p++) rc = issue_part(D, prod, ph, p, true);
    }
    if (rc != BSM_OK) return rc;
    D.produced = true;
    return prod.after();
}

// The frame of every product of a multi-device handle.  The drivers (FusedProduct, CopyProduct) supply only what
// differs between them: what they issue ahead of the parts (before), the work of a part in each phase (first_phase,
// second_phase), and what follows once every part's work has been issued (after).
//  - The part buffers are grown to K columns.
//  - prod.order.mode: how the product is ordered -- 0 events, 1 flags, 2 nothing at all (every part AND the caller's
//    vectors on the stream prod.single_stream() of one device: stream order is the order).  The forms do not see each
//    other: a change of form (e.g. the copy path of a host vector in between), or mode 2 on another stream, drains
//    every device first.
//  - The issue of every part's work is two phases with a host barrier in between (a stream can only wait for an event or
//    a counter value that HAS been written): first_phase(p) for every part, then second_phase(p).  Run inline by
//    the calling thread (bind: enter the part's device first), or from five parts on by one persistent worker thread
//    per device, bound to it once (the host-side issue cost no longer grows with the number of GPUs).
// What is left behind when a fan-out fails half-way: events degrade by themselves (an event that was never recorded
// counts as complete); sequence counters do not: the failed product has consumed a number, wait packets for it may
// already be queued, and the write packets that would release them were never issued -- the next product's
// wait_previous() would wait for flag >= seq forever and the drain of a mode change would block the host.  So on any
// error the host writes the product's number into every counter (coherent pinned memory: the queued waits fall through),
// drains the devices and leaves the handle as after create: no ordering form remembered, no delivery to wait for, work
// vectors "unknown" (the next fused product clears them once).
template <typename Product> static int fan_out(DistState &D, int K, Product &prod) {
    const int P = (int)D.parts.size();
    const int rc = issue(D, K, prod);
    if (rc == BSM_OK) return rc;
    if (D.flags) {
        volatile uint64_t *F = D.flags;
        for (int i = 0; i < 3 * P + 1; i++)
            if (F[i] < D.seq) F[i] = D.seq;
        __sync_synchronize();
    }
    (void)drain_devices(D);
    (void)hipGetLastError();
    for (auto &pt : D.parts) pt->w_clean = false;
    D.last_mode = -1;
    D.last_single_stream = nullptr;
    D.produced = false;
    return rc;
}

// ---- the fused path: device-resident vectors, every device of the context peer-accessible ----------------
// Where a part finds the x entries it reads, and where it delivers its y entries.  bsm_mul: ONE source (the
// caller's x) and one destination (the caller's y), on the caller's stream.  bsm_mul_parts: part q HOLDS the
// x entries plan.in[q] and receives the y entries plan.out[q], on its own stream.
struct VecSource {
    const char *base;   // virtual base: entry i of the global vector at base + i * es
    Range valid;        // entries this source holds
    int device;         // where the MEMORY lives (decides reading in place)
    int sdev;           // where the STREAM lives (a NULL stream is a different stream on every device): events of
                        // this source are recorded there, and "same stream" means the same stream on that device
    hipStream_t stream; // where the entries are produced
    hipEvent_t ready;   // recorded on `stream` at the start of the call
    int strided;        // column k of a multi-RHS batch at + k * ldx (else the source holds one column)
    int ready_flag = -1;  // flags mode: the counter that stands for `ready`
};
struct VecDest {
    char *base;  // virtual base of the y entries
    int device;  // where the memory lives (decides multiplying straight into y)
    int sdev;    // where the stream lives
    hipStream_t stream;
    hipEvent_t ready;
    int ready_flag = -1;
};

// Up to kMaxVecPieces pieces for one launch of a fetch / finish kernel.  add() hands a full set to `flush` first (more
// pieces than one launch takes); the caller launches what is left in pc[0..n).
struct PieceBatch {
    VecPieces pc;
    int n = 0;
    template <typename Flush> hipError_t add(const void *base, Range r, int strided, Flush &&flush) {
        if (n == kMaxVecPieces) {
            hipError_t e = flush(pc, n);
            if (e != hipSuccess) return e;
            n = 0;
        }
        pc.base[n] = base;
        pc.lo[n] = r.lo;
        pc.hi[n] = r.hi;
        pc.strided[n] = strided;
        n++;
        return hipSuccess;
    }
};

// One product on the fused path.  The constructor decides everything that does not depend on issuing: the plan, the
// stream of every part (run), the Ordering, and which parts multiply straight into y (direct).  fan_out then calls
// before(), first_phase(p) for every part, second_phase(p) for every part, after().  When any of them fails, fan_out
// releases every counter from the host (a number this product's Ordering consumed may already be waited for), drains the
// devices and forgets the ordering form -- nothing here has to undo anything.
struct FusedProduct {
    DistState &D;
    const int P, K;
    const Plan &pl;
    const bool opT, conj;
    const size_t es, vlen;
    const std::vector<VecSource> &src;
    const long long ldx;
    const std::vector<VecDest> &dst;
    const long long ldy;
    const void *const alpha, *const beta;
    const int beta_strong_zero;
    const std::vector<hipStream_t> run;  // the stream part p's work is issued on
    const bool several_streams;          // the parts' work is spread over more than one stream
    const Ordering order;
    const bool rezero;  // this product leaves the work vectors it uses zero again
    const void *one;    // 1 of the vector type
    std::vector<char> direct;  // part p multiplies straight into y (multiplies_into_y)

    FusedProduct(DistState &D_, int op, int K_, const std::vector<VecSource> &src_, long long ldx_, const std::vector<VecDest> &dst_,
                 long long ldy_, const void *alpha_, const void *beta_, int beta_strong_zero_)
        : D(D_), P((int)D_.parts.size()), K(K_), pl((op == BSM_OP_N || D_.symmetric) ? D_.plan_n : D_.plan_t), opT(op != BSM_OP_N),
          conj(op == BSM_OP_C), es((size_t)D_.es), vlen(D_.vlen), src(src_), ldx(ldx_), dst(dst_), ldy(ldy_), alpha(alpha_),
          beta(beta_), beta_strong_zero(beta_strong_zero_), run(part_streams()), several_streams(on_several_streams()),
          order(D_, on_one_stream(), several_streams), rezero(D_.rezero), direct((size_t)P, 0) {
        static const float kOneF[2] = {1.f, 0.f};
        static const double kOneD[2] = {1.0, 0.0};
        one = (D.dtype == 0 || D.dtype == 2) ? (const void *)kOneF : (const void *)kOneD;
        for (int p = 0; p < P; p++) direct[p] = multiplies_into_y(p);
    }

    // the destination of part p: the caller's y (bsm_mul), or the part's own slice (bsm_mul_parts)
    const VecDest &dest(int p) const { return dst[dst.size() == 1 ? 0 : (size_t)p]; }
    // (fan_out: the stream of a product that orders nothing at all)
    hipStream_t single_stream() const { return run[0]; }

    // The stream a part's work is issued on.  bsm_mul_parts: the caller's stream of that part -- local work needs
    // no cross-stream hop at all, only what depends on a PEER waits for an event.  bsm_mul: the first part that
    // lives on the caller's device works on the caller's stream for the same reason (the hops of the other
    // parts then overlap with it); the others use their own streams.
    std::vector<hipStream_t> part_streams() const {
        std::vector<hipStream_t> r((size_t)P);
        bool taken = false;
        for (int p = 0; p < P; p++) {
            const VecDest &yd = dest(p);
            // (bsm_mul: EVERY part on the caller's device works on the caller's stream -- parts that share a device gain
            // nothing from streams of their own, and each one costs two cross-stream hops per product)
            const bool mine = yd.sdev == D.parts[p]->device && (dst.size() > 1 || !taken || D.one_stream);
            r[p] = mine ? yd.stream : D.parts[p]->stream;
            if (mine) taken = true;
        }
        return r;
    }
    // flags pay where streams wait for each other; a product whose parts all work on ONE stream orders nothing at all
    // (on_one_stream)
    bool on_several_streams() const {
        bool several = false;
        for (int p = 1; p < P; p++) several = several || run[p] != run[0] || D.parts[p]->device != D.parts[0]->device;
        return several;
    }
    // everything on ONE stream of one device -- the parts and the caller's vectors (one part, or partitioned vectors
    // driven from one stream of one virtual device): stream order is all the ordering there is to do, no event is
    // recorded and none waited for (every record is a barrier packet between two launches: one part through a
    // context cost +15 us over the plain handle, tools/distbench.py)
    bool on_one_stream() const {
        bool single = !several_streams;
        for (const VecSource &s : src) single = single && s.stream == run[0] && s.sdev == D.parts[0]->device;
        for (const VecDest &d : dst) single = single && d.stream == run[0] && d.sdev == D.parts[0]->device;
        return single;
    }

    // A part that neither sends nor receives a y segment (VBCRS forward: block rows own disjoint y ranges,
    // reference src/vbcrs.jl:275-283) multiplies straight into the caller's y -- beta fused, no work vector,
    // no delivery launch.  Four conditions:
    //  1. y lies on the part's OWN device (and the part has an image): accumulate-mode images add with hardware fp
    //     atomics, which are not relied upon across xGMI; a remote y receives plain stores from the finish kernel instead;
    //  2. the rows it must define are exactly the rows it delivers (zr == out): nothing of its product lies outside
    //     its own slice of y;
    //  3. no transfer leaves it and none arrives: there is nothing for a finish kernel to add;
    //  4. not the interleaved multi-RHS pass across streams: that pass ends in Y = beta * Y + W over the part's rows
    //     and Y += W -- a plain read-modify-write of zeros -- over every OTHER row of y: into the caller's y that would
    //     race with the part that owns those rows whenever the two work on different streams.  Such a part goes through
    //     its work vector, whose delivery touches its own rows only.
    bool multiplies_into_y(int p) const {
        const Part &pt = *D.parts[p];
        bool alone = pt.has_image && dest(p).device == pt.device && pl.zr[p].lo == pl.out[p].lo && pl.zr[p].hi == pl.out[p].hi;
        for (const Transfer &t : pl.transfers) alone = alone && t.from != p && t.to != p;
        return alone && !(several_streams && takes_il(pt, opT, K));
    }

    // part p's stream waits for a step of THIS product recorded on `recorded_on`
    // (a NULL stream is a different stream on every device: "same stream" needs the same device too)
    hipError_t wait_for(int p, hipEvent_t ev, int flag, hipStream_t recorded_on, int recorded_dev) const {
        if (recorded_on == run[p] && recorded_dev == D.parts[p]->device) return hipSuccess;  // same stream: already ordered
        return order.await(run[p], ev, flag, order.seq);
    }

    // "x (and the incoming y) are ready" on every stream that produces them: each (event, counter) once
    int before() {
        hipError_t e = hipSuccess;
        std::vector<std::pair<hipEvent_t, int>> done;
        auto record = [&](hipEvent_t ev, int flag, hipStream_t st, int dev) -> hipError_t {
            for (const auto &d : done)
                if (d.first == ev && d.second == flag) return hipSuccess;
            done.emplace_back(ev, flag);
            DeviceGuard g;
            hipError_t e2 = g.enter(dev);
            return e2 == hipSuccess ? order.signal(ev, flag, st) : e2;
        };
        for (const VecSource &s : src) DCHECK(record(s.ready, s.ready_flag, s.stream, s.sdev), "record: inputs ready");
        for (const VecDest &d : dst) DCHECK(record(d.ready, d.ready_flag, d.stream, d.sdev), "record: inputs ready");
        return BSM_OK;
    }

    // Part p's stream waits for the PREVIOUS product of the handle: the peers that read this part's work vector then
    // have finished (their ev_done carries that product's record until second_phase of THIS product re-records it,
    // after a host barrier), and so has its own previous delivery.
    // (flags: the previous product's number; a first fused product after copy-path ones was drained by
    // fan_out.  Every wait is a packet in front of the product: each delivery once, and none for a delivery
    // that was recorded on this very stream)
    int wait_previous(int p) const {
        if (!D.produced || order.mode == 2) return BSM_OK;
        hipError_t e = hipSuccess;
        const Part &pt = *D.parts[p];
        hipStream_t st = run[(size_t)p];
        std::vector<int> waited;
        auto previous = [&](int q) -> hipError_t {
            const Part &pq = *D.parts[q];
            if (pq.done_stream == st && pq.device == pt.device) return hipSuccess;
            for (int w : waited)
                if (w == q) return hipSuccess;
            waited.push_back(q);
            return order.await(st, pq.ev_done, 2 * P + q, order.prev_seq);
        };
        for (const Transfer &t : D.plan_n.transfers)
            if (t.from == p) DCHECK(previous(t.to), "wait: previous delivery");
        for (const Transfer &t : D.plan_t.transfers)
            if (t.from == p) DCHECK(previous(t.to), "wait: previous delivery");
        DCHECK(previous(p), "wait: previous delivery");  // its own previous delivery (another stream, perhaps)
        if (order.mode == 0 && D.ev_tail) DCHECK(hipStreamWaitEvent(st, D.ev_tail, 0), "hipStreamWaitEvent");
        return BSM_OK;
    }

    // Where part p's product reads x: the caller's x in place when everything it reads lies on its own device, else
    // its x buffer, gathered from the sources that hold pieces of it (one launch; waits for each such source).
    int fetch_x(int p, const void **xp, long long *xld) const {
        hipError_t e = hipSuccess;
        Part &pt = *D.parts[p];
        hipStream_t st = run[(size_t)p];
        const Range xr = pl.xr[p];
        *xp = pt.d_x;
        *xld = (long long)vlen;
        auto fetch = [&](const VecPieces &pc, int np) { return launch_vec_fetch(D.dtype, pt.d_x, (long long)vlen, pc, np, ldx, K, st); };
        PieceBatch pieces;
        for (const VecSource &s : src) {
            const Range o = isect(s.valid, xr);
            if (o.empty()) continue;
            DCHECK(wait_for(p, s.ready, s.ready_flag, s.stream, s.sdev), "wait: x ready");
            if (o.lo == xr.lo && o.hi == xr.hi && s.device == pt.device) {  // everything it reads lies on its own device
                *xp = s.base;
                *xld = s.strided ? ldx : 0;
                return BSM_OK;
            }
            DCHECK(pieces.add(s.base, o, s.strided, fetch), "x fetch");
        }
        if (pieces.n) DCHECK(fetch(pieces.pc, pieces.n), "x fetch");
        return BSM_OK;
    }

    // Zero-keeping: part p's work vector is zero already unless its contents are unknown (cleared once, whole buffer);
    // either way it is not known to be zero again until the whole product has been issued (after).  Without
    // zero-keeping nothing is cleared here.
    hipError_t clear_unless_zero(Part &pt, hipStream_t st) const {
        hipError_t e = hipSuccess;
        if (rezero && !pt.w_clean) e = hipMemsetAsync(pt.d_w, 0, (size_t)D.kcap * vlen * es, st);
        pt.w_clean = false;  // (until the whole product has been issued)
        return e;
    }

    // phase 0 (part p): wait for the previous product's readers of its work vector (wait_previous), for the incoming y
    // and for every source of the x pieces it reads (fetch_x); gather those pieces (one launch), local product; record
    // "product done" (ev_prod / counter P + p).
    int first_phase(int p) {
        hipError_t e = hipSuccess;
        Part &pt = *D.parts[p];
        const VecDest &yd = dest(p);
        hipStream_t st = run[(size_t)p];
        int rc = wait_previous(p);
        if (rc != BSM_OK) return rc;
        DCHECK(wait_for(p, yd.ready, yd.ready_flag, yd.stream, yd.sdev), "wait: y ready");  // the incoming y (numeric beta) / its buffer
        const Range zr = pl.zr[p];
        if (pt.has_image) {
            const void *xp;
            long long xld;
            rc = fetch_x(p, &xp, &xld);
            if (rc != BSM_OK) return rc;
            const long long z[2] = {zr.lo, zr.hi};
            void *target = direct[p] ? (void *)yd.base : pt.d_w;
            const long long tld = direct[p] ? ldy : (long long)vlen;
            // into the work vector: `w = 0` first -- or, when the finish kernels keep it zero, plain accumulation
            // (beta = 1: no launch in front; unknown contents are cleared once, whole buffer)
            if (!direct[p]) DCHECK(clear_unless_zero(pt, st), "memset");
            const void *b = direct[p] ? beta : (rezero ? one : nullptr);
            const int sz = direct[p] ? beta_strong_zero : (rezero ? 0 : 1);
            DCHECK(launch_mul(pt.img, opT, conj, K, xp, xld, target, tld, alpha, b, sz, st, false, z, part_il(pt, opT, K),
                              pt.img.dtype),
                   "kernel launch");
        } else if (rezero) {
            DCHECK(clear_unless_zero(pt, st), "memset");
        } else if (!zr.empty()) {
            for (int k = 0; k < K; k++)
                DCHECK(hipMemsetAsync((char *)pt.d_w + ((size_t)k * vlen + zr.lo) * es, 0, (size_t)zr.len() * es, st), "memset");
        }
        DCHECK(order.signal(pt.ev_prod, P + p, st), "record: product done");
        return BSM_OK;
    }

    // phase 1 (part p): wait for "product done" of every peer that produced y segments for its rows, add those segments
    // (read from the peers' work vectors) and deliver (one launch); record "delivery done" (ev_done / counter 2 P + p).
    // Its own product needs no wait: same stream.
    int second_phase(int p) {
        hipError_t e = hipSuccess;
        Part &pt = *D.parts[p];
        hipStream_t st = run[(size_t)p];
        const Range o = pl.out[p];
        // more peers than one launch takes: fold these into the work vector first
        auto fold = [&](const VecPieces &pc, int np) {
            return launch_vec_finish(D.dtype, nullptr, 0, pt.d_w, (long long)vlen, pc, np, o.lo, o.hi, nullptr, 1, 1, rezero, K, st);
        };
        PieceBatch pieces;
        for (const Transfer &t : pl.transfers) {
            if (t.to != p) continue;
            Part &from = *D.parts[t.from];
            DCHECK(wait_for(p, from.ev_prod, P + t.from, run[(size_t)t.from], from.device), "wait: peer's product");
            DCHECK(pieces.add(from.d_w, t.range, 1, fold), "halo add");
        }
        if (!o.empty() && !direct[p])
            DCHECK(launch_vec_finish(D.dtype, dest(p).base, ldy, pt.d_w, (long long)vlen, pieces.pc, pieces.n, o.lo, o.hi, beta,
                                     beta_strong_zero, 0, rezero, K, st), "y delivery");
        DCHECK(order.signal(pt.ev_done, 2 * P + p, st), "record: delivery done");
        pt.done_stream = st;
        return BSM_OK;
    }

    int after() {
        hipError_t e = hipSuccess;
        for (int p = 0; p < P; p++)
            if (!direct[p]) D.parts[p]->w_clean = rezero;
        // the consumers of y continue when the parts that deliver to them are done
        for (int q = 0; q < P; q++) {
            const VecDest &yd = dest(q);
            if (yd.stream == run[(size_t)q] && yd.sdev == D.parts[q]->device) continue;  // delivered on the consumer's own stream
            DeviceGuard g;
            DCHECK(g.enter(yd.sdev), "hipSetDevice");
            DCHECK(order.await(yd.stream, D.parts[q]->ev_done, 2 * P + q, order.seq), "wait: delivery");
        }
        return BSM_OK;
    }
};

static int dist_mul_fused(DistState &D, int op, int K, const std::vector<VecSource> &src, long long ldx,
                          const std::vector<VecDest> &dst, long long ldy, const void *alpha, const void *beta,
                          int beta_strong_zero) {
    FusedProduct prod(D, op, K, src, ldx, dst, ldy, alpha, beta, beta_strong_zero);
    return fan_out(D, K, prod);
}

// a bsm_mul / bsm_mul_multi call, resolved once for whichever driver runs it
struct Call {
    bool host;               // BSM_MEM_HOST (else BSM_MEM_DEVICE)
    int xdev, ydev, sdev;    // where x, y and the caller's stream live (host vectors: -1, -1, the current device)
    hipStream_t stream;
    hipEvent_t ready;        // device vectors: "x and y are ready" on `stream` (ready_event), recorded by the driver
};

// ---- the copy path: host vectors, devices without peer access, BSM_DIST_COPIES=1 ----------------------------
// K <= 16 right-hand sides in one fan-out (K = 1: bsm_mul).  X / Y: column k at x + k * ldx / y + k * ldy
// elements.  The part buffers hold column k at k * vlen elements.  One stream per device:
//   phase 0 (part p): x to its device, local product, record ev_prod
//   phase 1 (part q): the y segments other parts produced for q's rows (peer copy over xGMI + add),
//                     then q's owned range to the caller's y, record ev_done
struct CopyProduct {
    DistState &D;
    const int P, K;
    const Plan &pl;
    const bool opT, conj;
    const size_t es;
    const long long ylen;
    const size_t vlen;  // elements per column of the part buffers
    const void *const x;
    const char *const xb;
    const long long ldx;
    char *const yb;
    const long long ldy;
    const void *const alpha, *beta;
    const Call &c;
    const bool host, numeric_beta;
    const size_t res_need;  // staging of numeric-beta results: column k at k * ylen
    const Ordering order;   // the events form (its records and waits are spelled out below)
    std::vector<char> late_flag;  // numeric beta, remote part, y on a device: combined in after()

    CopyProduct(DistState &D_, int op, int K_, const void *x_, long long ldx_, void *y_, long long ldy_, const void *alpha_,
                const void *beta_, int beta_strong_zero, const Call &c_)
        : D(D_), P((int)D_.parts.size()), K(K_), pl((op == BSM_OP_N || D_.symmetric) ? D_.plan_n : D_.plan_t), opT(op != BSM_OP_N),
          conj(op == BSM_OP_C), es((size_t)D_.es), ylen((op == BSM_OP_N) ? D_.nrows : D_.ncols), vlen(D_.vlen), x(x_),
          xb((const char *)x_), ldx(ldx_), yb((char *)y_), ldy(ldy_), alpha(alpha_), beta(beta_), c(c_), host(c_.host),
          numeric_beta(!beta_strong_zero), res_need((size_t)ylen * es * K), order(D_, false, false), late_flag((size_t)P, 0) {
        static const double kZero[2] = {0.0, 0.0};
        if (!beta) beta = kZero;  // "NULL = 0" of include/bsm_rocm.h, also where this file reads beta itself
    }

    hipStream_t single_stream() const { return nullptr; }

    int before() {
        hipError_t e = hipSuccess;
        for (auto &pt : D.parts) pt->w_clean = false;  // (this path leaves its partial sums in the work vectors)
        if (!host) {
            DeviceGuard g;
            DCHECK(g.enter(c.sdev), "hipSetDevice");
            DCHECK(hipEventRecord(c.ready, c.stream), "hipEventRecord");  // x (and the incoming y) are ready
        }
        if (numeric_beta && host && D.h_res.size() < res_need) D.h_res.resize(res_need);
        if (numeric_beta && !host) {
            bool remote = false;
            for (int q = 0; q < P; q++) remote |= (!pl.out[q].empty() && D.parts[q]->device != c.ydev);
            if (remote && (D.res_dev != c.ydev || D.res_bytes < res_need)) {
                if (D.d_res) {
                    DeviceGuard g;
                    (void)g.enter(D.res_dev);
                    (void)hipFree(D.d_res);
                    D.d_res = nullptr;
                }
                DeviceGuard g;
                DCHECK(g.enter(c.ydev), "hipSetDevice");
                DCHECK(hipMalloc(&D.d_res, res_need + 16), "hipMalloc(result staging)");
                D.res_dev = c.ydev;
                D.res_bytes = res_need;
            }
        }
        return BSM_OK;
    }

    int first_phase(int p) {
        hipError_t e = hipSuccess;  // (per invocation: the phases of different parts run concurrently)
        Part &pt = *D.parts[p];
        // the previous product of this handle -- peers still reading this part's work vector, the late
        // combine on the caller's stream reading the result staging -- is complete before this one starts
        if (D.produced) {
            for (int q = 0; q < P; q++) DCHECK(hipStreamWaitEvent(pt.stream, D.parts[q]->ev_done, 0), "hipStreamWaitEvent");
            if (D.ev_tail) DCHECK(hipStreamWaitEvent(pt.stream, D.ev_tail, 0), "hipStreamWaitEvent");
        }
        if (c.ready) DCHECK(hipStreamWaitEvent(pt.stream, c.ready, 0), "hipStreamWaitEvent");
        const Range zr = pl.zr[p];
        if (pt.has_image) {
            const Range xr = pl.xr[p];
            const void *xp = pt.d_x;
            long long xld = (long long)vlen;
            if (!host && c.xdev == pt.device) {
                xp = x;  // same device: the local product reads the caller's x directly
                xld = ldx;
            } else {
                for (int k = 0; k < K; k++) {
                    char *dst = (char *)pt.d_x + ((size_t)k * vlen + xr.lo) * es;
                    const char *src = xb + ((size_t)k * ldx + xr.lo) * es;
                    if (host)
                        DCHECK(hipMemcpyAsync(dst, src, (size_t)xr.len() * es, hipMemcpyHostToDevice, pt.stream), "x upload");
                    else
                        DCHECK(copy_between(dst, pt.device, src, c.xdev, (size_t)xr.len() * es, pt.stream), "x peer copy");
                }
            }
            const long long z[2] = {zr.lo, zr.hi};
            DCHECK(launch_mul(pt.img, opT, conj, K, xp, xld, pt.d_w, (long long)vlen, alpha, nullptr, 1, pt.stream,
                              pt.img.d_ws != nullptr, z, part_il(pt, opT, K), pt.img.dtype), "kernel launch");
        } else if (!zr.empty()) {
            for (int k = 0; k < K; k++)
                DCHECK(hipMemsetAsync((char *)pt.d_w + ((size_t)k * vlen + zr.lo) * es, 0, (size_t)zr.len() * es, pt.stream),
                       "memset");
        }
        DCHECK(hipEventRecord(pt.ev_prod, pt.stream), "hipEventRecord");
        return BSM_OK;
    }

    int second_phase(int p) {
        hipError_t e = hipSuccess;
        Part &pt = *D.parts[p];
        // 3: y segments produced for rows of THIS part: peer copy over xGMI + local add
        const size_t rstride = std::max(D.plan_n.recv_bytes[p], D.plan_t.recv_bytes[p]);
        for (const Transfer &t : pl.transfers) {
            if (t.to != p) continue;
            Part &src = *D.parts[t.from];
            DCHECK(hipStreamWaitEvent(pt.stream, src.ev_prod, 0), "hipStreamWaitEvent");
            for (int k = 0; k < K; k++) {
                char *rb = (char *)pt.d_recv + (size_t)k * rstride + t.recv_off;
                const size_t off = ((size_t)k * vlen + t.range.lo) * es;
                DCHECK(copy_between(rb, pt.device, (char *)src.d_w + off, src.device, (size_t)t.range.len() * es, pt.stream),
                       "halo peer copy");
                DCHECK(launch_vec_add(D.dtype, (char *)pt.d_w + off, rb, t.range.len(), pt.stream), "halo add");
            }
        }
        // 4: deliver the owned range
        const Range o = pl.out[p];
        if (!o.empty()) {
            const size_t bytes = (size_t)o.len() * es;
            for (int k = 0; k < K; k++) {
                const char *w = (const char *)pt.d_w + ((size_t)k * vlen + o.lo) * es;
                char *yk = yb + ((size_t)k * ldy + o.lo) * es;
                const size_t roff = ((size_t)k * ylen + o.lo) * es;
                if (host) {
                    char *dst = numeric_beta ? D.h_res.data() + roff : yk;
                    DCHECK(hipMemcpyAsync(dst, w, bytes, hipMemcpyDeviceToHost, pt.stream), "y download");
                } else if (!numeric_beta) {
                    DCHECK(copy_between(yk, c.ydev, w, pt.device, bytes, pt.stream), "y peer copy");
                } else if (pt.device == c.ydev) {
                    DCHECK(launch_vec_axpby(D.dtype, yk, w, o.len(), beta, pt.stream), "y combine");
                } else {
                    DCHECK(copy_between((char *)D.d_res + roff, c.ydev, w, pt.device, bytes, pt.stream), "y peer copy");
                    late_flag[p] = 1;
                }
            }
        }
        DCHECK(hipEventRecord(pt.ev_done, pt.stream), "hipEventRecord");
        return BSM_OK;
    }

    int after() { return host ? after_host() : after_device(); }

    // y on the host: every part's stream is waited for, then numeric beta is combined here
    int after_host() {
        hipError_t e = hipSuccess;
        for (int q = 0; q < P; q++) {
            Part &pt = *D.parts[q];
            DeviceGuard g;
            DCHECK(g.enter(pt.device), "hipSetDevice");
            DCHECK(hipStreamSynchronize(pt.stream), "multi-device mul");
        }
        if (numeric_beta) {
            for (int q = 0; q < P; q++) {
                const Range o = pl.out[q];
                if (o.empty()) continue;
                for (int k = 0; k < K; k++) {
                    char *yk = yb + ((size_t)k * ldy + o.lo) * es;
                    const char *rk = D.h_res.data() + ((size_t)k * ylen + o.lo) * es;
                    with_types(D.dtype, [&](auto r, auto, auto nc) {
                        using R = decltype(r);
                        using T = std::conditional_t<decltype(nc)::value == 1, R, std::complex<R>>;
                        host_axpby((T *)yk, (const T *)rk, o.len(), *(const T *)beta);
                    });
                }
            }
        }
        return BSM_OK;
    }

    // y on a device: the caller's stream continues when every part has delivered
    int after_device() {
        hipError_t e = hipSuccess;
        {
            DeviceGuard g;
            DCHECK(g.enter(c.sdev), "hipSetDevice");
            for (int q = 0; q < P; q++) DCHECK(hipStreamWaitEvent(c.stream, D.parts[q]->ev_done, 0), "hipStreamWaitEvent");
        }
        bool any_late = false;
        for (int q = 0; q < P; q++) any_late |= late_flag[q] != 0;
        if (any_late) {
            DeviceGuard g;
            DCHECK(g.enter(c.ydev), "hipSetDevice");
            for (int q = 0; q < P; q++) {
                if (!late_flag[q]) continue;
                const Range o = pl.out[q];
                for (int k = 0; k < K; k++)
                    DCHECK(launch_vec_axpby(D.dtype, yb + ((size_t)k * ldy + o.lo) * es,
                                            (char *)D.d_res + ((size_t)k * ylen + o.lo) * es, o.len(), beta, c.stream), "y combine");
            }
        }
        // the end of this product on the caller's stream: what the next product of the handle waits for
        DeviceGuard g;
        DCHECK(g.enter(c.sdev), "hipSetDevice");
        if (D.ev_tail && D.tail_dev != c.sdev) {
            (void)hipEventDestroy(D.ev_tail);
            D.ev_tail = nullptr;
        }
        if (!D.ev_tail) {
            DCHECK(hipEventCreateWithFlags(&D.ev_tail, hipEventDisableTiming), "hipEventCreate");
            D.tail_dev = c.sdev;
        }
        DCHECK(hipEventRecord(D.ev_tail, c.stream), "hipEventRecord");
        return BSM_OK;
    }
};

static int dist_mul_copies(DistState &D, int op, int K, const void *x, long long ldx, void *y, long long ldy,
                           const void *alpha, const void *beta, int beta_strong_zero, const Call &c) {
    CopyProduct prod(D, op, K, x, ldx, y, ldy, alpha, beta, beta_strong_zero, c);
    return fan_out(D, K, prod);
}

}  // namespace

// a multi-device product issues on several streams and devices and waits for events of earlier products: it cannot be
// recorded into the caller's graph (include/bsm_rocm.h) -- refuse instead of corrupting the capture
static const char kNoCapture[] = "a multi-device handle cannot be captured into a graph";

static int dist_mul_k(bsm_matrix_s *A, int op, int K, const void *x, long long ldx, void *y, long long ldy,
                      const void *alpha, const void *beta, int beta_strong_zero, int memspace, hipStream_t stream) {
    DistState &D = *A->dist;
    std::lock_guard<std::mutex> lock(D.mu);  // one product of a handle is ISSUED at a time (the work vectors are the handle's)
    if (memspace == BSM_MEM_DEVICE && stream && capturing(stream)) return fail(BSM_ERR_UNSUPPORTED, kNoCapture);
    if (memspace != BSM_MEM_HOST && memspace != BSM_MEM_DEVICE) return fail(BSM_ERR_INVALID, "bad memspace");
    Call c{memspace == BSM_MEM_HOST, -1, -1, 0, stream, nullptr};
    hipError_t e = hipGetDevice(&c.sdev);
    if (e != hipSuccess) return hip_fail(e, "hipGetDevice");
    if (!c.host) {
        const int cur = c.sdev;
        c.xdev = pointer_device(x, cur);
        c.ydev = pointer_device(y, cur);
        if (stream && hipStreamGetDevice(stream, &c.sdev) != hipSuccess) {
            (void)hipGetLastError();
            c.sdev = cur;
        }
        e = ready_event(D, c.sdev, &c.ready);
        if (e != hipSuccess) return hip_fail(e, "hipEventCreate");
        bool inside = false, xin = false, yin = false;
        for (const auto &pp : D.parts) {
            inside |= pp->device == c.sdev;
            xin |= pp->device == c.xdev;
            yin |= pp->device == c.ydev;
        }
        if (D.all_peer && inside && xin && yin) {  // x, y and the stream live on devices of the context: everybody can address them
            const long long xlen = (op == BSM_OP_N) ? D.ncols : D.nrows;
            const int P = (int)D.parts.size();
            std::vector<VecSource> src{VecSource{(const char *)x, Range{0, xlen}, c.xdev, c.sdev, stream, c.ready, 1, 3 * P}};
            std::vector<VecDest> dst{VecDest{(char *)y, c.ydev, c.sdev, stream, c.ready, 3 * P}};
            return dist_mul_fused(D, op, K, src, ldx, dst, ldy, alpha, beta, beta_strong_zero);
        }
    }
    return dist_mul_copies(D, op, K, x, ldx, y, ldy, alpha, beta, beta_strong_zero, c);
}

// bsm_mul_parts: x and y PARTITIONED over the devices of the handle (include/bsm_rocm.h)
int dist_mul_parts(bsm_matrix_s *A, int op, const void *const *x_parts, void *const *y_parts, const void *alpha,
                   const void *beta, int beta_strong_zero, void *const *streams) {
    DistState &D = *A->dist;
    std::lock_guard<std::mutex> lock(D.mu);
    if (!D.all_peer)
        return fail(BSM_ERR_UNSUPPORTED, "bsm_mul_parts needs peer access between all devices of the context");
    const int P = (int)D.parts.size();
    const bool along = (op == BSM_OP_N) || D.symmetric;
    const Plan &pl = along ? D.plan_n : D.plan_t;
    const size_t es = (size_t)D.es;
    std::vector<VecSource> src;
    std::vector<VecDest> dst;
    for (int p = 0; p < P; p++) {
        const Part &pt = *D.parts[p];
        const Range in = pl.in[p], out = pl.out[p];
        if ((!in.empty() && !x_parts[p]) || (!out.empty() && !y_parts[p]))
            return fail(BSM_ERR_INVALID, "part " + std::to_string(p) + ": null vector part");
        hipStream_t st = streams ? (hipStream_t)streams[p] : nullptr;
        if (st && capturing(st)) return fail(BSM_ERR_UNSUPPORTED, kNoCapture);  // like bsm_mul (include/bsm_rocm.h)
        src.push_back(VecSource{(const char *)x_parts[p] - (size_t)in.lo * es, in, pt.device, pt.device, st, pt.ev_in, 0, p});
        dst.push_back(VecDest{(char *)y_parts[p] - (size_t)out.lo * es, pt.device, pt.device, st, pt.ev_in, p});
    }
    return dist_mul_fused(D, op, 1, src, 0, dst, 0, alpha, beta, beta_strong_zero);
}
#undef DCHECK

// Y = alpha op(A) X + beta Y: every device streams its part of A ONCE per batch of up to 8 columns
// (bsm_mul_multi's own batching), the exchange and the delivery move the batch's columns together
int dist_mul_multi(bsm_matrix_s *A, int op, long long nrhs, const void *X, long long ldx, void *Y, long long ldy,
                   const void *alpha, const void *beta, int beta_strong_zero, int memspace, hipStream_t stream) {
    const size_t es = (size_t)A->dist->es;
    // batches of 8 columns per fan-out; Float32 / Float64 operators take 9 and more columns 16 at a time (the parts'
    // 16-column matrix-pipe passes, bsm_multi.hip: kMfmaReal)
    const bool real = A->dist->dtype == 0 || A->dist->dtype == 1;
    for (long long k = 0; k < nrhs;) {
        const long long left = nrhs - k;
        const int kb = (int)((real && left >= 9) ? std::min<long long>(16, left) : std::min<long long>(8, left));
        int rc = dist_mul_k(A, op, kb, (const char *)X + (size_t)k * ldx * es, ldx, (char *)Y + (size_t)k * ldy * es, ldy,
                            alpha, beta, beta_strong_zero, memspace, stream);
        if (rc != BSM_OK) return rc;
        k += kb;
    }
    return BSM_OK;
}

}  // namespace bsm
