// bsm_dist.h -- the state of ONE handle spread over the devices of a bsm_ctx_t, shared by bsm_dist.cpp (which builds and
// maintains it: partition, exchange plans, create / destroy / update) and bsm_fanout.cpp (which issues its products).
// Not part of the C ABI.
#pragma once
#include <algorithm>
#include <condition_variable>
#include <map>
#include <thread>

#include "bsm_internal.h"

namespace bsm {

struct Range {  // 0-based [lo, hi)
    long long lo = 0, hi = 0;
    bool empty() const { return hi <= lo; }
    long long len() const { return hi > lo ? hi - lo : 0; }
};
inline Range isect(Range a, Range b) { return Range{std::max(a.lo, b.lo), std::min(a.hi, b.hi)}; }
inline Range hull(Range a, Range b) {
    if (a.empty()) return b;
    if (b.empty()) return a;
    return Range{std::min(a.lo, b.lo), std::max(a.hi, b.hi)};
}

struct Transfer {  // part `from` produced y[range] for rows part `to` owns
    int from, to;
    Range range;
    size_t recv_off;  // byte offset in the receiver's staging buffer
};

// everything that depends on the direction of the product relative to the partition
struct Plan {
    std::vector<Range> xr;    // x entries part p reads
    std::vector<Range> in;    // x entries part p HOLDS when the vectors are partitioned (bsm_mul_parts): a tiling of [0, xlen)
    std::vector<Range> out;   // y entries part p delivers (a tiling of [0, ylen))
    std::vector<Range> zr;    // y entries part p must define in its work vector (touched + out)
    std::vector<Transfer> transfers;
    std::vector<size_t> recv_bytes;
};

// the part's operator on its device (`device` is set for every part; one that holds no block is never built), and what
// the fan-out adds to it
struct Part : LocalOperator {
    bool has_image = false;
    int64_t nblocks = 0;
    Range own;         // rows it owns
    Range rows, cols;  // hull of the row / column indices of its blocks
    hipStream_t stream = nullptr;
    hipEvent_t ev_prod = nullptr, ev_done = nullptr, ev_in = nullptr;
    hipStream_t done_stream = nullptr;  // where ev_done (or its flag) was last recorded, on `device`
    bool w_clean = false;               // d_w is zero everywhere (DistState::rezero)
    void *d_x = nullptr, *d_w = nullptr, *d_recv = nullptr;
    Range colpart;  // the part's share of the COLUMN partition (vectors of length ncols held in parts)
    // The work arrays of the interleaved multi-RHS pass (LocalOperator::il) need no claim here: a part's successive
    // products are ordered by the fan-out itself (a product waits for the part's own previous delivery, or everything
    // runs on one stream).
    bool il_failed = false;  // no memory for them: the ordinary kernels from then on

    // What the part owns beside its operator, made and released with `device` current (bsm_dist.cpp).
    // x and work vector of K columns of vec_bytes each, receive staging of K times recv_bytes (none where nothing is
    // received); the part holds no buffers when this is called
    hipError_t alloc_buffers(size_t vec_bytes, size_t recv_bytes, int K);
    void free_buffers();
    void release_sync();  // the stream and the three events
};

// One persistent thread per part, bound to the part's device once.  run(f) executes f(p) on every
// worker and returns when all are done (first failure wins; its message is handed to the caller's
// thread-local error slot).
class Workers {
  public:
    explicit Workers(const std::vector<int> &devices);
    ~Workers();
    template <typename F> int run(F &f) {
        return run_fn([](void *a, int p) { return (*static_cast<F *>(a))(p); }, &f);
    }

  private:
    using Fn = int (*)(void *, int);
    int run_fn(Fn fn, void *arg);
    void loop(int p, int dev);
    int n_;
    std::vector<std::thread> th_;
    std::mutex mu_;
    std::condition_variable go_, done_;
    uint64_t gen_ = 0;
    int pending_ = 0;
    bool stop_ = false;
    Fn fn_ = nullptr;
    void *arg_ = nullptr;
    std::vector<int> rc_;
    std::vector<std::string> msg_;
};

struct DistState {
    std::unique_ptr<Workers> workers;  // more than two parts: one issuing thread per device
    bsm_ctx_s *ctx = nullptr;
    int dtype = 1, es = 8;
    long long nrows = 0, ncols = 0;
    bool symmetric = false;  // op(A) has A's structure: every op runs ALONG the partition
    std::vector<std::unique_ptr<Part>> parts;
    Plan plan_n, plan_t;
    size_t vlen = 0;  // elements per column of the parts' x / work buffers
    int kcap = 1;     // columns those buffers hold (grows with bsm_mul_multi)
    std::mutex mu;  // one product in flight per handle: the work vectors belong to the handle
    std::map<int, hipEvent_t> ev_x;  // "x and y are ready" on the caller's stream, one event per device
    void *d_res = nullptr;  // numeric beta, y on a device: segments of remote parts wait here
    int res_dev = -1;
    size_t res_bytes = 0;
    std::vector<char> h_res;  // numeric beta, y on the host
    // every pair of the context's devices can address each other's memory: the vector traffic of a product
    // with device-resident vectors runs as two fused kernels per device (fetch / finish) instead of copies
    bool all_peer = false;
    bool produced = false;       // some product has been issued: ev_done / ev_tail carry a record
    hipEvent_t ev_tail = nullptr;  // end of the last copy-path product on its caller's stream
    int tail_dev = -1;
    // Cross-stream ordering of the fused path by FLAGS instead of events (BSM_DIST_FLAGS): a product has a sequence
    // number, "recorded" = hipStreamWriteValue64(stream, flag, seq), "waited for" = hipStreamWaitValue64(stream, flag,
    // seq, >=) on 64-bit counters in coherent pinned host memory (every device's command processor can poll them).
    // tools/hop_latency.hip: a dependency between two streams costs ~6 us this way against ~12.4 us through
    // hipEventRecord + hipStreamWaitEvent, and a product has two to three of them on its critical path.
    // flag[k * P + p], k = 0 "inputs of part p ready", 1 "product of part p done", 2 "delivery of part p done";
    // flag[3 P] "x / y of a full-vector call ready".
    bool use_flags = false;
    uint64_t *flags = nullptr;
    uint64_t seq = 0;
    // 0 events, 1 flags, 2 nothing at all (every part AND the caller's vectors on one stream of one device: stream order
    // is the order): a change drains every device first (the forms do not see each other)
    int last_mode = -1;
    hipStream_t last_single_stream = nullptr;  // mode 2: the stream (a different one next time drains as well)
    // The work vectors of the fused path are ZERO between two products: the finish kernels write zeros behind what they
    // read (every entry a product writes is read exactly once -- by its owner's finish kernel or by the peer it is
    // for), so a product accumulates into its work vector without the `w = 0` launch in front (one dependent launch
    // per part off the critical path).  Part::w_clean = false: unknown contents (fresh buffers, a copy-path product,
    // a failed product) -- the next fused product that uses the vector clears the whole buffer once.
    bool rezero = true;  // BSM_DIST_REZERO=0: the zeroing launch in front of every product, as before (A/B, diagnosis)
    bool one_stream = true;  // BSM_DIST_ONE_STREAM=0: parts that share the caller's device still get streams of their own
};

// Waits until nothing of any earlier product of the handle can still be running or reading a part's buffers
// (bsm_fanout.cpp; dist_update stands outside the fan-out and drains with it).
hipError_t drain_handle(DistState &D);

}  // namespace bsm
