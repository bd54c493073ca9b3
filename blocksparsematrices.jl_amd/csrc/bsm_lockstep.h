// bsm_lockstep.h -- the host side that the lockstep solver objects (bsm_cg.cpp: bsm_cg_*, bsm_bicgstab.cpp: bsm_bicgstab_*,
// bsm_gmres_multi.cpp: bsm_gmres_multi_* and its one-column front bsm_gmres_*, bsm_minres.cpp: bsm_minres_*, bsm_lsqr.cpp:
// bsm_lsqr_*; include/bsm_rocm.h) share: what a solver object
// holds whatever its method, the (handle, vector) pairings and the multi-column product on the workspace, create from the
// refusals to the one device allocation (lockstep_create: a method writes its layout once, as a function on a Carve), the
// start of x, the ring of pinned record slots (RecordRing), what the host takes from a record and reports from the last
// one, the look-ahead loop that reads one record per iteration (lockstep_run; the GMRES solvers, whose iterations come in
// cycles, drive the same ring in their own loop), the refusals of solve and the staging of host matrices.
#pragma once
#include <hip/hip_runtime_api.h>

#include <algorithm>
#include <cstdint>
#include <cstring>
#include <new>
#include <string>

#include "bsm_cg.h"
#include "bsm_internal.h"

// return from the enclosing function with the failure of a HIP call / of a call that returns a BSM status
#define HIP_TRY(call)                                     \
    do {                                                  \
        const hipError_t e_ = (call);                     \
        if (e_ != hipSuccess) return hip_fail(e_, #call); \
    } while (0)
#define RC_TRY(call)                  \
    do {                              \
        const int rc_ = (call);       \
        if (rc_ != BSM_OK) return rc_; \
    } while (0)

namespace bsm {

constexpr int kLockstepRing = 4;  // pinned record slots and events: at most two records are in flight

struct LockstepSolver {
    bsm_matrix_s *A = nullptr, *M = nullptr;
    int opA = 0, opM = 0, vt = 0, kmax = 0, device = 0;
    bool a_cvec = false, m_cvec = false;
    int64_t n = 0, ld = 0;  // rows of X = cols(op(A)), their leading dimension in the workspace
    int G = 1;
    // the same of the vectors of B's length, rows(op(A)): n, ld and G again for the solvers of square systems
    int64_t rows_b = 0, ld_b = 0;
    int G_b = 1;
    // ONE device allocation (info.workspace): the method's vectors as ld x kmax, its partials, the state
    void *ws = nullptr;
    int64_t ws_bytes = 0;
    CgState *state = nullptr;
    const CgRecord *rec = nullptr;  // the device record of a method with a state of its own (null: state->rec)
    CgRecord *slots = nullptr;      // pinned, kLockstepRing of them
    hipEvent_t ev[kLockstepRing] = {};
    // BSM_MEM_HOST solves: device copies of B (rows_b x kmax) and X (n x kmax), allocated at the first one
    void *hb = nullptr, *hx = nullptr;

    void release() {
        if (ws) (void)hipFree(ws);
        if (hb) (void)hipFree(hb);
        if (hx) (void)hipFree(hx);
        if (slots) (void)hipHostFree(slots);
        for (hipEvent_t &e : ev) {
            if (e) (void)hipEventDestroy(e);
            e = nullptr;
        }
        ws = hb = hx = nullptr;
        slots = nullptr;
    }
};

// how `H` is applied to vectors of type vt: 0 bsm_mul_multi, 1 bsm_mul_multi_cvec, -1 not at all
inline int pairing(const bsm_matrix_s *H, int vt) {
    const int dt = H->an.dtype;
    if (dt < 0 || dt > 5) return -1;
    if (vec_type(dt) == vt) return 0;
    if ((dt == BSM_F32 && vt == BSM_C64) || (dt == BSM_F64 && vt == BSM_C128)) return 1;
    return -1;
}

// Y = op(H) X on nrhs columns of the workspace (leading dimensions ldx of X, ldy of Y), Y overwritten
inline int apply(bsm_matrix_s *H, int op, bool cvec, int nrhs, int64_t ldx, int64_t ldy, int vt, const void *X, void *Y, hipStream_t st) {
    const double one_d[2] = {1, 0}, zero_d[2] = {0, 0};
    const float one_f[2] = {1, 0}, zero_f[2] = {0, 0};
    const bool f = real_bytes(vt) == 4;
    auto fn = cvec ? bsm_mul_multi_cvec : bsm_mul_multi;
    return fn(H, op, nrhs, X, ldx, Y, ldy, f ? (const void *)one_f : (const void *)one_d, f ? (const void *)zero_f : (const void *)zero_d, 1,
              BSM_MEM_DEVICE, (void *)st);
}

inline bool overlap(const void *a, size_t abytes, const void *b, size_t bbytes) {
    const uintptr_t p = (uintptr_t)a, q = (uintptr_t)b;
    return p < q + bbytes && q < p + abytes;
}

// The one allocation cut into 64-byte aligned pieces.  A method's layout is a function that takes its pieces in order; it
// runs without a base for the size (every piece null) and on the allocation for the pointers.
struct Carve {
    char *base = nullptr;
    int64_t off = 0;
    char *take(int64_t bytes) {
        const int64_t o = off;
        off += (bytes + 63) / 64 * 64;
        return base ? base + o : nullptr;
    }
};

// The argument checks every create begins with.  method_error: null, or what is wrong with the method's own argument
// (reported in its place in the order of the checks, behind vdtype).
inline int lockstep_check_create(const void *A, int opA, const void *M, int opM, int vdtype, int32_t nrhs_max,
                                 const char *method_error = nullptr) {
    if (!A) return fail(BSM_ERR_INVALID, "null handle");
    if (opA < 0 || opA > 2 || (M && (opM < 0 || opM > 2))) return fail(BSM_ERR_INVALID, "bad op");
    if (!is_vec_type(vdtype)) return fail(BSM_ERR_INVALID, "vdtype must be a vector type (BSM_F32 .. BSM_C128)");
    if (method_error) return fail(BSM_ERR_INVALID, method_error);
    if (nrhs_max < 1 || nrhs_max > BSM_CG_MAX_RHS) return fail(BSM_ERR_INVALID, "nrhs_max outside 1 .. BSM_CG_MAX_RHS");
    return BSM_OK;
}
// The other refusals of create that do not depend on the method (`what`: "bsm_cg", "bsm_bicgstab", "bsm_gmres_multi", "bsm_gmres"), and on success the fields
// of S that follow from the arguments.  square: the method needs op(A) square (else B has rows(op(A)) rows and X
// cols(op(A))).  out has been checked and cleared by the caller.
inline int lockstep_init(LockstepSolver *S, const char *what, bsm_matrix_s *A, int opA, bsm_matrix_s *M, int opM, int vdtype,
                         int32_t nrhs_max, bool square = true) {
    if (square && A->an.nrows != A->an.ncols) return fail(BSM_ERR_INVALID, "op(A) is not square");
    if (M && (M->an.nrows != A->an.nrows || M->an.ncols != A->an.ncols)) return fail(BSM_ERR_INVALID, "M has another order than A");
    const int pa = pairing(A, vdtype), pm = M ? pairing(M, vdtype) : 0;
    if (pa < 0 || pm < 0)
        return fail(BSM_ERR_INVALID, "a handle's vector type must be vdtype, or real and unmixed of the same precision under a complex vdtype");
    if (A->dist || (M && M->dist)) return fail(BSM_ERR_UNSUPPORTED, std::string("multi-device handles are not supported by ") + what);
    if (!A->on_device || (M && !M->on_device)) return fail(BSM_ERR_DEVICE, "handle has no device image (created with BSM_DEVICE_NONE)");
    // a handle that owns a row range only (one rank's share of a row partition) scales the owned rows of y alone: the other
    // rows of a product on the workspace would keep what the previous iteration left there
    for (const bsm_matrix_s *H : {A, M})
        if (H && (H->img.own_lo > 0 || H->img.own_hi < H->img.nrows))
            return fail(BSM_ERR_UNSUPPORTED, std::string("handles that own a row range only (bsm_options.own_lo / own_hi) are not supported by ") + what);
    if (M && M->img.device != A->img.device) return fail(BSM_ERR_INVALID, "A and M live on different devices");
    S->A = A, S->M = M, S->opA = opA, S->opM = opM, S->vt = vdtype, S->kmax = nrhs_max, S->device = A->img.device;
    S->a_cvec = pa == 1, S->m_cvec = pm == 1;
    S->n = opA == BSM_OP_N ? A->an.ncols : A->an.nrows;
    S->rows_b = opA == BSM_OP_N ? A->an.nrows : A->an.ncols;
    const int64_t es = elem_bytes(vdtype);
    S->ld = (std::max<int64_t>(S->n, 1) * es + 15) / 16 * 16 / es;
    S->G = krylov_grid(S->n, (int)es);
    S->ld_b = (std::max<int64_t>(S->rows_b, 1) * es + 15) / 16 * 16 / es;
    S->G_b = krylov_grid(S->rows_b, (int)es);
    return BSM_OK;
}

// The allocation of `bytes` (zeroed: the padding of the vectors is zero from here on, bsm_cg.h), the pinned slots and the
// events.  On failure everything is released; the caller deletes S.
inline int lockstep_alloc(LockstepSolver *S, int64_t bytes, const char *what) {
    S->ws_bytes = bytes;
    DeviceGuard guard;
    hipError_t e = guard.enter(S->device);
    if (e == hipSuccess) e = hipMalloc(&S->ws, (size_t)bytes);
    if (e == hipSuccess) e = hipMemset(S->ws, 0, (size_t)bytes);
    if (e == hipSuccess) e = hipHostMalloc((void **)&S->slots, sizeof(CgRecord) * kLockstepRing, hipHostMallocDefault);
    for (int i = 0; i < kLockstepRing && e == hipSuccess; i++) e = hipEventCreateWithFlags(&S->ev[i], hipEventDisableTiming);
    if (e == hipSuccess) return BSM_OK;
    S->release();
    return e == hipErrorOutOfMemory ? fail(BSM_ERR_ALLOC, std::string("out of device memory for the ") + what + " workspace")
                                    : hip_fail(e, (std::string(what) + " workspace").c_str());
}

// The whole of a create: out, the checks (method_error as in lockstep_check_create), the object, the refusals of
// lockstep_init, the allocation sized by layout(S, carve) (`ws_name`: "CG", .. for its failure) and the pointers from the
// same layout.  layout also sets the method's own fields of S.  square: as in lockstep_init.  refuse (may be null): a
// refusal of the method's own that needs the checked arguments -- called behind the argument checks, a status other than
// BSM_OK is returned as it is.
template <typename Solver, typename Layout>
int lockstep_create(const char *what, const char *ws_name, bsm_matrix_s *A, int opA, bsm_matrix_s *M, int opM, int vdtype, int32_t nrhs_max,
                    const char *method_error, Solver **out, Layout &&layout, bool square = true, int (*refuse)(bsm_matrix_s *, int) = nullptr) {
    if (!out) return fail(BSM_ERR_INVALID, "out is null");
    *out = nullptr;
    RC_TRY(lockstep_check_create(A, opA, M, opM, vdtype, nrhs_max, method_error));
    if (refuse) RC_TRY(refuse(A, opA));
    Solver *S = new (std::nothrow) Solver;
    if (!S) return fail(BSM_ERR_ALLOC, "out of host memory");
    int rc = lockstep_init(S, what, A, opA, M, opM, vdtype, nrhs_max, square);
    if (rc == BSM_OK) {
        Carve size;
        layout(*S, size);
        rc = lockstep_alloc(S, size.off, ws_name);
    }
    if (rc != BSM_OK) {
        delete S;
        return rc;
    }
    Carve cv{(char *)S->ws};
    layout(*S, cv);
    *out = S;
    return BSM_OK;
}

template <typename Solver> int lockstep_destroy(Solver *S) {
    if (!S) return BSM_OK;
    {
        DeviceGuard guard;
        (void)guard.enter(S->device);
        S->release();
    }
    delete S;
    return BSM_OK;
}

// The start of x every method shares: with use_x0 the caller's X into the workspace X and q = op(A) X (of B's length);
// else X = 0 (q is left alone: the method's start kernel gets no q).  d: the dimensions of X.
inline int lockstep_start_x(LockstepSolver *S, const CgDims &d, bool use_x0, void *X, int64_t ldx, void *wsX, void *q, hipStream_t st) {
    if (!use_x0) {
        HIP_TRY(hipMemsetAsync(wsX, 0, (size_t)S->ld * elem_bytes(S->vt) * d.nrhs, st));
        return BSM_OK;
    }
    HIP_TRY(launch_cg_copy(d, true, X, ldx, wsX, st));
    return apply(S->A, S->opA, S->a_cvec, d.nrhs, S->ld, S->ld_b, S->vt, wsX, q, st);
}

// The records of one solve: post() copies the record at the device address `rec` to the next pinned slot behind what has
// been enqueued, next() waits for the oldest unread one.  At most kLockstepRing - 1 may be unread.
struct RecordRing {
    LockstepSolver *S;
    const CgRecord *rec;
    hipStream_t st;
    int64_t posted = 0, read = 0;
    hipError_t post() {
        hipError_t q = hipMemcpyAsync(S->slots + posted % kLockstepRing, rec, sizeof(CgRecord), hipMemcpyDeviceToHost, st);
        if (q == hipSuccess) q = hipEventRecord(S->ev[posted % kLockstepRing], st);
        posted++;
        return q;
    }
    hipError_t next(const CgRecord *&r) {
        r = S->slots + read % kLockstepRing;
        return hipEventSynchronize(S->ev[read++ % kLockstepRing]);
    }
};
// what the host takes from a record as it arrives: the residual norms as row `row` of history (row < 0: none) -> the
// columns that still run
inline int lockstep_take(const CgRecord &r, int nrhs, int64_t row, const bsm_cg_params &p, double *history) {
    int running = 0;
    for (int c = 0; c < nrhs; c++) {
        running += r.status[c] == kCgRun;
        if (history && row >= 0 && row < p.history_capacity) history[row * nrhs + c] = r.rn[c];
    }
    return running;
}
// status, iterations and columns_converged of info and cols (may be null) from the last record of a solve
inline void lockstep_report(const CgRecord &r, int nrhs, bsm_cg_info &info, bsm_cg_column *cols) {
    for (int c = 0; c < nrhs; c++) {
        const int status = r.status[c] == kCgRun ? 1 : r.status[c];
        const int64_t its = r.done[c];
        info.status = std::max(info.status, status);
        info.iterations = std::max(info.iterations, its);
        info.columns_converged += status == 0;
        if (cols) {
            cols[c].status = status;
            cols[c].reserved = 0;
            cols[c].iterations = its;
            cols[c].residual = r.rn[c];
            cols[c].bnorm = r.bnorm[c];
        }
    }
}
// the end of a device solve: the copy-out of X (launch_cg_copy: n rows of nrhs columns and nothing else), then the report
inline int lockstep_finish(const CgDims &d, void *X, int64_t ldx, void *wsX, const CgRecord &last, bsm_cg_info &info, bsm_cg_column *cols,
                           hipStream_t st) {
    HIP_TRY(launch_cg_copy(d, false, X, ldx, wsX, st));
    HIP_TRY(hipStreamSynchronize(st));
    lockstep_report(last, d.nrhs, info, cols);
    return BSM_OK;
}

// The loop of a device solve after its start has been enqueued: record 0 (the start) is posted, iterate(j) enqueues
// iteration j (it leaves its record in state->rec), the host reads record j one iteration behind the enqueue, fills history
// and stops when no column runs or maxiter is reached; then lockstep_finish.  info.a_products / m_products are the caller's.
template <typename Iterate>
int lockstep_run(LockstepSolver *S, const CgDims &d, void *X, int64_t ldx, void *wsX, const bsm_cg_params &p, bsm_cg_info &info,
                 bsm_cg_column *cols, double *history, hipStream_t st, Iterate &&iterate) {
    const int64_t maxiter = std::min<int64_t>(p.maxiter, INT32_MAX);
    RecordRing ring{S, S->rec ? S->rec : &S->state->rec, st};
    HIP_TRY(ring.post());
    const CgRecord *last = nullptr;
    for (int64_t enq = 0;;) {
        if (enq < maxiter) {
            RC_TRY(iterate(enq));
            enq++;
            HIP_TRY(ring.post());
        }
        HIP_TRY(ring.next(last));
        const int64_t rd = ring.read - 1;
        if (lockstep_take(*last, d.nrhs, rd - 1, p, history) == 0 || rd == maxiter) break;
    }
    // (an iteration enqueued beyond the record read last found every column frozen: it wrote nothing)
    return lockstep_finish(d, X, ldx, wsX, *last, info, cols, st);
}

// The whole of a solve entry point but the method: the refusals, info cleared and its workspace fields set, n == 0, the
// device guard, and for BSM_MEM_HOST the staging through the dense buffers the solver keeps.  solve_device(B, ldb, X, ldx)
// is the solve on device matrices.  `what`: the entry's name for the capture refusal.
template <typename SolveDevice>
int lockstep_solve(LockstepSolver *S, const char *what, int32_t nrhs, const void *B, int64_t ldb, void *X, int64_t ldx, const bsm_cg_params *p,
                   bsm_cg_info *info, bsm_cg_column *cols, int memspace, hipStream_t st, SolveDevice &&solve_device) {
    if (!S || !p || !info) return fail(BSM_ERR_INVALID, "null argument");
    if (p->struct_size != (int32_t)sizeof(bsm_cg_params)) return fail(BSM_ERR_INVALID, "bsm_cg_params.struct_size mismatch");
    if (memspace != BSM_MEM_HOST && memspace != BSM_MEM_DEVICE) return fail(BSM_ERR_INVALID, "bad memspace");
    if (!(p->rtol >= 0) || !(p->atol >= 0) || p->maxiter < 0 || p->history_capacity < 0)
        return fail(BSM_ERR_INVALID, "rtol, atol, maxiter and history_capacity must be >= 0");
    if (nrhs < 1 || nrhs > S->kmax) return fail(BSM_ERR_INVALID, "nrhs outside 1 .. nrhs_max");
    // B has the rows of op(A), X its columns: one number for the solvers of square systems
    const int64_t n = S->n, mb = S->rows_b;
    const bool empty = n == 0 || mb == 0;
    if (ldb < std::max<int64_t>(mb, 1) || ldx < std::max<int64_t>(n, 1)) return fail(BSM_ERR_INVALID, "ldb / ldx < max(n, 1)");
    const size_t es = (size_t)elem_bytes(S->vt);
    const size_t bbytes = ((size_t)(nrhs - 1) * (size_t)ldb + (size_t)mb) * es, xbytes = ((size_t)(nrhs - 1) * (size_t)ldx + (size_t)n) * es;
    if (!empty && (!B || !X)) return fail(BSM_ERR_INVALID, "null matrix");
    if (!empty && overlap(B, bbytes, X, xbytes)) return fail(BSM_ERR_INVALID, "X must not overlap B");
    if (capturing(st)) return fail(BSM_ERR_INVALID, std::string(what) + " must not be graph-captured");
    std::memset(info, 0, sizeof(*info));
    info->workspace_bytes = S->ws_bytes;
    info->workspace = (uint64_t)(uintptr_t)S->ws;
    if (empty) {  // nothing to solve: status 0, no iteration, B and X (which may be null) untouched
        info->columns_converged = nrhs;
        if (cols) std::memset(cols, 0, sizeof(*cols) * (size_t)nrhs);
        return BSM_OK;
    }
    DeviceGuard guard;
    hipError_t e = guard.enter(S->device);
    if (e != hipSuccess) return hip_fail(e, "hipSetDevice");
    if (memspace == BSM_MEM_DEVICE) return solve_device(B, ldb, X, ldx);
    // host matrices: staged column by column through dense buffers the solver keeps
    const size_t col = (size_t)n * es, bcol = (size_t)mb * es;
    if (!S->hb || !S->hx) {
        if (!S->hb) e = hipMalloc(&S->hb, bcol * (size_t)S->kmax + 16);
        if (e == hipSuccess && !S->hx) e = hipMalloc(&S->hx, col * (size_t)S->kmax + 16);
        if (e != hipSuccess) {  // (a buffer that was obtained is kept; the next host solve asks for the other again)
            if (e != hipErrorOutOfMemory) return hip_fail(e, "staging buffers");
            (void)hipGetLastError();
            return fail(BSM_ERR_ALLOC, "out of device memory for the staging buffers");
        }
    }
    for (int c = 0; c < nrhs && e == hipSuccess; c++) {
        e = hipMemcpyAsync((char *)S->hb + c * bcol, (const char *)B + (size_t)c * (size_t)ldb * es, bcol, hipMemcpyHostToDevice, st);
        if (e == hipSuccess && p->use_x0)
            e = hipMemcpyAsync((char *)S->hx + c * col, (const char *)X + (size_t)c * (size_t)ldx * es, col, hipMemcpyHostToDevice, st);
    }
    if (e != hipSuccess) return hip_fail(e, "host-staged solve");
    const int rc = solve_device(S->hb, mb, S->hx, n);
    if (rc != BSM_OK) return rc;
    for (int c = 0; c < nrhs && e == hipSuccess; c++)
        e = hipMemcpyAsync((char *)X + (size_t)c * (size_t)ldx * es, (char *)S->hx + c * col, col, hipMemcpyDeviceToHost, st);
    if (e == hipSuccess) e = hipStreamSynchronize(st);
    if (e != hipSuccess) return hip_fail(e, "host-staged solve");
    return BSM_OK;
}

}  // namespace bsm
