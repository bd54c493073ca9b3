// bsm_gmres_multi.cpp -- the bsm_gmres_multi_* solver object (include/bsm_rocm.h): the host side of right-preconditioned
// restarted GMRES on up to BSM_CG_MAX_RHS right-hand sides in lockstep.  The products go through the public bsm_mul_multi /
// bsm_mul_multi_cvec, the vector work through the kernels of bsm_gmres_multi.hip.  Every decision of the method is taken on
// the device; the host only enqueues, and reads one record per gm_begin / gm_hess one step late.  Refusals, allocation
// and the staging of host matrices are bsm_lockstep.h, shared with bsm_cg.cpp and bsm_bicgstab.cpp; the loop over cycles is
// this unit's (lockstep_run is one flat sequence of iterations).
#include <hip/hip_runtime_api.h>

#include <algorithm>
#include <cstdint>
#include <new>

#define BSM_KRYLOV_LAUNCH
#include "bsm_internal.h"
#include "bsm_gmres_multi.h"
#include "bsm_lockstep.h"

using namespace bsm;

struct bsm_gmres_multi_s : LockstepSolver {
    int m = 0;
    // in the one allocation: V_0 .. V_m, W, X (and Z with M) as ld x kmax, the small arrays and partials per column, the state
    char *V = nullptr, *W = nullptr, *X = nullptr, *Z = nullptr;
    GmSmall sm = {};
    GmState *gst = nullptr;
    char *basis(int64_t i) const { return V + i * ld * kmax * elem_bytes(vt); }
};

extern "C" int bsm_gmres_multi_create(bsm_matrix_t A, int opA, bsm_matrix_t M, int opM, int vdtype, int32_t nrhs_max, int32_t restart,
                                      struct bsm_gmres_multi_s **out) {
    if (!out) return fail(BSM_ERR_INVALID, "out is null");
    *out = nullptr;
    int rc = lockstep_check_create(A, opA, M, opM, vdtype, nrhs_max,
                                   restart < 1 || restart > BSM_GMRES_MAX_RESTART ? "restart outside 1 .. BSM_GMRES_MAX_RESTART" : nullptr);
    if (rc != BSM_OK) return rc;
    bsm_gmres_multi_s *S = new (std::nothrow) bsm_gmres_multi_s;
    if (!S) return fail(BSM_ERR_ALLOC, "out of host memory");
    if ((rc = lockstep_init(S, "bsm_gmres_multi", A, opA, M, opM, vdtype, nrhs_max)) != BSM_OK) {
        delete S;
        return rc;
    }
    S->m = restart;
    const int64_t es = elem_bytes(vdtype), rs = real_bytes(vdtype), K = nrhs_max, m = restart, G = S->G;
    Carve cv;
    const int64_t vec = S->ld * es * K;
    const int64_t oV = cv.take(vec * (m + 1)), oW = cv.take(vec), oX = cv.take(vec), oZ = M ? cv.take(vec) : 0;
    const int64_t oH = cv.take(K * m * (m + 1) * es), ocs = cv.take(K * m * rs), osn = cv.take(K * m * es), og = cv.take(K * (m + 1) * es);
    const int64_t oy = cv.take(K * m * es), ohs = cv.take(K * m * es), oinv = cv.take(K * rs), opart = cv.take(K * m * G * es);
    const int64_t onrm = cv.take(K * G * rs), ost = cv.take((int64_t)sizeof(GmState));
    if ((rc = lockstep_alloc(S, cv.off, "GMRES")) != BSM_OK) {
        delete S;
        return rc;
    }
    char *b = (char *)S->ws;
    S->V = b + oV, S->W = b + oW, S->X = b + oX, S->Z = M ? b + oZ : nullptr;
    S->sm = GmSmall{b + oH, b + ocs, b + osn, b + og, b + oy, b + ohs, b + oinv, b + opart, b + onrm};
    S->gst = (GmState *)(b + ost);
    *out = S;
    return BSM_OK;
}

extern "C" int bsm_gmres_multi_destroy(struct bsm_gmres_multi_s *S) {
    if (!S) return BSM_OK;
    lockstep_destroy(S);
    delete S;
    return BSM_OK;
}

namespace {

// the solve on device matrices B, X (arguments checked)
int solve_device(bsm_gmres_multi_s *S, int nrhs, const void *B, int64_t ldb, void *X, int64_t ldx, const bsm_cg_params &p, bsm_cg_info &info,
                 bsm_cg_column *cols, double *history, hipStream_t st) {
    const int vt = S->vt, es = elem_bytes(vt), m = S->m;
    const GmDims g{CgDims{vt, S->n, S->ld, S->G, nrhs, true}, m, S->kmax};
    const size_t vec_bytes = (size_t)S->ld * es * nrhs;
    const int64_t maxiter = std::min<int64_t>(p.maxiter, INT32_MAX);
    const GmSmall &sm = S->sm;
    GmState *const gs = S->gst;
    hipError_t e = hipSuccess;
    int rc = BSM_OK;
#define HIP_TRY(call)                                   \
    do {                                                \
        e = (call);                                     \
        if (e != hipSuccess) return hip_fail(e, #call); \
    } while (0)
#define RC_TRY(call)                 \
    do {                             \
        rc = (call);                 \
        if (rc != BSM_OK) return rc; \
    } while (0)
    // ---- the records: posted behind gm_begin (row -1) and gm_hess (row = the lockstep iteration), read in order, at most
    // one of them unread while the host enqueues
    int64_t posted = 0, read = 0, row_of[kLockstepRing] = {};
    CgRecord last = {};
    int running = nrhs;          // of the record read last
    bool last_was_begin = true;  // the record read last came from a gm_begin
    bool stopped = false;        // a record showed no column running: what was enqueued behind it wrote nothing and is not read
    int64_t restarts_used = 0;   // restarts that found a column running: their op(A) X product is part of the answer
    auto post = [&](int64_t row) -> hipError_t {
        hipError_t q = hipMemcpyAsync(S->slots + posted % kLockstepRing, &gs->rec, sizeof(CgRecord), hipMemcpyDeviceToHost, st);
        if (q == hipSuccess) q = hipEventRecord(S->ev[posted % kLockstepRing], st);
        row_of[posted % kLockstepRing] = row;
        posted++;
        return q;
    };
    auto read_until = [&](int64_t unread) -> hipError_t {  // reads records until at most `unread` of the posted ones are left
        while (posted - read > unread) {
            const hipError_t q = hipEventSynchronize(S->ev[read % kLockstepRing]);
            if (q != hipSuccess) return q;
            if (stopped) {
                read++;
                continue;
            }
            const int64_t row = row_of[read % kLockstepRing];
            if (row < 0 && read > 0 && running > 0) restarts_used++;
            last = S->slots[read % kLockstepRing];
            last_was_begin = row < 0;
            running = 0;
            for (int c = 0; c < nrhs; c++) {
                running += last.status[c] == kCgRun;
                if (history && row >= 0 && row < p.history_capacity) history[row * nrhs + c] = last.rn[c];
            }
            stopped = running == 0;
            read++;
        }
        return hipSuccess;
    };
    // ---- the start: x, r -> V_0, the norms, the first decision
    int par = 0;  // the slot of the state the launches read
    if (p.use_x0) {
        HIP_TRY(launch_cg_copy(g.d, true, X, ldx, S->X, st));
        RC_TRY(apply(S->A, S->opA, S->a_cvec, nrhs, S->ld, vt, S->X, S->W, st));
    } else {
        HIP_TRY(hipMemsetAsync(S->X, 0, vec_bytes, st));
    }
    HIP_TRY(launch_gm_start(g, true, 0, B, ldb, p.use_x0 ? S->W : nullptr, S->basis(0), sm, gs, st));
    HIP_TRY(launch_gm_begin(g, true, 0, p.rtol, p.atol, S->basis(0), sm, gs, st));
    HIP_TRY(post(-1));
    // ---- the cycles
    int64_t it = 0;  // lockstep iterations enqueued
    for (;;) {
        const int jmax = (int)std::min<int64_t>(m, maxiter - it);
        int j = 0;
        for (; j < jmax; j++) {
            const char *vj = S->basis(j);
            if (S->M) {
                RC_TRY(apply(S->M, S->opM, S->m_cvec, nrhs, S->ld, vt, vj, S->Z, st));
                RC_TRY(apply(S->A, S->opA, S->a_cvec, nrhs, S->ld, vt, S->Z, S->W, st));
            } else {
                RC_TRY(apply(S->A, S->opA, S->a_cvec, nrhs, S->ld, vt, vj, S->W, st));
            }
            for (int pass = 0; pass < 2; pass++) {
                HIP_TRY(launch_gm_dot(g, par, j + 1, S->V, S->W, sm, gs, st));
                HIP_TRY(launch_gm_update(g, par, j + 1, S->V, S->W, sm, gs, st));
            }
            HIP_TRY(launch_gm_hess(g, par, j, sm, gs, st));
            par ^= 1;
            HIP_TRY(launch_gm_scale(g, par, S->W, S->basis(j + 1), sm, gs, st));
            HIP_TRY(post(it));
            it++;
            HIP_TRY(read_until(1));
            if (running == 0) {  // (the iteration just enqueued found every column frozen: it wrote nothing)
                j++;
                break;
            }
        }
        // the end of the cycle, enqueued without waiting: x += opM(M) V y on the columns that owe it, harmless on the others.  A
        // cycle none of whose iterations was used -- the record of its gm_begin showed no column running -- is skipped.
        if (j > 0 && !(stopped && last_was_begin)) {
            HIP_TRY(launch_gm_trsolve(g, par, sm, gs, st));
            HIP_TRY(launch_gm_combine(g, par, S->V, S->W, sm, gs, st));
            if (S->M) RC_TRY(apply(S->M, S->opM, S->m_cvec, nrhs, S->ld, vt, S->W, S->Z, st));
            HIP_TRY(launch_gm_axpy(g, par, S->M ? S->Z : S->W, S->X, gs, st));
        }
        if (running == 0 || it >= maxiter) break;
        // the restart, enqueued without waiting: the true residual b - op(A) x into V_0, its norm, the decision
        RC_TRY(apply(S->A, S->opA, S->a_cvec, nrhs, S->ld, vt, S->X, S->W, st));
        HIP_TRY(launch_gm_start(g, false, par, B, ldb, S->W, S->basis(0), sm, gs, st));
        HIP_TRY(launch_gm_begin(g, false, par, p.rtol, p.atol, S->basis(0), sm, gs, st));
        par ^= 1;
        HIP_TRY(post(-1));
        HIP_TRY(read_until(1));
        if (running == 0) break;  // (the restart found every column frozen: it wrote nothing)
    }
    HIP_TRY(read_until(0));
    HIP_TRY(launch_cg_copy(g.d, false, X, ldx, S->X, st));
    HIP_TRY(hipStreamSynchronize(st));
    for (int c = 0; c < nrhs; c++) {
        const int status = last.status[c] == kCgRun ? 1 : last.status[c];
        const int64_t its = last.done[c];
        info.status = std::max(info.status, status);
        info.iterations = std::max(info.iterations, its);
        info.columns_converged += status == 0;
        if (cols) {
            cols[c].status = status;
            cols[c].reserved = 0;
            cols[c].iterations = its;
            cols[c].residual = last.rn[c];
            cols[c].bnorm = last.bnorm[c];
        }
    }
    const int64_t cycles = (info.iterations + m - 1) / m;
    info.a_products = info.iterations + restarts_used + (p.use_x0 ? 1 : 0);
    info.m_products = S->M ? info.iterations + cycles : 0;
#undef HIP_TRY
#undef RC_TRY
    return BSM_OK;
}

}  // namespace

extern "C" int bsm_gmres_multi_solve(struct bsm_gmres_multi_s *S, int32_t nrhs, const void *B, int64_t ldb, void *X, int64_t ldx,
                                     const bsm_cg_params *p, bsm_cg_info *info, bsm_cg_column *cols, double *history, int memspace,
                                     void *stream) {
    const hipStream_t st = (hipStream_t)stream;
    return lockstep_solve(S, "bsm_gmres_multi_solve", nrhs, B, ldb, X, ldx, p, info, cols, memspace, st,
                          [&](const void *Bd, int64_t ldbd, void *Xd, int64_t ldxd) {
                              return solve_device(S, nrhs, Bd, ldbd, Xd, ldxd, *p, *info, cols, history, st);
                          });
}
