// bsm_gmres_multi.cpp -- the bsm_gmres_multi_* and bsm_gmres_* solver objects (include/bsm_rocm.h): the host side of
// right-preconditioned restarted GMRES on up to BSM_CG_MAX_RHS right-hand sides in lockstep, and its one-column front.  The
// products go through the public bsm_mul_multi / bsm_mul_multi_cvec, the vector work through the kernels of
// bsm_gmres_multi.hip.  Every decision of the method is taken on the device; the host only enqueues, and reads one record
// per gm_begin / gm_hess one step late.  Create but for the layout of the workspace, the refusals, the staging of host
// matrices, the record ring and the report are bsm_lockstep.h, shared with bsm_cg.cpp and bsm_bicgstab.cpp; the loop over
// cycles -- which record belongs to which history row, the restarts -- is this unit's (lockstep_run is one flat sequence of
// iterations).  bsm_gmres_* is the same solver created with nrhs_max = 1 behind its own parameter and info structs.
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

// the solver of bsm_gmres_*: the lockstep solver with one column
struct bsm_gmres_s : bsm_gmres_multi_s {};

namespace {

// create of both solver objects (`what`: "bsm_gmres_multi", "bsm_gmres")
template <typename Solver>
int gm_create(const char *what, bsm_matrix_t A, int opA, bsm_matrix_t M, int opM, int vdtype, int32_t nrhs_max, int32_t restart, Solver **out) {
    return lockstep_create(what, "GMRES", A, opA, M, opM, vdtype, nrhs_max,
                           restart < 1 || restart > BSM_GMRES_MAX_RESTART ? "restart outside 1 .. BSM_GMRES_MAX_RESTART" : nullptr, out,
                           [&](Solver &S, Carve &cv) {
                               S.m = restart;
                               const int64_t es = elem_bytes(vdtype), rs = real_bytes(vdtype), K = nrhs_max, m = restart, G = S.G, vec = S.ld * es * K;
                               S.V = cv.take(vec * (m + 1)), S.W = cv.take(vec), S.X = cv.take(vec), S.Z = M ? cv.take(vec) : nullptr;
                               // (Hm, cs, sn, g, y, hsum, inv, part, nrm: in this order)
                               S.sm = GmSmall{cv.take(K * m * (m + 1) * es), cv.take(K * m * rs), cv.take(K * m * es), cv.take(K * (m + 1) * es),
                                              cv.take(K * m * es),           cv.take(K * m * es), cv.take(K * rs),     cv.take(K * m * G * es),
                                              cv.take(K * G * rs)};
                               S.gst = (GmState *)cv.take((int64_t)sizeof(GmState));
                           });
}

// the solve on device matrices B, X (arguments checked)
int solve_device(bsm_gmres_multi_s *S, int nrhs, const void *B, int64_t ldb, void *X, int64_t ldx, const bsm_cg_params &p, bsm_cg_info &info,
                 bsm_cg_column *cols, double *history, hipStream_t st) {
    const int vt = S->vt, m = S->m;
    const GmDims g{CgDims{vt, S->n, S->ld, S->G, nrhs, true}, m, S->kmax};
    const int64_t maxiter = std::min<int64_t>(p.maxiter, INT32_MAX);
    const GmSmall &sm = S->sm;
    GmState *const gs = S->gst;
    // ---- the records: posted behind gm_begin (row -1) and gm_hess (row = the lockstep iteration), read in order, at most
    // one of them unread while the host enqueues
    RecordRing ring{S, &gs->rec, st};
    int64_t row_of[kLockstepRing] = {};
    CgRecord last = {};
    int running = nrhs;          // of the record read last
    bool last_was_begin = true;  // the record read last came from a gm_begin
    bool stopped = false;        // a record showed no column running: what was enqueued behind it wrote nothing and is not read
    int64_t restarts_used = 0;   // restarts that found a column running: their op(A) X product is part of the answer
    auto post = [&](int64_t row) -> hipError_t {
        row_of[ring.posted % kLockstepRing] = row;
        return ring.post();
    };
    auto read_until = [&](int64_t unread) -> hipError_t {  // reads records until at most `unread` of the posted ones are left
        while (ring.posted - ring.read > unread) {
            const int64_t row = row_of[ring.read % kLockstepRing];
            const bool restart = row < 0 && ring.read > 0;
            const CgRecord *r = nullptr;
            const hipError_t q = ring.next(r);
            if (q != hipSuccess) return q;
            if (stopped) continue;
            if (restart && running > 0) restarts_used++;
            last = *r;
            last_was_begin = row < 0;
            running = lockstep_take(last, nrhs, row, p, history);
            stopped = running == 0;
        }
        return hipSuccess;
    };
    // ---- the start: x, r -> V_0, the norms, the first decision
    int par = 0;  // the slot of the state the launches read
    RC_TRY(lockstep_start_x(S, g.d, p.use_x0, X, ldx, S->X, S->W, st));
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
                RC_TRY(apply(S->M, S->opM, S->m_cvec, nrhs, S->ld, S->ld, vt, vj, S->Z, st));
                RC_TRY(apply(S->A, S->opA, S->a_cvec, nrhs, S->ld, S->ld, vt, S->Z, S->W, st));
            } else {
                RC_TRY(apply(S->A, S->opA, S->a_cvec, nrhs, S->ld, S->ld, vt, vj, S->W, st));
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
            if (S->M) RC_TRY(apply(S->M, S->opM, S->m_cvec, nrhs, S->ld, S->ld, vt, S->W, S->Z, st));
            HIP_TRY(launch_gm_axpy(g, par, S->M ? S->Z : S->W, S->X, gs, st));
        }
        if (running == 0 || it >= maxiter) break;
        // the restart, enqueued without waiting: the true residual b - op(A) x into V_0, its norm, the decision
        RC_TRY(apply(S->A, S->opA, S->a_cvec, nrhs, S->ld, S->ld, vt, S->X, S->W, st));
        HIP_TRY(launch_gm_start(g, false, par, B, ldb, S->W, S->basis(0), sm, gs, st));
        HIP_TRY(launch_gm_begin(g, false, par, p.rtol, p.atol, S->basis(0), sm, gs, st));
        par ^= 1;
        HIP_TRY(post(-1));
        HIP_TRY(read_until(1));
        if (running == 0) break;  // (the restart found every column frozen: it wrote nothing)
    }
    HIP_TRY(read_until(0));
    RC_TRY(lockstep_finish(g.d, X, ldx, S->X, last, info, cols, st));
    const int64_t cycles = (info.iterations + m - 1) / m;
    info.a_products = info.iterations + restarts_used + (p.use_x0 ? 1 : 0);
    info.m_products = S->M ? info.iterations + cycles : 0;
    return BSM_OK;
}

// solve of both solver objects (`what`: the entry's name)
int gm_solve(bsm_gmres_multi_s *S, const char *what, int32_t nrhs, const void *B, int64_t ldb, void *X, int64_t ldx, const bsm_cg_params *p,
             bsm_cg_info *info, bsm_cg_column *cols, double *history, int memspace, hipStream_t st) {
    return lockstep_solve(S, what, nrhs, B, ldb, X, ldx, p, info, cols, memspace, st, [&](const void *Bd, int64_t ldbd, void *Xd, int64_t ldxd) {
        return solve_device(S, nrhs, Bd, ldbd, Xd, ldxd, *p, *info, cols, history, st);
    });
}

}  // namespace

extern "C" int bsm_gmres_multi_create(bsm_matrix_t A, int opA, bsm_matrix_t M, int opM, int vdtype, int32_t nrhs_max, int32_t restart,
                                      struct bsm_gmres_multi_s **out) {
    return gm_create("bsm_gmres_multi", A, opA, M, opM, vdtype, nrhs_max, restart, out);
}

extern "C" int bsm_gmres_multi_solve(struct bsm_gmres_multi_s *S, int32_t nrhs, const void *B, int64_t ldb, void *X, int64_t ldx,
                                     const bsm_cg_params *p, bsm_cg_info *info, bsm_cg_column *cols, double *history, int memspace,
                                     void *stream) {
    return gm_solve(S, "bsm_gmres_multi_solve", nrhs, B, ldb, X, ldx, p, info, cols, history, memspace, (hipStream_t)stream);
}

extern "C" int bsm_gmres_multi_destroy(struct bsm_gmres_multi_s *S) { return lockstep_destroy(S); }

// ---- bsm_gmres_*: one column.  Its own structs in, bsm_cg_params / bsm_cg_info / one bsm_cg_column through gm_solve, its
// own info out; history row i of one column is history[i].
extern "C" int bsm_gmres_create(bsm_matrix_t A, int opA, bsm_matrix_t M, int opM, int vdtype, int32_t restart, bsm_gmres_t *out) {
    return gm_create("bsm_gmres", A, opA, M, opM, vdtype, 1, restart, out);
}

extern "C" int bsm_gmres_solve(bsm_gmres_t S, const void *b, void *x, const bsm_gmres_params *p, bsm_gmres_info *info,
                               double *history, int memspace, void *stream) {
    if (!S || !p || !info) return fail(BSM_ERR_INVALID, "null argument");
    if (p->struct_size != (int32_t)sizeof(bsm_gmres_params)) return fail(BSM_ERR_INVALID, "bsm_gmres_params.struct_size mismatch");
    const size_t bytes = (size_t)S->n * elem_bytes(S->vt);
    if (S->n > 0 && (!b || !x)) return fail(BSM_ERR_INVALID, "null vector");
    if (S->n > 0 && overlap(b, bytes, x, bytes)) return fail(BSM_ERR_INVALID, "x must not alias b");
    const bsm_cg_params q{(int32_t)sizeof(bsm_cg_params), p->use_x0, p->rtol, p->atol, p->maxiter, p->history_capacity};
    const int64_t ld = std::max<int64_t>(S->n, 1);
    bsm_cg_info ci;
    bsm_cg_column col;
    const int rc = gm_solve(S, "bsm_gmres_solve", 1, b, ld, x, ld, &q, &ci, &col, history, memspace, (hipStream_t)stream);
    if (rc != BSM_OK) return rc;
    *info = bsm_gmres_info{ci.status,     (int32_t)((ci.iterations + S->m - 1) / S->m), ci.iterations,      col.residual, col.bnorm,
                           ci.a_products, ci.m_products,                                ci.workspace_bytes, ci.workspace};
    return BSM_OK;
}

extern "C" int bsm_gmres_destroy(bsm_gmres_t S) { return lockstep_destroy(S); }
