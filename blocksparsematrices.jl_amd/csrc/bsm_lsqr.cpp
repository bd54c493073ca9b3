// bsm_lsqr.cpp -- the bsm_lsqr_* solver object and the test hook bsm_debug_lsqr_step (include/bsm_rocm.h): the host side of
// LSQR on up to BSM_CG_MAX_RHS right-hand sides in lockstep, for rectangular, rank-deficient and damped least-squares
// problems.  It is the one lockstep solver whose vectors have two lengths -- B, U, Q have the rows of op(A), X, V, W, P its
// columns -- and the one that issues the adjoint product: per iteration Q = op(A) V and P = op(A)^H U, both through the
// public bsm_mul_multi / bsm_mul_multi_cvec, the vector work through the kernels of bsm_lsqr.hip.  Every decision of the
// method is taken on the device; the host only enqueues and reads one record per iteration from a pinned slot, one
// iteration late.  What does not depend on the method is bsm_lockstep.h, shared with the other four drivers.
#include <hip/hip_runtime_api.h>

#include <cstdint>
#include <new>

#define BSM_KRYLOV_LAUNCH
#include "bsm_internal.h"
#include "bsm_lockstep.h"
#include "bsm_lsqr.h"

using namespace bsm;

struct bsm_lsqr_s : LockstepSolver {
    // in the one allocation: X, V, W, P as ld x kmax, U, Q as ld_b x kmax, the partials of both grids, the state
    char *X = nullptr, *V = nullptr, *W = nullptr, *P = nullptr, *U = nullptr, *Q = nullptr;
    char *pbb = nullptr, *pu = nullptr, *pv = nullptr;
    LsState *ls = nullptr;
    int opH = 0;  // op(A)^H as an op of the handle
};

namespace {

// op(A)^H of op(A) = A^T is conj(A), which no product offers; on a real handle it is A
int refuse_conj(bsm_matrix_s *A, int opA) {
    const bool cplx = A->an.dtype == BSM_C64 || A->an.dtype == BSM_C128 || A->an.dtype == BSM_C128_C64;
    if (opA == BSM_OP_T && cplx)
        return fail(BSM_ERR_UNSUPPORTED, "bsm_lsqr: opA = BSM_OP_T on a complex handle needs products with conj(A), which are not "
                                         "available; use BSM_OP_N or BSM_OP_C");
    return BSM_OK;
}

}  // namespace

extern "C" int bsm_lsqr_create(bsm_matrix_t A, int opA, int vdtype, int32_t nrhs_max, struct bsm_lsqr_s **out) {
    return lockstep_create(
        "bsm_lsqr", "LSQR", A, opA, nullptr, 0, vdtype, nrhs_max, nullptr, out,
        [&](bsm_lsqr_s &S, Carve &cv) {
            const int64_t es = elem_bytes(vdtype), rs = real_bytes(vdtype), K = nrhs_max;
            const int64_t nvec = S.ld * es * K, mvec = S.ld_b * es * K;
            S.X = cv.take(nvec), S.V = cv.take(nvec), S.W = cv.take(nvec), S.P = cv.take(nvec);
            S.U = cv.take(mvec), S.Q = cv.take(mvec);
            S.pbb = cv.take(K * S.G_b * rs), S.pu = cv.take(K * S.G_b * rs), S.pv = cv.take(K * S.G * rs);
            S.ls = (LsState *)cv.take((int64_t)sizeof(LsState));
            S.rec = S.ls ? &S.ls->rec : nullptr;
            S.opH = opA == BSM_OP_N ? BSM_OP_C : BSM_OP_N;
        },
        false, refuse_conj);
}

extern "C" int bsm_lsqr_destroy(struct bsm_lsqr_s *S) { return lockstep_destroy(S); }

namespace {

// the solve on device matrices B, X (arguments checked)
int solve_device(bsm_lsqr_s *S, int nrhs, const void *B, int64_t ldb, void *X, int64_t ldx, const bsm_lsqr_params &lp, const bsm_cg_params &p,
                 bsm_cg_info &info, bsm_cg_column *cols, double *history, double *arnorm, double *anorm, hipStream_t st) {
    const int vt = S->vt, Gm = S->G_b;
    const CgDims dn{vt, S->n, S->ld, S->G, nrhs, true}, dm{vt, S->rows_b, S->ld_b, S->G_b, nrhs, true};
    auto forward = [&](const void *v, void *q) { return apply(S->A, S->opA, S->a_cvec, nrhs, S->ld, S->ld_b, vt, v, q, st); };
    auto adjoint = [&](const void *u, void *pp) { return apply(S->A, S->opH, S->a_cvec, nrhs, S->ld_b, S->ld, vt, u, pp, st); };
    // ---- the start: x, u = b - op(A) x0, v = op(A)^H u / beta, the norms, the first decision
    RC_TRY(lockstep_start_x(S, dn, p.use_x0, X, ldx, S->X, S->Q, st));
    HIP_TRY(launch_ls_start(dm, B, ldb, p.use_x0 ? S->Q : nullptr, S->U, S->pbb, S->pu, st));
    RC_TRY(adjoint(S->U, S->P));
    HIP_TRY(launch_ls_begin(dn, Gm, S->pu, S->P, S->V, S->pv, st));
    HIP_TRY(launch_ls_decide(dn, true, 0, 0, Gm, p.rtol, p.atol, lp.ntol, S->pbb, S->pu, S->pv, S->ls, st));
    // ---- the iterations, their records read one behind the enqueue
    int64_t enqueued = 0;
    RC_TRY(lockstep_run(S, dn, X, ldx, S->X, p, info, cols, history, st, [&](int64_t j) -> int {
        const int par = (int)(j & 1);
        enqueued = j + 1;
        RC_TRY(forward(S->V, S->Q));
        HIP_TRY(launch_ls_u(dm, par, S->Q, S->U, S->pu, S->ls, st));
        RC_TRY(adjoint(S->U, S->P));
        HIP_TRY(launch_ls_v(dn, j == 0, par, Gm, S->pu, S->P, S->V, S->W, S->pv, S->ls, st));
        HIP_TRY(launch_ls_update(dn, par, Gm, lp.damp, lp.ntol, S->pu, S->pv, S->V, S->W, S->X, S->ls, st));
        HIP_TRY(launch_ls_decide(dn, false, par, j + 1, Gm, p.rtol, p.atol, lp.ntol, S->pbb, S->pu, S->pv, S->ls, st));
        return BSM_OK;
    }));
    info.a_products = 2 * info.iterations + 1 + (p.use_x0 ? 1 : 0);
    info.m_products = 0;
    if (arnorm || anorm) {
        // the estimates of every column, from the slot the last enqueued decision wrote (it carries frozen columns over)
        LsSlot last;
        HIP_TRY(hipMemcpyAsync(&last, &S->ls->slot[enqueued & 1], sizeof(last), hipMemcpyDeviceToHost, st));
        HIP_TRY(hipStreamSynchronize(st));
        for (int c = 0; c < nrhs; c++) {
            if (arnorm) arnorm[c] = last.arnorm[c];
            if (anorm) anorm[c] = last.anorm[c];
        }
    }
    return BSM_OK;
}

}  // namespace

extern "C" int bsm_lsqr_solve(struct bsm_lsqr_s *S, int32_t nrhs, const void *B, int64_t ldb, void *X, int64_t ldx, const bsm_lsqr_params *lp,
                              bsm_cg_info *info, bsm_cg_column *cols, double *history, double *arnorm, double *anorm, int memspace,
                              void *stream) {
    if (!S || !lp || !info) return fail(BSM_ERR_INVALID, "null argument");
    if (lp->struct_size != (int32_t)sizeof(bsm_lsqr_params)) return fail(BSM_ERR_INVALID, "bsm_lsqr_params.struct_size mismatch");
    if (!(lp->ntol >= 0) || !(lp->damp >= 0)) return fail(BSM_ERR_INVALID, "ntol and damp must be >= 0");
    const bsm_cg_params p{(int32_t)sizeof(bsm_cg_params), lp->use_x0, lp->rtol, lp->atol, lp->maxiter, lp->history_capacity};
    const hipStream_t st = (hipStream_t)stream;
    const int rc = lockstep_solve(S, "bsm_lsqr_solve", nrhs, B, ldb, X, ldx, &p, info, cols, memspace, st,
                                  [&](const void *Bd, int64_t ldbd, void *Xd, int64_t ldxd) {
                                      return solve_device(S, nrhs, Bd, ldbd, Xd, ldxd, *lp, p, *info, cols, history, arnorm, anorm, st);
                                  });
    if (rc == BSM_OK && (S->n == 0 || S->rows_b == 0)) {  // nothing was solved: the estimates are zero like the columns
        for (int c = 0; c < nrhs; c++) {
            if (arnorm) arnorm[c] = 0;
            if (anorm) anorm[c] = 0;
        }
    }
    return rc;
}

// test hook (unexported in the header, like bsm_debug_krylov_lsq_host): lsqr_step of bsm_lsqr.h in double, the arithmetic
// ls_update runs for one column.  in: alpha, beta, phibar, rhobar, res2, anorm;  out: the six of the next iteration, then cx,
// cw, rnorm, arnorm;  status: -1 (the column runs on), 0 or 2.  Needs no device.
extern "C" int bsm_debug_lsqr_step(const double *in, double betan, double alphan, double damp, double tol, double ntol, double *out,
                                   int32_t *status) {
    if (!in || !out || !status) return fail(BSM_ERR_INVALID, "null argument");
    const LsqrScalars<double> cur{in[0], in[1], in[2], in[3], in[4], in[5]};
    LsqrStep<double> s;
    lsqr_step(cur, betan, alphan, damp, tol, ntol, s);
    const double o[10] = {s.next.alpha, s.next.beta, s.next.phibar, s.next.rhobar, s.next.res2, s.next.anorm, s.cx, s.cw, s.rnorm, s.arnorm};
    for (int i = 0; i < 10; i++) out[i] = o[i];
    *status = s.status;
    return BSM_OK;
}
