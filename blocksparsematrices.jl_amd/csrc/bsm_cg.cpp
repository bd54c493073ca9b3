// bsm_cg.cpp -- the bsm_cg_* solver object (include/bsm_rocm.h): the host side of preconditioned CG / COCG on up to
// BSM_CG_MAX_RHS right-hand sides in lockstep.  The products go through the public bsm_mul_multi / bsm_mul_multi_cvec, the
// vector work through the kernels of bsm_cg.hip.  Every decision of the method is taken on the device; the host only
// enqueues, and reads one record per iteration from a pinned slot, one iteration late (the look-ahead), to know when to
// stop enqueuing.  What does not depend on the method -- the refusals, the allocation, the staging of host matrices, that
// loop, create but for the layout of the workspace -- is bsm_lockstep.h, shared with bsm_bicgstab.cpp and bsm_gmres_multi.cpp.
#include <hip/hip_runtime_api.h>

#include <cstdint>
#include <new>

#define BSM_KRYLOV_LAUNCH
#include "bsm_internal.h"
#include "bsm_cg.h"
#include "bsm_lockstep.h"

using namespace bsm;

struct bsm_cg_s : LockstepSolver {
    bool conj = true;
    // in the one allocation: X, R, P, Q (and Z with M) as ld x kmax, the partials, the state
    char *X = nullptr, *R = nullptr, *P = nullptr, *Q = nullptr, *Z = nullptr;
    char *ppq = nullptr, *prz = nullptr, *pnn = nullptr, *pbb = nullptr;
};

extern "C" int bsm_cg_create(bsm_matrix_t A, int opA, bsm_matrix_t M, int opM, int vdtype, int32_t nrhs_max, int32_t method,
                             struct bsm_cg_s **out) {
    const bool method_ok = method == BSM_CG_METHOD_CG || method == BSM_CG_METHOD_COCG;
    return lockstep_create("bsm_cg", "CG", A, opA, M, opM, vdtype, nrhs_max,
                           method_ok ? nullptr : "method must be BSM_CG_METHOD_CG or BSM_CG_METHOD_COCG", out, [&](bsm_cg_s &S, Carve &cv) {
                               S.conj = method == BSM_CG_METHOD_CG;
                               const int64_t es = elem_bytes(vdtype), rs = real_bytes(vdtype), K = nrhs_max, vec = S.ld * es * K;
                               S.X = cv.take(vec), S.R = cv.take(vec), S.P = cv.take(vec), S.Q = cv.take(vec), S.Z = M ? cv.take(vec) : nullptr;
                               S.ppq = cv.take(K * S.G * es), S.prz = cv.take(K * S.G * es), S.pnn = cv.take(K * S.G * rs), S.pbb = cv.take(K * S.G * rs);
                               S.state = (CgState *)cv.take((int64_t)sizeof(CgState));
                           });
}

extern "C" int bsm_cg_destroy(struct bsm_cg_s *S) { return lockstep_destroy(S); }

namespace {

// the solve on device matrices B, X (arguments checked)
int solve_device(bsm_cg_s *S, int nrhs, const void *B, int64_t ldb, void *X, int64_t ldx, const bsm_cg_params &p, bsm_cg_info &info,
                 bsm_cg_column *cols, double *history, hipStream_t st) {
    const int vt = S->vt;
    const CgDims d{vt, S->n, S->ld, S->G, nrhs, S->conj};
    char *const Zv = S->M ? S->Z : S->R;          // z = r without M
    void *const prz_fused = S->M ? nullptr : S->prz;  // without M, cg_start / cg_update leave the shares of <r, r> themselves
    // z = M r and the shares of <r, z> (with M only)
    auto precondition = [&](int par) -> int {
        if (!S->M) return BSM_OK;
        const int r = apply(S->M, S->opM, S->m_cvec, nrhs, S->ld, S->ld, vt, S->R, S->Z, st);
        if (r != BSM_OK) return r;
        const hipError_t q = launch_cg_dot(d, par, S->R, S->Z, S->prz, S->state, st);
        return q == hipSuccess ? BSM_OK : hip_fail(q, "launch_cg_dot");
    };
    // ---- the start: x, r, the norms, p = z, the first decision
    RC_TRY(lockstep_start_x(S, d, p.use_x0, X, ldx, S->X, S->Q, st));
    HIP_TRY(launch_cg_start(d, B, ldb, p.use_x0 ? S->Q : nullptr, S->R, S->pbb, S->pnn, prz_fused, S->state, st));
    RC_TRY(precondition(-1));
    HIP_TRY(launch_cg_dir(d, true, 0, 0, p.rtol, p.atol, S->pbb, S->pnn, S->prz, Zv, S->P, S->state, st));
    // ---- the iterations, their records read one behind the enqueue
    RC_TRY(lockstep_run(S, d, X, ldx, S->X, p, info, cols, history, st, [&](int64_t j) -> int {
        const int par = (int)(j & 1);
        RC_TRY(apply(S->A, S->opA, S->a_cvec, nrhs, S->ld, S->ld, vt, S->P, S->Q, st));
        HIP_TRY(launch_cg_dot(d, par, S->P, S->Q, S->ppq, S->state, st));
        HIP_TRY(launch_cg_update(d, par, S->ppq, S->P, S->Q, S->X, S->R, S->pnn, prz_fused, S->state, st));
        RC_TRY(precondition(par));
        HIP_TRY(launch_cg_dir(d, false, par, j + 1, p.rtol, p.atol, S->pbb, S->pnn, S->prz, Zv, S->P, S->state, st));
        return BSM_OK;
    }));
    info.a_products = info.iterations + (p.use_x0 ? 1 : 0);
    info.m_products = S->M ? info.iterations + 1 : 0;
    return BSM_OK;
}

}  // namespace

extern "C" int bsm_cg_solve(struct bsm_cg_s *S, int32_t nrhs, const void *B, int64_t ldb, void *X, int64_t ldx, const bsm_cg_params *p,
                            bsm_cg_info *info, bsm_cg_column *cols, double *history, int memspace, void *stream) {
    const hipStream_t st = (hipStream_t)stream;
    return lockstep_solve(S, "bsm_cg_solve", nrhs, B, ldb, X, ldx, p, info, cols, memspace, st,
                          [&](const void *Bd, int64_t ldbd, void *Xd, int64_t ldxd) {
                              return solve_device(S, nrhs, Bd, ldbd, Xd, ldxd, *p, *info, cols, history, st);
                          });
}
