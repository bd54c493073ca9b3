// bsm_cg.cpp -- the bsm_cg_* solver object (include/bsm_rocm.h): the host side of preconditioned CG / COCG on up to
// BSM_CG_MAX_RHS right-hand sides in lockstep.  The products go through the public bsm_mul_multi / bsm_mul_multi_cvec, the
// vector work through the kernels of bsm_cg.hip.  Every decision of the method is taken on the device; the host only
// enqueues, and reads one record per iteration from a pinned slot, one iteration late (the look-ahead), to know when to
// stop enqueuing.  What does not depend on the method -- the refusals, the allocation, the staging of host matrices, that
// loop -- is bsm_lockstep.h, shared with bsm_bicgstab.cpp.
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
    if (!out) return fail(BSM_ERR_INVALID, "out is null");
    *out = nullptr;
    const bool method_ok = method == BSM_CG_METHOD_CG || method == BSM_CG_METHOD_COCG;
    int rc = lockstep_check_create(A, opA, M, opM, vdtype, nrhs_max, method_ok ? nullptr : "method must be BSM_CG_METHOD_CG or BSM_CG_METHOD_COCG");
    if (rc != BSM_OK) return rc;
    bsm_cg_s *S = new (std::nothrow) bsm_cg_s;
    if (!S) return fail(BSM_ERR_ALLOC, "out of host memory");
    if ((rc = lockstep_init(S, "bsm_cg", A, opA, M, opM, vdtype, nrhs_max)) != BSM_OK) {
        delete S;
        return rc;
    }
    S->conj = method == BSM_CG_METHOD_CG;
    const int64_t es = elem_bytes(vdtype), rs = real_bytes(vdtype), K = nrhs_max;
    Carve cv;
    const int64_t vec = S->ld * es * K;
    const int64_t oX = cv.take(vec), oR = cv.take(vec), oP = cv.take(vec), oQ = cv.take(vec), oZ = M ? cv.take(vec) : 0;
    const int64_t opq = cv.take(K * S->G * es), orz = cv.take(K * S->G * es), onn = cv.take(K * S->G * rs), obb = cv.take(K * S->G * rs);
    const int64_t ost = cv.take((int64_t)sizeof(CgState));
    if ((rc = lockstep_alloc(S, cv.off, "CG")) != BSM_OK) {
        delete S;
        return rc;
    }
    char *b = (char *)S->ws;
    S->X = b + oX, S->R = b + oR, S->P = b + oP, S->Q = b + oQ, S->Z = M ? b + oZ : nullptr;
    S->ppq = b + opq, S->prz = b + orz, S->pnn = b + onn, S->pbb = b + obb;
    S->state = (CgState *)(b + ost);
    *out = S;
    return BSM_OK;
}

extern "C" int bsm_cg_destroy(struct bsm_cg_s *S) {
    if (!S) return BSM_OK;
    lockstep_destroy(S);
    delete S;
    return BSM_OK;
}

namespace {

// the solve on device matrices B, X (arguments checked)
int solve_device(bsm_cg_s *S, int nrhs, const void *B, int64_t ldb, void *X, int64_t ldx, const bsm_cg_params &p, bsm_cg_info &info,
                 bsm_cg_column *cols, double *history, hipStream_t st) {
    const int vt = S->vt, es = elem_bytes(vt);
    const CgDims d{vt, S->n, S->ld, S->G, nrhs, S->conj};
    const size_t vec_bytes = (size_t)S->ld * es * nrhs;
    char *const Zv = S->M ? S->Z : S->R;          // z = r without M
    void *const prz_fused = S->M ? nullptr : S->prz;  // without M, cg_start / cg_update leave the shares of <r, r> themselves
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
    // z = M r and the shares of <r, z> (with M only)
    auto precondition = [&](int par) -> int {
        if (!S->M) return BSM_OK;
        const int r = apply(S->M, S->opM, S->m_cvec, nrhs, S->ld, vt, S->R, S->Z, st);
        if (r != BSM_OK) return r;
        const hipError_t q = launch_cg_dot(d, par, S->R, S->Z, S->prz, S->state, st);
        return q == hipSuccess ? BSM_OK : hip_fail(q, "launch_cg_dot");
    };
    // ---- the start: x, r, the norms, p = z, the first decision
    if (p.use_x0) {
        HIP_TRY(launch_cg_copy(d, true, X, ldx, S->X, st));
        RC_TRY(apply(S->A, S->opA, S->a_cvec, nrhs, S->ld, vt, S->X, S->Q, st));
    } else {
        HIP_TRY(hipMemsetAsync(S->X, 0, vec_bytes, st));
    }
    HIP_TRY(launch_cg_start(d, B, ldb, p.use_x0 ? S->Q : nullptr, S->R, S->pbb, S->pnn, prz_fused, S->state, st));
    RC_TRY(precondition(-1));
    HIP_TRY(launch_cg_dir(d, true, 0, 0, p.rtol, p.atol, S->pbb, S->pnn, S->prz, Zv, S->P, S->state, st));
    HIP_TRY(lockstep_post(S, 0, st));
    // ---- the iterations, their records read one behind the enqueue
    RC_TRY(lockstep_run(S, d, X, ldx, S->X, p, info, cols, history, st, [&](int64_t j) -> int {
        const int par = (int)(j & 1);
        RC_TRY(apply(S->A, S->opA, S->a_cvec, nrhs, S->ld, vt, S->P, S->Q, st));
        HIP_TRY(launch_cg_dot(d, par, S->P, S->Q, S->ppq, S->state, st));
        HIP_TRY(launch_cg_update(d, par, S->ppq, S->P, S->Q, S->X, S->R, S->pnn, prz_fused, S->state, st));
        RC_TRY(precondition(par));
        HIP_TRY(launch_cg_dir(d, false, par, j + 1, p.rtol, p.atol, S->pbb, S->pnn, S->prz, Zv, S->P, S->state, st));
        return BSM_OK;
    }));
    info.a_products = info.iterations + (p.use_x0 ? 1 : 0);
    info.m_products = S->M ? info.iterations + 1 : 0;
#undef HIP_TRY
#undef RC_TRY
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
