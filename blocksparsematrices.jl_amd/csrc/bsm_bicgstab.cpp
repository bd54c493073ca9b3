// bsm_bicgstab.cpp -- the bsm_bicgstab_* solver object (include/bsm_rocm.h): the host side of right-preconditioned BiCGSTAB
// on up to BSM_CG_MAX_RHS right-hand sides in lockstep, for operators that need not be symmetric.  The products go through
// the public bsm_mul_multi / bsm_mul_multi_cvec, the vector work through the kernels of bsm_bicgstab.hip.  Every decision
// of the method is taken on the device; the host only enqueues, and reads one record per iteration one iteration late.
// Refusals, allocation, staging of host matrices and that loop are bsm_lockstep.h, shared with bsm_cg.cpp.
#include <hip/hip_runtime_api.h>

#include <cstdint>
#include <new>

#define BSM_KRYLOV_LAUNCH
#include "bsm_internal.h"
#include "bsm_bicgstab.h"
#include "bsm_lockstep.h"

using namespace bsm;

struct bsm_bicgstab_s : LockstepSolver {
    // in the one allocation: X, R, Rhat, P, V, T (and Z with M: phat, then shat) as ld x kmax, the partials, the state
    char *X = nullptr, *R = nullptr, *Rhat = nullptr, *P = nullptr, *V = nullptr, *T = nullptr, *Z = nullptr;
    BicgPartials part = {};
};

extern "C" int bsm_bicgstab_create(bsm_matrix_t A, int opA, bsm_matrix_t M, int opM, int vdtype, int32_t nrhs_max,
                                   struct bsm_bicgstab_s **out) {
    if (!out) return fail(BSM_ERR_INVALID, "out is null");
    *out = nullptr;
    int rc = lockstep_check_create(A, opA, M, opM, vdtype, nrhs_max);
    if (rc != BSM_OK) return rc;
    bsm_bicgstab_s *S = new (std::nothrow) bsm_bicgstab_s;
    if (!S) return fail(BSM_ERR_ALLOC, "out of host memory");
    if ((rc = lockstep_init(S, "bsm_bicgstab", A, opA, M, opM, vdtype, nrhs_max)) != BSM_OK) {
        delete S;
        return rc;
    }
    const int64_t es = elem_bytes(vdtype), rs = real_bytes(vdtype), K = nrhs_max;
    Carve cv;
    const int64_t vec = S->ld * es * K, pe = K * S->G * es, pr = K * S->G * rs;
    const int64_t oX = cv.take(vec), oR = cv.take(vec), oH = cv.take(vec), oP = cv.take(vec), oV = cv.take(vec), oT = cv.take(vec);
    const int64_t oZ = M ? cv.take(vec) : 0;
    const int64_t osig = cv.take(pe), oss = cv.take(pr), ots = cv.take(pe), ott = cv.take(pr), onn = cv.take(pr), orho = cv.take(pe),
                  obb = cv.take(pr);
    const int64_t ost = cv.take((int64_t)sizeof(CgState));
    if ((rc = lockstep_alloc(S, cv.off, "BiCGSTAB")) != BSM_OK) {
        delete S;
        return rc;
    }
    char *b = (char *)S->ws;
    S->X = b + oX, S->R = b + oR, S->Rhat = b + oH, S->P = b + oP, S->V = b + oV, S->T = b + oT, S->Z = M ? b + oZ : nullptr;
    S->part = BicgPartials{b + osig, b + oss, b + ots, b + ott, b + onn, b + orho, b + obb};
    S->state = (CgState *)(b + ost);
    *out = S;
    return BSM_OK;
}

extern "C" int bsm_bicgstab_destroy(struct bsm_bicgstab_s *S) {
    if (!S) return BSM_OK;
    lockstep_destroy(S);
    delete S;
    return BSM_OK;
}

namespace {

// the solve on device matrices B, X (arguments checked)
int solve_device(bsm_bicgstab_s *S, int nrhs, const void *B, int64_t ldb, void *X, int64_t ldx, const bsm_cg_params &p, bsm_cg_info &info,
                 bsm_cg_column *cols, double *history, hipStream_t st) {
    const int vt = S->vt, es = elem_bytes(vt);
    const CgDims d{vt, S->n, S->ld, S->G, nrhs, true};
    const size_t vec_bytes = (size_t)S->ld * es * nrhs;
    const BicgPartials &P = S->part;
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
    // what = op(A) opM(M) w: through Z with M, else straight from w.  -> the vector op(A) was applied to
    auto product = [&](const char *w, char *out, const char *&hat) -> int {
        hat = w;
        if (S->M) {
            const int r = apply(S->M, S->opM, S->m_cvec, nrhs, S->ld, vt, w, S->Z, st);
            if (r != BSM_OK) return r;
            hat = S->Z;
        }
        return apply(S->A, S->opA, S->a_cvec, nrhs, S->ld, vt, hat, out, st);
    };
    // ---- the start: x, r = rhat, the norms, p = r, the first decision
    if (p.use_x0) {
        HIP_TRY(launch_cg_copy(d, true, X, ldx, S->X, st));
        RC_TRY(apply(S->A, S->opA, S->a_cvec, nrhs, S->ld, vt, S->X, S->V, st));
    } else {
        HIP_TRY(hipMemsetAsync(S->X, 0, vec_bytes, st));
    }
    HIP_TRY(launch_bicg_start(d, B, ldb, p.use_x0 ? S->V : nullptr, S->R, S->Rhat, P, st));
    HIP_TRY(launch_bicg_dir(d, true, 0, 0, p.rtol, p.atol, P, S->R, S->V, S->P, S->state, st));
    HIP_TRY(lockstep_post(S, 0, st));
    // ---- the iterations, their records read one behind the enqueue
    RC_TRY(lockstep_run(S, d, X, ldx, S->X, p, info, cols, history, st, [&](int64_t j) -> int {
        const int par = (int)(j & 1);
        const char *phat = nullptr, *shat = nullptr;
        RC_TRY(product(S->P, S->V, phat));
        HIP_TRY(launch_bicg_dot(d, par, S->Rhat, S->V, P.sig, nullptr, S->state, st));
        HIP_TRY(launch_bicg_half(d, par, P, phat, S->V, S->X, S->R, S->state, st));
        RC_TRY(product(S->R, S->T, shat));  // (Z is free again: the half step has consumed phat)
        HIP_TRY(launch_bicg_dot(d, par, S->T, S->R, P.ts, P.tt, S->state, st));
        HIP_TRY(launch_bicg_update(d, par, P, S->M ? shat : nullptr, S->T, S->Rhat, S->X, S->R, S->state, st));
        HIP_TRY(launch_bicg_dir(d, false, par, j + 1, p.rtol, p.atol, P, S->R, S->V, S->P, S->state, st));
        return BSM_OK;
    }));
    info.a_products = 2 * info.iterations + (p.use_x0 ? 1 : 0);
    info.m_products = S->M ? 2 * info.iterations : 0;
#undef HIP_TRY
#undef RC_TRY
    return BSM_OK;
}

}  // namespace

extern "C" int bsm_bicgstab_solve(struct bsm_bicgstab_s *S, int32_t nrhs, const void *B, int64_t ldb, void *X, int64_t ldx,
                                  const bsm_cg_params *p, bsm_cg_info *info, bsm_cg_column *cols, double *history, int memspace,
                                  void *stream) {
    const hipStream_t st = (hipStream_t)stream;
    return lockstep_solve(S, "bsm_bicgstab_solve", nrhs, B, ldb, X, ldx, p, info, cols, memspace, st,
                          [&](const void *Bd, int64_t ldbd, void *Xd, int64_t ldxd) {
                              return solve_device(S, nrhs, Bd, ldbd, Xd, ldxd, *p, *info, cols, history, st);
                          });
}
