// bsm_bicgstab.cpp -- the bsm_bicgstab_* solver object (include/bsm_rocm.h): the host side of right-preconditioned BiCGSTAB
// on up to BSM_CG_MAX_RHS right-hand sides in lockstep, for operators that need not be symmetric.  The products go through
// the public bsm_mul_multi / bsm_mul_multi_cvec, the vector work through the kernels of bsm_bicgstab.hip.  Every decision
// of the method is taken on the device; the host only enqueues, and reads one record per iteration one iteration late.
// Create but for the layout of the workspace, the refusals, the staging of host matrices and that loop are bsm_lockstep.h,
// shared with bsm_cg.cpp and bsm_gmres_multi.cpp.
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
    return lockstep_create("bsm_bicgstab", "BiCGSTAB", A, opA, M, opM, vdtype, nrhs_max, nullptr, out, [&](bsm_bicgstab_s &S, Carve &cv) {
        const int64_t es = elem_bytes(vdtype), rs = real_bytes(vdtype), K = nrhs_max;
        const int64_t vec = S.ld * es * K, pe = K * S.G * es, pr = K * S.G * rs;
        S.X = cv.take(vec), S.R = cv.take(vec), S.Rhat = cv.take(vec), S.P = cv.take(vec), S.V = cv.take(vec), S.T = cv.take(vec);
        S.Z = M ? cv.take(vec) : nullptr;
        // (sig, ss, ts, tt, nn, rho, bb: in this order)
        S.part = BicgPartials{cv.take(pe), cv.take(pr), cv.take(pe), cv.take(pr), cv.take(pr), cv.take(pe), cv.take(pr)};
        S.state = (CgState *)cv.take((int64_t)sizeof(CgState));
    });
}

extern "C" int bsm_bicgstab_destroy(struct bsm_bicgstab_s *S) { return lockstep_destroy(S); }

namespace {

// the solve on device matrices B, X (arguments checked)
int solve_device(bsm_bicgstab_s *S, int nrhs, const void *B, int64_t ldb, void *X, int64_t ldx, const bsm_cg_params &p, bsm_cg_info &info,
                 bsm_cg_column *cols, double *history, hipStream_t st) {
    const int vt = S->vt;
    const CgDims d{vt, S->n, S->ld, S->G, nrhs, true};
    const BicgPartials &P = S->part;
    // what = op(A) opM(M) w: through Z with M, else straight from w.  -> the vector op(A) was applied to
    auto product = [&](const char *w, char *out, const char *&hat) -> int {
        hat = w;
        if (S->M) {
            const int r = apply(S->M, S->opM, S->m_cvec, nrhs, S->ld, S->ld, vt, w, S->Z, st);
            if (r != BSM_OK) return r;
            hat = S->Z;
        }
        return apply(S->A, S->opA, S->a_cvec, nrhs, S->ld, S->ld, vt, hat, out, st);
    };
    // ---- the start: x, r = rhat, the norms, p = r, the first decision
    RC_TRY(lockstep_start_x(S, d, p.use_x0, X, ldx, S->X, S->V, st));
    HIP_TRY(launch_bicg_start(d, B, ldb, p.use_x0 ? S->V : nullptr, S->R, S->Rhat, P, st));
    HIP_TRY(launch_bicg_dir(d, true, 0, 0, p.rtol, p.atol, P, S->R, S->V, S->P, S->state, st));
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
