// bsm_minres.cpp -- the bsm_minres_* solver object (include/bsm_rocm.h): the host side of symmetric-preconditioned MINRES
// on up to BSM_CG_MAX_RHS right-hand sides in lockstep, for symmetric / Hermitian operators that need not be definite.  The
// products go through the public bsm_mul_multi / bsm_mul_multi_cvec, the vector work through the kernels of
// bsm_minres.hip.  Every decision of the method is taken on the device; the host only enqueues, rotates the pointers of the
// Lanczos and direction vectors by the parity of the iteration, and reads one record per iteration from a pinned slot, one
// iteration late.  What does not depend on the method is bsm_lockstep.h, shared with bsm_cg.cpp, bsm_bicgstab.cpp and
// bsm_gmres_multi.cpp.
#include <hip/hip_runtime_api.h>

#include <cstdint>
#include <new>

#define BSM_KRYLOV_LAUNCH
#include "bsm_internal.h"
#include "bsm_lockstep.h"
#include "bsm_minres.h"

using namespace bsm;

struct bsm_minres_s : LockstepSolver {
    // in the one allocation: X, R, V0, V1, W0, W1, Q (and Z0, Z1 with M) as ld x kmax, the partials, the state.
    // Iteration j holds v in V[j & 1] and v_old in the other one, which takes v_new; W and Z likewise.
    char *X = nullptr, *R = nullptr, *V[2] = {}, *W[2] = {}, *Q = nullptr, *Z[2] = {};
    char *pzq = nullptr, *pvz = nullptr, *pnn = nullptr, *pbb = nullptr;
    MrState *mr = nullptr;
};

extern "C" int bsm_minres_create(bsm_matrix_t A, int opA, bsm_matrix_t M, int opM, int vdtype, int32_t nrhs_max, struct bsm_minres_s **out) {
    return lockstep_create("bsm_minres", "MINRES", A, opA, M, opM, vdtype, nrhs_max, nullptr, out, [&](bsm_minres_s &S, Carve &cv) {
        const int64_t es = elem_bytes(vdtype), rs = real_bytes(vdtype), K = nrhs_max, vec = S.ld * es * K;
        S.X = cv.take(vec), S.R = cv.take(vec), S.V[0] = cv.take(vec), S.V[1] = cv.take(vec);
        S.W[0] = cv.take(vec), S.W[1] = cv.take(vec), S.Q = cv.take(vec);
        S.Z[0] = M ? cv.take(vec) : nullptr, S.Z[1] = M ? cv.take(vec) : nullptr;
        S.pzq = cv.take(K * S.G * rs), S.pvz = cv.take(K * S.G * rs), S.pnn = cv.take(K * S.G * rs), S.pbb = cv.take(K * S.G * rs);
        S.mr = (MrState *)cv.take((int64_t)sizeof(MrState));
        S.rec = S.mr ? &S.mr->rec : nullptr;
    });
}

extern "C" int bsm_minres_destroy(struct bsm_minres_s *S) { return lockstep_destroy(S); }

namespace {

// the solve on device matrices B, X (arguments checked)
int solve_device(bsm_minres_s *S, int nrhs, const void *B, int64_t ldb, void *X, int64_t ldx, const bsm_cg_params &p, bsm_cg_info &info,
                 bsm_cg_column *cols, double *history, hipStream_t st) {
    const int vt = S->vt;
    const CgDims d{vt, S->n, S->ld, S->G, nrhs, true};
    // z_new = M v_new and the shares of <v_new, z_new> (with M only; without, z IS v and mr_lanczos leaves the shares)
    auto precondition = [&](int par, int slot) -> int {
        if (!S->M) return BSM_OK;
        RC_TRY(apply(S->M, S->opM, S->m_cvec, nrhs, S->ld, S->ld, vt, S->V[slot], S->Z[slot], st));
        HIP_TRY(launch_mr_dot(d, par, S->V[slot], S->Z[slot], S->pvz, S->mr, st));
        return BSM_OK;
    };
    // ---- the start: x, r = v, the norms, z, the first decision
    RC_TRY(lockstep_start_x(S, d, p.use_x0, X, ldx, S->X, S->Q, st));
    HIP_TRY(launch_mr_start(d, B, ldb, p.use_x0 ? S->Q : nullptr, S->R, S->V[0], S->V[1], S->W[0], S->W[1], S->pbb, S->pnn, st));
    RC_TRY(precondition(-1, 0));
    HIP_TRY(launch_mr_decide(d, true, 0, 0, p.rtol, p.atol, S->pbb, S->pnn, S->M ? S->pvz : S->pnn, S->mr, st));
    // ---- the iterations, their records read one behind the enqueue
    RC_TRY(lockstep_run(S, d, X, ldx, S->X, p, info, cols, history, st, [&](int64_t j) -> int {
        const int par = (int)(j & 1), cur = par, old = par ^ 1;
        char *const z = S->M ? S->Z[cur] : S->V[cur];
        RC_TRY(apply(S->A, S->opA, S->a_cvec, nrhs, S->ld, S->ld, vt, z, S->Q, st));
        HIP_TRY(launch_mr_dot(d, par, z, S->Q, S->pzq, S->mr, st));
        HIP_TRY(launch_mr_lanczos(d, par, S->pzq, S->Q, S->V[cur], S->V[old], S->M ? nullptr : S->pvz, S->mr, st));
        RC_TRY(precondition(par, old));
        HIP_TRY(launch_mr_update(d, par, S->pzq, S->pvz, z, S->W[old], S->W[cur], S->X, S->R, S->V[old], S->pnn, S->mr, st));
        HIP_TRY(launch_mr_decide(d, false, par, j + 1, p.rtol, p.atol, S->pbb, S->pnn, S->pvz, S->mr, st));
        return BSM_OK;
    }));
    info.a_products = info.iterations + (p.use_x0 ? 1 : 0);
    info.m_products = S->M ? info.iterations + 1 : 0;
    return BSM_OK;
}

}  // namespace

extern "C" int bsm_minres_solve(struct bsm_minres_s *S, int32_t nrhs, const void *B, int64_t ldb, void *X, int64_t ldx, const bsm_cg_params *p,
                                bsm_cg_info *info, bsm_cg_column *cols, double *history, int memspace, void *stream) {
    const hipStream_t st = (hipStream_t)stream;
    return lockstep_solve(S, "bsm_minres_solve", nrhs, B, ldb, X, ldx, p, info, cols, memspace, st,
                          [&](const void *Bd, int64_t ldbd, void *Xd, int64_t ldxd) {
                              return solve_device(S, nrhs, Bd, ldbd, Xd, ldxd, *p, *info, cols, history, st);
                          });
}
