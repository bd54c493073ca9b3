// bsm_poly.cpp -- composed handles (include/bsm_rocm.h: bsm_poly_create, bsm_poly_info): a polynomial preconditioner
// z = p(A) x over an operator handle A and an optional inner preconditioner handle D, as a bsm_matrix_t of its own, so that
// bsm_mul / bsm_mul_multi and every solver's (M, opM) pair apply it without knowing.  The host side: the refusals of create
// (those of the lockstep solvers, bsm_lockstep.h, and its own), the one device allocation, and the product -- per batch of at
// most nrhs_max columns s - 1 multi-column products with A and s with D through the public bsm_mul_multi / bsm_mul_multi_cvec,
// the vector work between them through the kernels of bsm_poly.hip.  A product allocates nothing and synchronises nothing.
#include <hip/hip_runtime_api.h>

#include <cmath>
#include <cstdint>
#include <memory>
#include <new>

#define BSM_KRYLOV_LAUNCH
#include "bsm_internal.h"
#include "bsm_lockstep.h"
#include "bsm_poly.h"

using namespace bsm;

namespace bsm {

int poly_refusal(const bsm_matrix_s *A, const char *what) {
    if (A && A->poly)
        return fail(BSM_ERR_UNSUPPORTED, std::string(what) + ": not available on a composed handle (bsm_poly_create); it holds no entries of its own");
    return BSM_OK;
}

void poly_release(bsm_matrix_s *M) {
    if (!M->poly) return;
    if (M->poly->ws) (void)hipFree(M->poly->ws);
    M->poly->ws = nullptr;
}

namespace {

bool complex_handle(const bsm_matrix_s *H) { return H->an.dtype == BSM_C64 || H->an.dtype == BSM_C128 || H->an.dtype == BSM_C128_C64; }

// op applied to opH(H) as ONE op of the handle H -> out;  T on C (or C on T) is conj(H): H itself when it is real
int compose(int op, int opH, const bsm_matrix_s *H, int &out) {
    if (op == BSM_OP_N || opH == BSM_OP_N) {
        out = op == BSM_OP_N ? opH : op;
        return BSM_OK;
    }
    if (op != opH && complex_handle(H))
        return fail(BSM_ERR_UNSUPPORTED, "composed handle: this op needs products with conj(A) of a complex handle, which are not available");
    out = BSM_OP_N;
    return BSM_OK;
}

// one scalar of the vector type vt at p (null: dflt) as (re, im)
void read_scalar(const void *p, int vt, double dflt, double *out) {
    out[0] = dflt, out[1] = 0;
    if (!p) return;
    const bool cplx = vt == BSM_C64 || vt == BSM_C128;
    if (real_bytes(vt) == 4) {
        out[0] = ((const float *)p)[0];
        if (cplx) out[1] = ((const float *)p)[1];
    } else {
        out[0] = ((const double *)p)[0];
        if (cplx) out[1] = ((const double *)p)[1];
    }
}

// the layout of the one allocation: R, d, acc, Q (, T with D), each ld x kmax
void layout(PolyState &P, Carve &cv) {
    const int64_t vec = P.ld * elem_bytes(P.vt) * P.kmax;
    P.R = cv.take(vec), P.d = cv.take(vec), P.acc = cv.take(vec), P.Q = cv.take(vec);
    P.T = P.D ? cv.take(vec) : nullptr;
}

// z = p(A) x on kb <= kmax columns: X, Y device matrices (arguments checked), oa / od the composed ops
int poly_batch(PolyState &P, int oa, int od, int kb, const void *X, int64_t ldx, void *Y, int64_t ldy, const double *alpha,
               const double *beta, bool strong, hipStream_t st) {
    const CgDims dm{P.vt, P.n, P.ld, P.G, kb, true};
    auto times = [&](bsm_matrix_s *H, int op, bool cvec, const void *v, void *w) { return apply(H, op, cvec, kb, P.ld, P.ld, P.vt, v, w, st); };
    HIP_TRY(launch_poly_load(dm, X, ldx, P.R, P.D ? nullptr : P.d, P.b[0], st));
    if (P.D) {
        RC_TRY(times(P.D, od, P.d_cvec, P.R, P.T));
        HIP_TRY(launch_poly_dir(dm, true, 0.0, P.b[0], P.T, P.d, st));
    }
    for (int k = 0; k + 1 < P.steps; k++) {
        RC_TRY(times(P.A, oa, P.a_cvec, P.d, P.Q));
        if (!P.D) {
            HIP_TRY(launch_poly_step(dm, k == 0, P.a[k + 1], P.b[k + 1], P.acc, P.R, P.Q, P.d, st));
            continue;
        }
        HIP_TRY(launch_poly_resid(dm, k == 0, P.acc, P.d, P.R, P.Q, st));
        RC_TRY(times(P.D, od, P.d_cvec, P.R, P.T));
        HIP_TRY(launch_poly_dir(dm, false, P.a[k + 1], P.b[k + 1], P.T, P.d, st));
    }
    HIP_TRY(launch_poly_store(dm, alpha, beta, strong, P.steps > 1 ? P.acc : nullptr, P.d, Y, ldy, st));
    return BSM_OK;
}

}  // namespace

// the product of a composed handle behind the four product entry points (bsm_capi.cpp: mul_entry)
int poly_mul(bsm_matrix_s *M, int op, bool cplx, bool multi, int64_t nrhs, const void *X, int64_t ldx, void *Y, int64_t ldy,
             const void *alpha, const void *beta, int beta_strong_zero, int memspace, hipStream_t st) {
    PolyState &P = *M->poly;
    if (cplx)
        return fail(BSM_ERR_UNSUPPORTED, "composed handle: its vectors have the vdtype it was created with (bsm_mul / bsm_mul_multi); for complex "
                                         "vectors over real handles create it with a complex vdtype");
    if (op < 0 || op > 2) return fail(BSM_ERR_INVALID, "bad op");
    if (nrhs < 0) return fail(BSM_ERR_INVALID, "negative nrhs");
    if (nrhs == 0) return BSM_OK;
    if (!X || !Y) return fail(BSM_ERR_INVALID, multi ? "null matrix" : "null vector");
    if (memspace == BSM_MEM_HOST) return fail(BSM_ERR_UNSUPPORTED, "composed handle: device vectors only (BSM_MEM_DEVICE)");
    if (memspace != BSM_MEM_DEVICE) return fail(BSM_ERR_INVALID, "bad memspace");
    const int64_t n1 = std::max<int64_t>(P.n, 1);
    if (!multi) ldx = ldy = n1;
    if (ldx < n1 || ldy < n1) return fail(BSM_ERR_INVALID, "leading dimension smaller than the vector length");
    int oa = 0, od = 0;
    RC_TRY(compose(op, P.opA, P.A, oa));
    if (P.D) RC_TRY(compose(op, P.opD, P.D, od));
    if (capturing(st)) return fail(BSM_ERR_UNSUPPORTED, "composed handle: its product must not be graph-captured");
    if (P.n == 0) return BSM_OK;
    DeviceGuard guard;
    HIP_TRY(guard.enter(M->img.device));
    double al[2], be[2];
    read_scalar(alpha, P.vt, 1.0, al);
    read_scalar(beta, P.vt, 0.0, be);
    const size_t es = (size_t)elem_bytes(P.vt);
    for (int64_t k0 = 0; k0 < nrhs; k0 += P.kmax) {  // more columns than the workspace holds: batches of nrhs_max
        const int kb = (int)std::min<int64_t>(P.kmax, nrhs - k0);
        RC_TRY(poly_batch(P, oa, od, kb, (const char *)X + (size_t)k0 * (size_t)ldx * es, ldx, (char *)Y + (size_t)k0 * (size_t)ldy * es, ldy, al,
                          be, beta_strong_zero != 0, st));
    }
    return BSM_OK;
}

}  // namespace bsm

extern "C" int bsm_poly_create(bsm_matrix_t A, int opA, bsm_matrix_t D, int opD, int vdtype, int32_t nrhs_max, int32_t steps, const double *a,
                               const double *b, bsm_matrix_t *out) {
    BSM_GUARDED(
        if (!out) return fail(BSM_ERR_INVALID, "out is null");
        *out = nullptr;
        const char *bad = nullptr;
        if (steps < 1 || steps > BSM_POLY_MAX_STEPS) bad = "steps outside 1 .. BSM_POLY_MAX_STEPS";
        else if (!a || !b) bad = "null coefficient array";
        else
            for (int32_t k = 0; k < steps; k++)
                if (!std::isfinite(b[k]) || (k > 0 && !std::isfinite(a[k]))) bad = "a coefficient is not finite";
        RC_TRY(lockstep_check_create(A, opA, D, opD, vdtype, nrhs_max, bad));
        LockstepSolver S;  // the refusals of the lockstep solvers, and n, ld, G and the pairings as they carve them
        RC_TRY(lockstep_init(&S, "bsm_poly", A, opA, D, opD, vdtype, nrhs_max));
        if (A->poly || (D && D->poly)) return fail(BSM_ERR_UNSUPPORTED, "bsm_poly: A and D must be operator handles, not composed ones");
        std::unique_ptr<bsm_matrix_s> M(new bsm_matrix_s());
        M->poly.reset(new PolyState());
        PolyState &P = *M->poly;
        P.A = A, P.D = D, P.opA = opA, P.opD = D ? opD : 0, P.vt = vdtype, P.kmax = nrhs_max, P.steps = steps;
        P.a_cvec = S.a_cvec, P.d_cvec = S.m_cvec, P.n = S.n, P.ld = S.ld, P.G = S.G;
        for (int32_t k = 0; k < steps; k++) P.a[k] = k ? a[k] : 0.0, P.b[k] = b[k];
        Carve size;
        layout(P, size);
        P.ws_bytes = size.off;
        {
            DeviceGuard guard;
            hipError_t e = guard.enter(S.device);
            if (e == hipSuccess) e = hipMalloc(&P.ws, (size_t)P.ws_bytes);
            if (e == hipSuccess) e = hipMemset(P.ws, 0, (size_t)P.ws_bytes);  // the padding of the vectors is zero from here on
            if (e != hipSuccess) {
                poly_release(M.get());
                return e == hipErrorOutOfMemory ? fail(BSM_ERR_ALLOC, "out of device memory for the polynomial workspace")
                                                : hip_fail(e, "polynomial workspace");
            }
        }
        Carve cv{(char *)P.ws};
        layout(P, cv);
        // what pairing(), lockstep_init and bsm_stats read of a handle
        M->device = S.device;
        M->an.nrows = M->an.ncols = P.n;
        M->an.dtype = vdtype;
        M->img.dtype = vdtype;
        M->img.device = S.device;
        M->img.nrows = M->img.ncols = P.n;
        M->img.own_lo = 0, M->img.own_hi = P.n;
        M->img.device_bytes = P.ws_bytes;
        M->on_device = true;
        *out = M.release();
        return BSM_OK;)
}

extern "C" int bsm_poly_info(bsm_matrix_t M, int32_t *steps, double *a, double *b, int64_t *workspace_bytes) {
    if (!M) return fail(BSM_ERR_INVALID, "null handle");
    if (!M->poly) return fail(BSM_ERR_INVALID, "not a composed handle (bsm_poly_create)");
    const PolyState &P = *M->poly;
    if (steps) *steps = P.steps;
    for (int k = 0; k < P.steps; k++) {
        if (a) a[k] = P.a[k];
        if (b) b[k] = P.b[k];
    }
    if (workspace_bytes) *workspace_bytes = P.ws_bytes;
    return BSM_OK;
}
