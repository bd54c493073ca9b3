// bsm_svds.cpp -- the bsm_svds_* solver object and the test hooks bsm_debug_svds_* (include/bsm_rocm.h): the host side of
// thick-restart Golub-Kahan-Lanczos bidiagonalisation with full two-sided reorthogonalisation for a few of the largest or
// smallest singular triplets of a rectangular op(A).  It is the eigen-type solver that uses the transposed half of the engine:
// a step is one product with B and one with B^H, B = op(A) or op(A)^H whichever is tall.  A cycle is enqueued without a host
// read -- per step two products, two Gram-Schmidt passes on either side (bsm_krylov.hip), two norms, two guarded scales
// (bsm_eig.hip) -- and ends with ONE copy of the alpha, the beta and ||v0|| and one synchronisation; the host then decomposes
// the small projected matrix (bsm_svds.h), decides, and restarts through two basis compressions in place (bsm_eig.hip).
#include <hip/hip_runtime_api.h>

#include <cmath>
#include <cstdint>
#include <cstring>
#include <limits>
#include <new>
#include <string>
#include <vector>

#define BSM_KRYLOV_LAUNCH
#include "bsm_internal.h"
#include "bsm_lockstep.h"
#include "bsm_svds.h"

using namespace bsm;

struct bsm_svds_s {
    bsm_matrix_s *A = nullptr;
    int opA = 0, opH = 0, vt = 0, nsv = 0, ncv = 0, device = 0, rcols = 1;
    // op(A) is m x n.  B = op(A) when m >= n, else op(A)^H: l x s with l >= s; opF / opB are B and B^H as ops of the handle
    int64_t m = 0, n = 0, l = 0, s = 0, ld_l = 0, ld_s = 0, ld_m = 0, ld_n = 0;
    int opF = 0, opB = 0, G_l = 1, G_s = 1, G_m = 1, G_n = 1;
    bool tall = true;
    // ONE device allocation: P (ld_s x (ncv + 1)), Q (ld_l x ncv), RM (ld_m x rcols), RN (ld_n x rcols), alpha (ncv reals), beta
    // (ncv + 1 reals: [ncv] is ||v0||), SY and SX (ncv x ncv reals each: the columns of Y and of X a compression takes), sigma (ncv
    // reals), the partials of a Gram-Schmidt pass, of a norm, of the residual pass, the packed scalars, the residuals
    void *ws = nullptr;
    int64_t ws_bytes = 0;
    char *P = nullptr, *Q = nullptr, *RM = nullptr, *RN = nullptr, *alpha = nullptr, *beta = nullptr, *SY = nullptr, *SX = nullptr, *sigma = nullptr,
         *part = nullptr, *nrmpart = nullptr, *rpart = nullptr;
    double *pack = nullptr, *res = nullptr;
    // pinned: what a cycle's copy lands in (2 ncv + 1 doubles), the residuals (2 ncv), and what is uploaded (SY, SX, sigma)
    char *pinned = nullptr;
    double *h_pack = nullptr, *h_res = nullptr;
    char *h_SY = nullptr, *h_SX = nullptr, *h_sigma = nullptr;
    // BSM_MEM_HOST solves: device copies of v0 (s), U (m x nsv) and V (n x nsv), allocated at the first one
    void *hv = nullptr, *hu = nullptr, *hvv = nullptr;
    SvdProjected proj;

    void release() {
        if (ws) (void)hipFree(ws);
        if (hv) (void)hipFree(hv);
        if (hu) (void)hipFree(hu);
        if (hvv) (void)hipFree(hvv);
        if (pinned) (void)hipHostFree(pinned);
        ws = hv = hu = hvv = nullptr;
        pinned = nullptr;
    }
    void layout(Carve &cv) {
        const int64_t es = elem_bytes(vt), rs = real_bytes(vt), G = std::max(G_l, G_s);
        P = cv.take(ld_s * es * (ncv + 1));
        Q = cv.take(ld_l * es * ncv);
        RM = cv.take(ld_m * es * rcols);
        RN = cv.take(ld_n * es * rcols);
        alpha = cv.take(ncv * rs);
        beta = cv.take((ncv + 1) * rs);
        SY = cv.take((int64_t)ncv * ncv * rs);
        SX = cv.take((int64_t)ncv * ncv * rs);
        sigma = cv.take(ncv * rs);
        part = cv.take((int64_t)ncv * G * es);
        nrmpart = cv.take(G * rs);
        rpart = cv.take((int64_t)kCgMaxRhs * (G_m + G_n) * rs);
        pack = (double *)cv.take((2 * ncv + 1) * (int64_t)sizeof(double));
        res = (double *)cv.take(2 * ncv * (int64_t)sizeof(double));
    }
};

extern "C" int bsm_svds_create(bsm_matrix_t A, int opA, int vdtype, int32_t nsv, int32_t ncv, struct bsm_svds_s **out) {
    if (!out) return fail(BSM_ERR_INVALID, "out is null");
    *out = nullptr;
    if (!A) return fail(BSM_ERR_INVALID, "null handle");
    if (opA < 0 || opA > 2) return fail(BSM_ERR_INVALID, "bad op");
    if (!is_vec_type(vdtype)) return fail(BSM_ERR_INVALID, "vdtype must be a vector type (BSM_F32 .. BSM_C128)");
    if (A->poly) return fail(BSM_ERR_UNSUPPORTED, "bsm_svds: composed handles (bsm_poly_create) are not supported");
    if (A->an.dtype < 0 || A->an.dtype > 5 || vec_type(A->an.dtype) != vdtype)
        return fail(BSM_ERR_INVALID, "vdtype must be the handle's own vector type (a real handle under a complex vdtype has no use here)");
    if (A->dist) return fail(BSM_ERR_UNSUPPORTED, "multi-device handles are not supported by bsm_svds");
    if (!A->on_device) return fail(BSM_ERR_DEVICE, "handle has no device image (created with BSM_DEVICE_NONE)");
    if (A->img.own_lo > 0 || A->img.own_hi < A->img.nrows)
        return fail(BSM_ERR_UNSUPPORTED, "handles that own a row range only (bsm_options.own_lo / own_hi) are not supported by bsm_svds");
    const bool cplx = vdtype == BSM_C64 || vdtype == BSM_C128;
    if (opA == BSM_OP_T && cplx)
        return fail(BSM_ERR_UNSUPPORTED, "bsm_svds: opA = BSM_OP_T on a complex handle needs products with conj(A), which are not "
                                         "available; use BSM_OP_N or BSM_OP_C");
    const int64_t m = opA == BSM_OP_N ? A->an.nrows : A->an.ncols, n = opA == BSM_OP_N ? A->an.ncols : A->an.nrows;
    if (nsv < 1 || (int64_t)ncv < (int64_t)nsv + 2 || ncv > std::min<int64_t>(std::min(m, n), BSM_GMRES_MAX_RESTART))
        return fail(BSM_ERR_INVALID, "nsv < 1, or ncv outside nsv + 2 .. min(m, n, BSM_GMRES_MAX_RESTART)");
    bsm_svds_s *S = new (std::nothrow) bsm_svds_s;
    if (!S) return fail(BSM_ERR_ALLOC, "out of host memory");
    const int64_t es = elem_bytes(vdtype);
    auto padded = [&](int64_t rows) { return (std::max<int64_t>(rows, 1) * es + 15) / 16 * 16 / es; };
    S->A = A, S->opA = opA, S->opH = opA == BSM_OP_N ? BSM_OP_C : BSM_OP_N, S->vt = vdtype, S->nsv = nsv, S->ncv = ncv;
    S->device = A->img.device, S->m = m, S->n = n, S->tall = m >= n;
    S->l = std::max(m, n), S->s = std::min(m, n);
    S->opF = S->tall ? S->opA : S->opH, S->opB = S->tall ? S->opH : S->opA;
    S->ld_m = padded(m), S->ld_n = padded(n), S->ld_l = padded(S->l), S->ld_s = padded(S->s);
    S->G_m = krylov_grid(m, (int)es), S->G_n = krylov_grid(n, (int)es);
    S->G_l = std::max(S->G_m, S->G_n), S->G_s = std::min(S->G_m, S->G_n);
    S->rcols = std::min<int>(nsv, kCgMaxRhs);
    Carve size;
    S->layout(size);
    S->ws_bytes = size.off;
    const int64_t pin = (int64_t)sizeof(double) * (2 * ncv + 1 + 2 * ncv + 2 * (int64_t)ncv * ncv + ncv);
    DeviceGuard guard;
    hipError_t e = guard.enter(S->device);
    if (e == hipSuccess) e = hipMalloc(&S->ws, (size_t)size.off);
    if (e == hipSuccess) e = hipMemset(S->ws, 0, (size_t)size.off);
    if (e == hipSuccess) e = hipHostMalloc((void **)&S->pinned, (size_t)pin, hipHostMallocDefault);
    if (e != hipSuccess) {
        S->release();
        delete S;
        return e == hipErrorOutOfMemory ? fail(BSM_ERR_ALLOC, "out of device memory for the svds workspace") : hip_fail(e, "svds workspace");
    }
    Carve cv{(char *)S->ws};
    S->layout(cv);
    S->h_pack = (double *)S->pinned;
    S->h_res = S->h_pack + 2 * ncv + 1;
    S->h_SY = (char *)(S->h_res + 2 * ncv);
    S->h_SX = S->h_SY + (size_t)ncv * ncv * sizeof(double);
    S->h_sigma = S->h_SX + (size_t)ncv * ncv * sizeof(double);
    *out = S;
    return BSM_OK;
}

extern "C" int bsm_svds_destroy(struct bsm_svds_s *S) {
    if (!S) return BSM_OK;
    {
        DeviceGuard guard;
        (void)guard.enter(S->device);
        S->release();
    }
    delete S;
    return BSM_OK;
}

namespace {

// doubles -> the real type of vt
void to_real(int vt, const double *src, size_t count, void *dst) {
    if (real_bytes(vt) == 4) {
        for (size_t i = 0; i < count; i++) ((float *)dst)[i] = (float)src[i];
    } else {
        std::memcpy(dst, src, count * sizeof(double));
    }
}

// uploads columns idx[0 .. k) of the d x d matrix M (Y or X of the projected problem) through the pinned `stage` into `dst` (d x k,
// leading dimension d).  (Every earlier upload has run: a cycle's synchronisation lies between two of them.)
int upload_columns(bsm_svds_s *E, const std::vector<double> &M, const int *idx, int k, char *stage, char *dst, hipStream_t st) {
    const int d = E->proj.d;
    const size_t rs = (size_t)real_bytes(E->vt);
    for (int c = 0; c < k; c++) to_real(E->vt, M.data() + (size_t)idx[c] * d, (size_t)d, stage + (size_t)c * d * rs);
    HIP_TRY(hipMemcpyAsync(dst, stage, (size_t)d * k * rs, hipMemcpyHostToDevice, st));
    return BSM_OK;
}

// column c of a matrix scaled to norm one (zero or not finite: left zero, nothing divided); slot: one real
int unit_column(bsm_svds_s *E, int64_t rows, int G, char *col, char *slot, hipStream_t st) {
    HIP_TRY(launch_krylov_update(E->vt, rows, 0, E->P, E->ld_s, col, E->part, nullptr, E->nrmpart, st));
    HIP_TRY(launch_krylov_norm(E->vt, G, E->nrmpart, slot, st));
    HIP_TRY(launch_eig_scale(E->vt, rows, col, slot, st));
    return BSM_OK;
}

// the solve on device operands (arguments checked)
int solve_device(bsm_svds_s *E, const void *v0, void *U, int64_t ldu, void *V, int64_t ldv, const bsm_svds_params &p, bsm_svds_info &info,
                 bsm_svds_triplet *trip, hipStream_t st) {
    const int vt = E->vt, ncv = E->ncv, nsv = E->nsv;
    const int64_t l = E->l, s = E->s, ld_l = E->ld_l, ld_s = E->ld_s, es = elem_bytes(vt), rs = real_bytes(vt);
    const double one_d[2] = {1, 0}, zero_d[2] = {0, 0};
    const float one_f[2] = {1, 0}, zero_f[2] = {0, 0};
    const bool f = rs == 4;
    const void *one = f ? (const void *)one_f : (const void *)one_d, *zero = f ? (const void *)zero_f : (const void *)zero_d;
    auto pcol = [&](int j) { return E->P + (int64_t)j * ld_s * es; };
    auto qcol = [&](int j) { return E->Q + (int64_t)j * ld_l * es; };
    // w orthogonalised against the k leading columns of `basis` twice, its norm into `nrm`, then the guarded scale
    auto orth_scale = [&](int64_t rows, int64_t ld, int G, const char *basis, int k, char *w, char *nrm) -> int {
        if (k == 0) HIP_TRY(launch_krylov_update(vt, rows, 0, basis, ld, w, E->part, nullptr, E->nrmpart, st));
        for (int pass = 0; pass < 2 && k > 0; pass++) {
            HIP_TRY(launch_krylov_dot(vt, rows, k, basis, ld, w, E->part, st));
            HIP_TRY(launch_krylov_update(vt, rows, k, basis, ld, w, E->part, nullptr, pass ? E->nrmpart : nullptr, st));
        }
        HIP_TRY(launch_krylov_norm(vt, G, E->nrmpart, nrm, st));
        HIP_TRY(launch_eig_scale(vt, rows, w, nrm, st));
        return BSM_OK;
    };
    SvdProjected &Pj = E->proj;
    Pj.reset(ncv);
    // ---- p_0 = v0 / ||v0||
    const CgDims d1{vt, s, ld_s, E->G_s, 1, true};
    HIP_TRY(launch_cg_copy(d1, true, const_cast<void *>(v0), std::max<int64_t>(s, 1), pcol(0), st));
    RC_TRY(orth_scale(s, ld_s, E->G_s, E->P, 0, pcol(0), E->beta + (int64_t)ncv * rs));
    const double nan = std::numeric_limits<double>::quiet_NaN();
    std::vector<int> idx((size_t)ncv);
    int64_t steps = 0;
    int status = -1, nconv = 0;
    double beta_m = 0;
    for (int cycle = 1;; cycle++) {
        info.cycles = cycle;
        for (int j = Pj.start; j < ncv; j++) {
            RC_TRY(bsm_mul(E->A, E->opF, pcol(j), qcol(j), one, zero, 1, BSM_MEM_DEVICE, (void *)st));
            RC_TRY(orth_scale(l, ld_l, E->G_l, E->Q, j, qcol(j), E->alpha + (int64_t)j * rs));
            RC_TRY(bsm_mul(E->A, E->opB, qcol(j), pcol(j + 1), one, zero, 1, BSM_MEM_DEVICE, (void *)st));
            RC_TRY(orth_scale(s, ld_s, E->G_s, E->P, j + 1, pcol(j + 1), E->beta + (int64_t)j * rs));
            steps++;
        }
        // ---- the one copy and the one synchronisation of the cycle
        HIP_TRY(launch_svds_pack(vt, ncv, E->alpha, E->beta, E->pack, st));
        HIP_TRY(hipMemcpyAsync(E->h_pack, E->pack, sizeof(double) * (size_t)(2 * ncv + 1), hipMemcpyDeviceToHost, st));
        HIP_TRY(hipStreamSynchronize(st));
        const double *alpha = E->h_pack, *beta = E->h_pack + ncv, v0norm = beta[ncv];
        if (!std::isfinite(v0norm)) {
            status = 2;
            break;
        }
        if (v0norm == 0.0) {  // a zero start vector: the space is empty
            Pj.d = 0;
            status = 3;
            break;
        }
        Pj.cycle(alpha, beta);
        if (!Pj.finite) {
            status = 2;
            break;
        }
        beta_m = beta[Pj.d - 1];
        if (Pj.d < ncv) {  // the space ended: its triplets are exact
            nconv = std::min(nsv, Pj.d);
            status = Pj.d >= nsv ? 0 : 3;
            svds_select(p.which, Pj.d, nconv, idx.data());
            break;
        }
        svds_select(p.which, Pj.d, nsv, idx.data());
        const double tol = std::max(p.rtol * Pj.anorm, p.atol);
        bool all = true;
        for (int i = 0; i < nsv; i++) all = all && Pj.estimate(idx[i], beta_m) <= tol;
        if (all || cycle >= p.maxcycles) {
            status = all ? 0 : 1;
            nconv = nsv;
            break;
        }
        // ---- the thick restart: P[:, 0:keep] = P[:, 0:ncv] Y[:, kept] in place with p_m carried behind them, Q[:, 0:keep] = Q X[:, kept]
        const int keep = svds_keep(nsv, ncv);
        svds_select(p.which, Pj.d, keep, idx.data());
        Pj.orthonormalise(idx.data(), keep);
        RC_TRY(upload_columns(E, Pj.Y, idx.data(), keep, E->h_SY, E->SY, st));
        RC_TRY(upload_columns(E, Pj.X, idx.data(), keep, E->h_SX, E->SX, st));
        HIP_TRY(launch_eig_combine(vt, s, ncv, keep, E->P, ld_s, E->SY, ncv, E->P, ld_s, ncv, st));
        HIP_TRY(launch_eig_combine(vt, l, ncv, keep, E->Q, ld_l, E->SX, ncv, E->Q, ld_l, -1, st));
        Pj.restart(idx.data(), keep, beta_m);
    }
    info.status = status;
    info.nconv = nconv;
    info.anorm = Pj.anorm;
    info.a_products = 2 * steps;
    for (int i = 0; i < nsv; i++) trip[i].value = trip[i].estimate = trip[i].residual_av = trip[i].residual_ahu = nan;
    for (int i = 0; i < nconv; i++) {
        trip[i].value = Pj.sigma[idx[i]];
        trip[i].estimate = trip[i].residual_ahu = Pj.estimate(idx[i], beta_m);
        trip[i].residual_av = 0.0;  // (B v = sigma u holds by construction; which of the two carries the estimate is set below)
    }
    if (!E->tall)
        for (int i = 0; i < nconv; i++) std::swap(trip[i].residual_av, trip[i].residual_ahu);
    if (!p.vectors || nconv == 0) return BSM_OK;
    // ---- the vectors: right ones of B = P Y[:, wanted] (s rows), left ones = Q X[:, wanted] (l rows); B = op(A)^H exchanges them
    void *right = E->tall ? V : U, *left = E->tall ? U : V;
    const int64_t ldr = E->tall ? ldv : ldu, ldl = E->tall ? ldu : ldv;
    Pj.orthonormalise(idx.data(), nconv);
    RC_TRY(upload_columns(E, Pj.Y, idx.data(), nconv, E->h_SY, E->SY, st));
    RC_TRY(upload_columns(E, Pj.X, idx.data(), nconv, E->h_SX, E->SX, st));
    HIP_TRY(launch_eig_combine(vt, s, Pj.d, nconv, E->P, ld_s, E->SY, Pj.d, right, ldr, -1, st));
    HIP_TRY(launch_eig_combine(vt, l, Pj.d, nconv, E->Q, ld_l, E->SX, Pj.d, left, ldl, -1, st));
    // (a kept column's norm drifts by a rounding error per restart: the vectors leave as unit vectors; the slots of beta are free)
    for (int c = 0; c < nconv; c++) {
        RC_TRY(unit_column(E, s, E->G_s, (char *)right + (int64_t)c * ldr * es, E->beta + (int64_t)c * rs, st));
        RC_TRY(unit_column(E, l, E->G_l, (char *)left + (int64_t)c * ldl * es, E->beta + (int64_t)c * rs, st));
    }
    // ---- the TRUE residuals in batches of the R blocks
    std::vector<double> sg((size_t)nconv);
    for (int i = 0; i < nconv; i++) sg[i] = Pj.sigma[idx[i]];
    to_real(vt, sg.data(), (size_t)nconv, E->h_sigma);
    HIP_TRY(hipMemcpyAsync(E->sigma, E->h_sigma, (size_t)nconv * rs, hipMemcpyHostToDevice, st));
    for (int c0 = 0; c0 < nconv; c0 += E->rcols) {
        const int k = std::min(E->rcols, nconv - c0);
        const char *Ub = (const char *)U + (int64_t)c0 * ldu * es, *Vb = (const char *)V + (int64_t)c0 * ldv * es;
        RC_TRY(bsm_mul_multi(E->A, E->opA, k, Vb, ldv, E->RM, E->ld_m, one, zero, 1, BSM_MEM_DEVICE, (void *)st));
        RC_TRY(bsm_mul_multi(E->A, E->opH, k, Ub, ldu, E->RN, E->ld_n, one, zero, 1, BSM_MEM_DEVICE, (void *)st));
        HIP_TRY(launch_svds_resid(vt, E->m, E->n, k, E->RM, E->ld_m, Ub, ldu, E->RN, E->ld_n, Vb, ldv, E->sigma + (int64_t)c0 * rs, E->rpart,
                                  E->res + c0, E->res + nconv + c0, st));  // packed: r_av in [0, nconv), r_ahu behind them
    }
    info.a_products += 2 * nconv;
    HIP_TRY(hipMemcpyAsync(E->h_res, E->res, sizeof(double) * (size_t)(2 * nconv), hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    for (int i = 0; i < nconv; i++) {
        trip[i].residual_av = E->h_res[i];
        trip[i].residual_ahu = E->h_res[nconv + i];
    }
    return BSM_OK;
}

}  // namespace

extern "C" int bsm_svds_solve(struct bsm_svds_s *S, const void *v0, void *U, int64_t ldu, void *V, int64_t ldv, const bsm_svds_params *p,
                              bsm_svds_info *info, bsm_svds_triplet *trip, int memspace, void *stream) {
    if (!S || !p || !info || !trip || !v0) return fail(BSM_ERR_INVALID, "null argument");
    if (p->struct_size != (int32_t)sizeof(bsm_svds_params)) return fail(BSM_ERR_INVALID, "bsm_svds_params.struct_size mismatch");
    if (memspace != BSM_MEM_HOST && memspace != BSM_MEM_DEVICE) return fail(BSM_ERR_INVALID, "bad memspace");
    if (p->which != kSvdsLM && p->which != kSvdsSM) return fail(BSM_ERR_INVALID, "which must be BSM_SVDS_LM or BSM_SVDS_SM");
    if (!(p->rtol >= 0) || !(p->atol >= 0) || p->maxcycles < 1) return fail(BSM_ERR_INVALID, "rtol and atol must be >= 0, maxcycles >= 1");
    const int64_t m = S->m, n = S->n;
    const size_t es = (size_t)elem_bytes(S->vt);
    if (p->vectors) {
        if (!U || !V) return fail(BSM_ERR_INVALID, "null matrix");
        if (ldu < std::max<int64_t>(m, 1) || ldv < std::max<int64_t>(n, 1)) return fail(BSM_ERR_INVALID, "ldu < max(m, 1) or ldv < max(n, 1)");
        const size_t ub = ((size_t)(S->nsv - 1) * (size_t)ldu + (size_t)m) * es, vb = ((size_t)(S->nsv - 1) * (size_t)ldv + (size_t)n) * es;
        if (overlap(v0, (size_t)S->s * es, U, ub) || overlap(v0, (size_t)S->s * es, V, vb)) return fail(BSM_ERR_INVALID, "U and V must not overlap v0");
        if (overlap(U, ub, V, vb)) return fail(BSM_ERR_INVALID, "U and V must not overlap");
    }
    const hipStream_t st = (hipStream_t)stream;
    if (capturing(st)) return fail(BSM_ERR_INVALID, "bsm_svds_solve must not be graph-captured");
    std::memset(info, 0, sizeof(*info));
    info->workspace_bytes = S->ws_bytes;
    info->workspace = (uint64_t)(uintptr_t)S->ws;
    DeviceGuard guard;
    hipError_t e = guard.enter(S->device);
    if (e != hipSuccess) return hip_fail(e, "hipSetDevice");
    BSM_GUARDED({
        if (memspace == BSM_MEM_DEVICE) return solve_device(S, v0, U, ldu, V, ldv, *p, *info, trip, st);
        // host operands: staged through dense buffers the solver keeps
        const size_t ucol = (size_t)m * es, vcol = (size_t)n * es;
        if (!S->hv) e = hipMalloc(&S->hv, (size_t)S->s * es + 16);
        if (e == hipSuccess && !S->hu) e = hipMalloc(&S->hu, ucol * (size_t)S->nsv + 16);
        if (e == hipSuccess && !S->hvv) e = hipMalloc(&S->hvv, vcol * (size_t)S->nsv + 16);
        if (e != hipSuccess) {
            if (e != hipErrorOutOfMemory) return hip_fail(e, "staging buffers");
            (void)hipGetLastError();
            return fail(BSM_ERR_ALLOC, "out of device memory for the staging buffers");
        }
        e = hipMemcpyAsync(S->hv, v0, (size_t)S->s * es, hipMemcpyHostToDevice, st);
        if (e != hipSuccess) return hip_fail(e, "host-staged solve");
        const int rc = solve_device(S, S->hv, S->hu, std::max<int64_t>(m, 1), S->hvv, std::max<int64_t>(n, 1), *p, *info, trip, st);
        if (rc != BSM_OK) return rc;
        if (p->vectors) {
            for (int c = 0; c < info->nconv && e == hipSuccess; c++) {
                e = hipMemcpyAsync((char *)U + (size_t)c * (size_t)ldu * es, (char *)S->hu + c * ucol, ucol, hipMemcpyDeviceToHost, st);
                if (e == hipSuccess) e = hipMemcpyAsync((char *)V + (size_t)c * (size_t)ldv * es, (char *)S->hvv + c * vcol, vcol, hipMemcpyDeviceToHost, st);
            }
            if (e == hipSuccess) e = hipStreamSynchronize(st);
            if (e != hipSuccess) return hip_fail(e, "host-staged solve");
        }
        return BSM_OK;
    })
}

// ---- test hooks (unexported in the header, like bsm_debug_eig_jacobi); none needs a device ---------------------------------
// svds_jacobi of bsm_svds.h on B (m x m, column-major, ldb >= m; not written): sigma descending, X, Y (m x m) -> the sweeps taken
extern "C" int bsm_debug_svds_jacobi(int32_t m, const double *B, int64_t ldb, double *sigma, double *X, double *Y, int32_t *sweeps) {
    if (m < 1 || m > 4096 || !B || ldb < m || !sigma || !X || !Y) return fail(BSM_ERR_INVALID, "bad argument");
    BSM_GUARDED({
        std::vector<double> work((size_t)m * m);
        for (int c = 0; c < m; c++)
            for (int r = 0; r < m; r++) work[(size_t)r + (size_t)c * m] = B[(size_t)r + (size_t)c * ldb];
        const int sw = svds_jacobi(m, work.data(), sigma, X, Y);
        if (sweeps) *sweeps = sw;
        return BSM_OK;
    })
}
// svds_select: the `count` of m descending values that `which` wants, in its order -> idx (0-based)
extern "C" int bsm_debug_svds_select(int which, int32_t m, int32_t count, int32_t *idx) {
    if ((which != kSvdsLM && which != kSvdsSM) || m < 0 || count < 0 || count > m || !idx) return fail(BSM_ERR_INVALID, "bad argument");
    svds_select(which, m, count, idx);
    return BSM_OK;
}
extern "C" int bsm_debug_svds_keep(int32_t nsv, int32_t ncv) { return svds_keep(nsv, ncv); }
// SvdProjected over `cycles` cycles of ncv alpha / beta each (rows of alpha, beta: cycles x ncv, row-major; entries below the
// cycle's start are not read), restarting on the `keep` triplets `which` selects after every cycle but the last:
// -> d, the sigma (d), the estimates (d) of the last cycle, and the kept values and arrow (keep each) it started from
extern "C" int bsm_debug_svds_cycles(int which, int32_t nsv, int32_t ncv, int32_t cycles, const double *alpha, const double *beta, int32_t *d,
                                     double *sigma, double *estimate, double *kept, double *arrow) {
    if ((which != kSvdsLM && which != kSvdsSM) || nsv < 1 || ncv < nsv + 2 || cycles < 1 || !alpha || !beta || !d || !sigma || !estimate)
        return fail(BSM_ERR_INVALID, "bad argument");
    BSM_GUARDED({
        SvdProjected P;
        P.reset(ncv);
        std::vector<int> idx((size_t)ncv);
        const int keep = svds_keep(nsv, ncv);
        for (int c = 0; c < cycles; c++) {
            const double *a = alpha + (size_t)c * ncv, *b = beta + (size_t)c * ncv;
            P.cycle(a, b);
            if (!P.finite || P.d < ncv || c + 1 == cycles) {
                *d = P.finite ? P.d : -1;
                for (int i = 0; i < P.d; i++) sigma[i] = P.sigma[i], estimate[i] = P.estimate(i, b[P.d - 1]);
                for (int i = 0; i < P.start && kept && arrow; i++) kept[i] = P.kept[i], arrow[i] = P.arrow[i];
                return BSM_OK;
            }
            svds_select(which, P.d, keep, idx.data());
            P.orthonormalise(idx.data(), keep);
            P.restart(idx.data(), keep, b[P.d - 1]);
        }
        return BSM_OK;
    })
}
