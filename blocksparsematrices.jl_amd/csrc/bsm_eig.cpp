// bsm_eig.cpp -- bsm_krylov_combine, the bsm_eigsh_* solver object and the test hooks bsm_debug_eig_* (include/bsm_rocm.h): the
// host side of thick-restart Lanczos (the Hermitian Krylov-Schur method) for a few extreme eigenpairs of a symmetric /
// Hermitian op(A).  A cycle is enqueued without a host read -- product, two Gram-Schmidt passes (bsm_krylov.hip), norm,
// guarded scale per step -- and ends with ONE copy of diag(H), beta and ||v0|| and one synchronisation; the host then
// diagonalises the small projected matrix (bsm_eig.h), decides, and restarts through bsm_krylov_combine in place.
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
#include "bsm_eig.h"

using namespace bsm;

// ---- bsm_krylov_combine -----------------------------------------------------------------------------------------------------
extern "C" int64_t bsm_krylov_combine_tile(int dtype, int64_t m) {
    if (!is_vec_type(dtype) || m < 1 || m > BSM_GMRES_MAX_RESTART) return (int64_t)fail(BSM_ERR_INVALID, "bad argument");
    return combine_tile_reals(m, real_bytes(dtype)) / (elem_bytes(dtype) / real_bytes(dtype));
}

extern "C" int bsm_krylov_combine(int dtype, int64_t n, int64_t m, int64_t k, const void *V, int64_t ldv, const void *S, int64_t lds,
                                  void *Out, int64_t ldo, int64_t carry, void *stream) {
    const std::string why = vec_type_refusal("bsm_krylov_combine", dtype);
    if (!why.empty()) return fail(BSM_ERR_INVALID, why);
    if (n < 0 || m < 1 || m > BSM_GMRES_MAX_RESTART) return fail(BSM_ERR_INVALID, "n < 0, or m outside 1 .. BSM_GMRES_MAX_RESTART");
    if (k < 0 || k > m || carry < -1 || carry > m) return fail(BSM_ERR_INVALID, "k outside 0 .. m, or carry outside -1 .. m");
    if (ldv < std::max<int64_t>(n, 1) || ldo < std::max<int64_t>(n, 1) || lds < m) return fail(BSM_ERR_INVALID, "ldv / ldo < max(n, 1), or lds < m");
    if ((k > 0 && !S) || (n > 0 && (!V || !Out))) return fail(BSM_ERR_INVALID, "null argument");
    const int64_t vcols = std::max<int64_t>(m, carry + 1), ocols = k + (carry >= 0 ? 1 : 0);
    const size_t es = (size_t)elem_bytes(dtype);
    if (n > 0 && ocols > 0 && !(Out == V && ldo == ldv) &&
        overlap(V, ((size_t)(vcols - 1) * (size_t)ldv + (size_t)n) * es, Out, ((size_t)(ocols - 1) * (size_t)ldo + (size_t)n) * es))
        return fail(BSM_ERR_INVALID, "Out overlaps V (only Out == V with ldo == ldv works in place)");
    if (n > 0 && ocols > 0 && k > 0 &&
        overlap(S, ((size_t)(k - 1) * (size_t)lds + (size_t)m) * (size_t)real_bytes(dtype), Out, ((size_t)(ocols - 1) * (size_t)ldo + (size_t)n) * es))
        return fail(BSM_ERR_INVALID, "S overlaps Out (other workgroups would read it while it is written)");
    const hipStream_t st = (hipStream_t)stream;
    // the launch goes to the device of `stream` when one is given (nothing is allocated, so this is capture-safe)
    DeviceGuard guard;
    int dev = -1;
    if (st && hipStreamGetDevice(st, &dev) == hipSuccess) {
        const hipError_t g = guard.enter(dev);
        if (g != hipSuccess) return hip_fail(g, "hipSetDevice");
    } else {
        (void)hipGetLastError();
    }
    const hipError_t e = launch_eig_combine(dtype, n, (int)m, (int)k, V, ldv, S, lds, Out, ldo, (int)carry, st);
    if (e != hipSuccess) return hip_fail(e, "combine launch");
    return BSM_OK;
}

// ---- bsm_eigsh_* ------------------------------------------------------------------------------------------------------------
struct bsm_eigsh_s {
    bsm_matrix_s *A = nullptr;
    int opA = 0, vt = 0, nev = 0, ncv = 0, device = 0, G = 1, qcols = 1;
    int64_t n = 0, ld = 0;
    // ONE device allocation: V (ld x (ncv + 1)), Q (ld x qcols), H (ncv x ncv), beta (ncv + 1 reals: [ncv] is ||v0||), S (ncv x
    // ncv reals), theta (ncv reals), the partials of a Gram-Schmidt pass, of the residual pass, the packed scalars, the residuals
    void *ws = nullptr;
    int64_t ws_bytes = 0;
    char *V = nullptr, *Q = nullptr, *H = nullptr, *beta = nullptr, *S = nullptr, *theta = nullptr, *part = nullptr, *nrmpart = nullptr,
         *rpart = nullptr;
    double *pack = nullptr, *res = nullptr;
    // pinned: what a cycle's copy lands in (2 ncv + 1 doubles), the residuals (ncv), and what is uploaded (S, theta)
    char *pinned = nullptr;
    double *h_pack = nullptr, *h_res = nullptr;
    char *h_S = nullptr, *h_theta = nullptr;
    // BSM_MEM_HOST solves: device copies of v0 (n) and X (n x nev), allocated at the first one
    void *hv = nullptr, *hx = nullptr;
    EigProjected proj;

    void release() {
        if (ws) (void)hipFree(ws);
        if (hv) (void)hipFree(hv);
        if (hx) (void)hipFree(hx);
        if (pinned) (void)hipHostFree(pinned);
        ws = hv = hx = nullptr;
        pinned = nullptr;
    }
    void layout(Carve &cv) {
        const int64_t es = elem_bytes(vt), rs = real_bytes(vt);
        V = cv.take(ld * es * (ncv + 1));
        Q = cv.take(ld * es * qcols);
        H = cv.take((int64_t)ncv * ncv * es);
        beta = cv.take((ncv + 1) * rs);
        S = cv.take((int64_t)ncv * ncv * rs);
        theta = cv.take(ncv * rs);
        part = cv.take((int64_t)ncv * G * es);
        nrmpart = cv.take(G * rs);
        rpart = cv.take((int64_t)kCgMaxRhs * G * rs);
        pack = (double *)cv.take((2 * ncv + 1) * (int64_t)sizeof(double));
        res = (double *)cv.take(ncv * (int64_t)sizeof(double));
    }
};

extern "C" int bsm_eigsh_create(bsm_matrix_t A, int opA, int vdtype, int32_t nev, int32_t ncv, struct bsm_eigsh_s **out) {
    if (!out) return fail(BSM_ERR_INVALID, "out is null");
    *out = nullptr;
    if (!A) return fail(BSM_ERR_INVALID, "null handle");
    if (opA < 0 || opA > 2) return fail(BSM_ERR_INVALID, "bad op");
    if (!is_vec_type(vdtype)) return fail(BSM_ERR_INVALID, "vdtype must be a vector type (BSM_F32 .. BSM_C128)");
    if (A->poly) return fail(BSM_ERR_UNSUPPORTED, "bsm_eigsh: composed handles (bsm_poly_create) are not supported");
    if (A->an.nrows != A->an.ncols) return fail(BSM_ERR_INVALID, "op(A) is not square");
    if (A->an.dtype < 0 || A->an.dtype > 5 || vec_type(A->an.dtype) != vdtype)
        return fail(BSM_ERR_INVALID, "vdtype must be the handle's own vector type (a real handle under a complex vdtype has no use here)");
    if (A->dist) return fail(BSM_ERR_UNSUPPORTED, "multi-device handles are not supported by bsm_eigsh");
    if (!A->on_device) return fail(BSM_ERR_DEVICE, "handle has no device image (created with BSM_DEVICE_NONE)");
    if (A->img.own_lo > 0 || A->img.own_hi < A->img.nrows)
        return fail(BSM_ERR_UNSUPPORTED, "handles that own a row range only (bsm_options.own_lo / own_hi) are not supported by bsm_eigsh");
    const int64_t n = A->an.nrows;
    if (nev < 1 || (int64_t)ncv < (int64_t)nev + 2 || ncv > std::min<int64_t>(n, BSM_GMRES_MAX_RESTART))
        return fail(BSM_ERR_INVALID, "nev < 1, or ncv outside nev + 2 .. min(n, BSM_GMRES_MAX_RESTART)");
    bsm_eigsh_s *S = new (std::nothrow) bsm_eigsh_s;
    if (!S) return fail(BSM_ERR_ALLOC, "out of host memory");
    const int64_t es = elem_bytes(vdtype);
    S->A = A, S->opA = opA, S->vt = vdtype, S->nev = nev, S->ncv = ncv, S->device = A->img.device, S->n = n;
    S->ld = (std::max<int64_t>(n, 1) * es + 15) / 16 * 16 / es;
    S->G = krylov_grid(n, (int)es);
    S->qcols = std::min<int>(nev, kCgMaxRhs);
    Carve size;
    S->layout(size);
    S->ws_bytes = size.off;
    const int64_t pin = (int64_t)sizeof(double) * (2 * ncv + 1 + ncv + (int64_t)ncv * ncv + ncv);
    DeviceGuard guard;
    hipError_t e = guard.enter(S->device);
    if (e == hipSuccess) e = hipMalloc(&S->ws, (size_t)size.off);
    if (e == hipSuccess) e = hipMemset(S->ws, 0, (size_t)size.off);
    if (e == hipSuccess) e = hipHostMalloc((void **)&S->pinned, (size_t)pin, hipHostMallocDefault);
    if (e != hipSuccess) {
        S->release();
        delete S;
        return e == hipErrorOutOfMemory ? fail(BSM_ERR_ALLOC, "out of device memory for the eigsh workspace") : hip_fail(e, "eigsh workspace");
    }
    Carve cv{(char *)S->ws};
    S->layout(cv);
    S->h_pack = (double *)S->pinned;
    S->h_res = S->h_pack + 2 * ncv + 1;
    S->h_S = (char *)(S->h_res + ncv);
    S->h_theta = S->h_S + (size_t)ncv * ncv * sizeof(double);
    *out = S;
    return BSM_OK;
}

extern "C" int bsm_eigsh_destroy(struct bsm_eigsh_s *S) {
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

// uploads columns idx[0 .. k) of the d x d eigenvector matrix as S (d x k, leading dimension d) and their theta
int upload_selection(bsm_eigsh_s *E, const int *idx, int k, hipStream_t st) {
    const EigProjected &P = E->proj;
    const int d = P.d;
    const size_t rs = (size_t)real_bytes(E->vt);
    std::vector<double> th((size_t)k);
    for (int c = 0; c < k; c++) {
        to_real(E->vt, P.S.data() + (size_t)idx[c] * d, (size_t)d, E->h_S + (size_t)c * d * rs);
        th[c] = P.theta[idx[c]];
    }
    to_real(E->vt, th.data(), (size_t)k, E->h_theta);
    HIP_TRY(hipMemcpyAsync(E->S, E->h_S, (size_t)d * k * rs, hipMemcpyHostToDevice, st));
    HIP_TRY(hipMemcpyAsync(E->theta, E->h_theta, (size_t)k * rs, hipMemcpyHostToDevice, st));
    return BSM_OK;
}

// the solve on device operands (arguments checked)
int solve_device(bsm_eigsh_s *E, const void *v0, void *X, int64_t ldx, const bsm_eigsh_params &p, bsm_eigsh_info &info, bsm_eigsh_pair *pairs,
                 hipStream_t st) {
    const int vt = E->vt, ncv = E->ncv, nev = E->nev, G = E->G;
    const int64_t n = E->n, ld = E->ld, es = elem_bytes(vt), rs = real_bytes(vt);
    const double one_d[2] = {1, 0}, zero_d[2] = {0, 0};
    const float one_f[2] = {1, 0}, zero_f[2] = {0, 0};
    const bool f = rs == 4;
    const void *one = f ? (const void *)one_f : (const void *)one_d, *zero = f ? (const void *)zero_f : (const void *)zero_d;
    auto col = [&](int j) { return E->V + (int64_t)j * ld * es; };
    EigProjected &P = E->proj;
    P.reset(ncv);
    // ---- v_0 = v0 / ||v0||
    const CgDims d1{vt, n, ld, G, 1, true};
    HIP_TRY(launch_cg_copy(d1, true, const_cast<void *>(v0), std::max<int64_t>(n, 1), col(0), st));
    HIP_TRY(launch_krylov_update(vt, n, 0, E->V, ld, col(0), E->part, nullptr, E->nrmpart, st));
    HIP_TRY(launch_krylov_norm(vt, G, E->nrmpart, E->beta + (int64_t)ncv * rs, st));
    HIP_TRY(launch_eig_scale(vt, n, col(0), E->beta + (int64_t)ncv * rs, st));
    const double nan = std::numeric_limits<double>::quiet_NaN();
    std::vector<int> idx((size_t)ncv);
    int64_t steps = 0;
    int status = -1, nconv = 0;
    double beta_m = 0;
    for (int cycle = 1;; cycle++) {
        info.cycles = cycle;
        HIP_TRY(hipMemsetAsync(E->H, 0, (size_t)ncv * ncv * es, st));
        for (int j = P.start; j < ncv; j++) {
            char *w = col(j + 1), *hcol = E->H + (int64_t)j * ncv * es;
            RC_TRY(bsm_mul(E->A, E->opA, col(j), w, one, zero, 1, BSM_MEM_DEVICE, (void *)st));
            for (int pass = 0; pass < 2; pass++) {
                HIP_TRY(launch_krylov_dot(vt, n, j + 1, E->V, ld, w, E->part, st));
                HIP_TRY(launch_krylov_update(vt, n, j + 1, E->V, ld, w, E->part, hcol, pass ? E->nrmpart : nullptr, st));
            }
            HIP_TRY(launch_krylov_norm(vt, G, E->nrmpart, E->beta + (int64_t)j * rs, st));
            HIP_TRY(launch_eig_scale(vt, n, w, E->beta + (int64_t)j * rs, st));
            steps++;
        }
        // ---- the one copy and the one synchronisation of the cycle
        HIP_TRY(launch_eig_pack(vt, ncv, E->H, E->beta, E->pack, st));
        HIP_TRY(hipMemcpyAsync(E->h_pack, E->pack, sizeof(double) * (size_t)(2 * ncv + 1), hipMemcpyDeviceToHost, st));
        HIP_TRY(hipStreamSynchronize(st));
        const double *alpha = E->h_pack, *beta = E->h_pack + ncv, v0norm = beta[ncv];
        if (!std::isfinite(v0norm)) {
            status = 2;
            break;
        }
        if (v0norm == 0.0) {  // a zero start vector: the Krylov space is empty
            P.d = 0;
            status = 3;
            break;
        }
        P.cycle(alpha, beta);
        if (!P.finite) {
            status = 2;
            break;
        }
        beta_m = beta[P.d - 1];
        if (P.d < ncv) {  // the space ended: its Ritz pairs are exact
            nconv = std::min(nev, P.d);
            status = P.d >= nev ? 0 : 3;
            eig_select(p.which, P.d, P.theta.data(), nconv, idx.data());
            break;
        }
        eig_select(p.which, P.d, P.theta.data(), nev, idx.data());
        const double tol = std::max(p.rtol * P.anorm, p.atol);
        bool all = true;
        for (int i = 0; i < nev; i++) all = all && P.estimate(idx[i], beta_m) <= tol;
        if (all || cycle >= p.maxcycles) {
            status = all ? 0 : 1;
            nconv = nev;
            break;
        }
        // ---- the thick restart: V[:, 0:keep] = V[:, 0:ncv] S in place, v_m carried behind them
        const int keep = eig_keep(nev, ncv);
        eig_select(p.which, P.d, P.theta.data(), keep, idx.data());
        P.orthonormalise(idx.data(), keep);
        RC_TRY(upload_selection(E, idx.data(), keep, st));
        HIP_TRY(launch_eig_combine(vt, n, ncv, keep, E->V, ld, E->S, ncv, E->V, ld, ncv, st));
        P.restart(idx.data(), keep, beta_m);
    }
    info.status = status;
    info.nconv = nconv;
    info.anorm = P.anorm;
    info.a_products = steps;
    for (int i = 0; i < nev; i++) pairs[i].value = pairs[i].estimate = pairs[i].residual = nan;
    for (int i = 0; i < nconv; i++) {
        pairs[i].value = P.theta[idx[i]];
        pairs[i].estimate = pairs[i].residual = P.estimate(idx[i], beta_m);
    }
    if (!p.vectors || nconv == 0) return BSM_OK;
    // ---- X = V S[:, wanted], then the true residuals in batches of the Q block
    P.orthonormalise(idx.data(), nconv);
    RC_TRY(upload_selection(E, idx.data(), nconv, st));
    HIP_TRY(launch_eig_combine(vt, n, P.d, nconv, E->V, ld, E->S, P.d, X, ldx, -1, st));
    // (a kept column's norm drifts by a rounding error per restart: the vectors leave as unit vectors; the slots of beta are free)
    for (int c = 0; c < nconv; c++) {
        char *xc = (char *)X + (int64_t)c * ldx * es, *slot = E->beta + (int64_t)c * rs;
        HIP_TRY(launch_krylov_update(vt, n, 0, E->V, ld, xc, E->part, nullptr, E->nrmpart, st));
        HIP_TRY(launch_krylov_norm(vt, G, E->nrmpart, slot, st));
        HIP_TRY(launch_eig_scale(vt, n, xc, slot, st));
    }
    for (int c0 = 0; c0 < nconv; c0 += E->qcols) {
        const int k = std::min(E->qcols, nconv - c0);
        const char *Xb = (const char *)X + (int64_t)c0 * ldx * es;
        RC_TRY(bsm_mul_multi(E->A, E->opA, k, Xb, ldx, E->Q, ld, one, zero, 1, BSM_MEM_DEVICE, (void *)st));
        HIP_TRY(launch_eig_resid(vt, n, k, E->Q, ld, Xb, ldx, E->theta + (int64_t)c0 * rs, E->rpart, E->res + c0, st));
    }
    info.a_products += nconv;
    HIP_TRY(hipMemcpyAsync(E->h_res, E->res, sizeof(double) * (size_t)nconv, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    for (int i = 0; i < nconv; i++) pairs[i].residual = E->h_res[i];
    return BSM_OK;
}

}  // namespace

extern "C" int bsm_eigsh_solve(struct bsm_eigsh_s *S, const void *v0, void *X, int64_t ldx, const bsm_eigsh_params *p, bsm_eigsh_info *info,
                               bsm_eigsh_pair *pairs, int memspace, void *stream) {
    if (!S || !p || !info || !pairs || !v0) return fail(BSM_ERR_INVALID, "null argument");
    if (p->struct_size != (int32_t)sizeof(bsm_eigsh_params)) return fail(BSM_ERR_INVALID, "bsm_eigsh_params.struct_size mismatch");
    if (memspace != BSM_MEM_HOST && memspace != BSM_MEM_DEVICE) return fail(BSM_ERR_INVALID, "bad memspace");
    if (p->which < kEigLA || p->which > kEigLM) return fail(BSM_ERR_INVALID, "which must be BSM_EIGSH_LA, _SA, _BE or _LM");
    if (!(p->rtol >= 0) || !(p->atol >= 0) || p->maxcycles < 1) return fail(BSM_ERR_INVALID, "rtol and atol must be >= 0, maxcycles >= 1");
    const int64_t n = S->n;
    const size_t es = (size_t)elem_bytes(S->vt);
    if (p->vectors) {
        if (!X) return fail(BSM_ERR_INVALID, "null matrix");
        if (ldx < std::max<int64_t>(n, 1)) return fail(BSM_ERR_INVALID, "ldx < max(n, 1)");
        if (overlap(v0, (size_t)n * es, X, ((size_t)(S->nev - 1) * (size_t)ldx + (size_t)n) * es)) return fail(BSM_ERR_INVALID, "X must not overlap v0");
    }
    const hipStream_t st = (hipStream_t)stream;
    if (capturing(st)) return fail(BSM_ERR_INVALID, "bsm_eigsh_solve must not be graph-captured");
    std::memset(info, 0, sizeof(*info));
    info->workspace_bytes = S->ws_bytes;
    info->workspace = (uint64_t)(uintptr_t)S->ws;
    DeviceGuard guard;
    hipError_t e = guard.enter(S->device);
    if (e != hipSuccess) return hip_fail(e, "hipSetDevice");
    BSM_GUARDED({
        if (memspace == BSM_MEM_DEVICE) return solve_device(S, v0, X, ldx, *p, *info, pairs, st);
        // host operands: staged through dense buffers the solver keeps
        const size_t colb = (size_t)n * es;
        if (!S->hv) e = hipMalloc(&S->hv, colb + 16);
        if (e == hipSuccess && !S->hx) e = hipMalloc(&S->hx, colb * (size_t)S->nev + 16);
        if (e != hipSuccess) {
            if (e != hipErrorOutOfMemory) return hip_fail(e, "staging buffers");
            (void)hipGetLastError();
            return fail(BSM_ERR_ALLOC, "out of device memory for the staging buffers");
        }
        e = hipMemcpyAsync(S->hv, v0, colb, hipMemcpyHostToDevice, st);
        if (e != hipSuccess) return hip_fail(e, "host-staged solve");
        const int rc = solve_device(S, S->hv, S->hx, n, *p, *info, pairs, st);
        if (rc != BSM_OK) return rc;
        if (p->vectors) {
            for (int c = 0; c < info->nconv && e == hipSuccess; c++)
                e = hipMemcpyAsync((char *)X + (size_t)c * (size_t)ldx * es, (char *)S->hx + c * colb, colb, hipMemcpyDeviceToHost, st);
            if (e == hipSuccess) e = hipStreamSynchronize(st);
            if (e != hipSuccess) return hip_fail(e, "host-staged solve");
        }
        return BSM_OK;
    })
}

// ---- test hooks (unexported in the header, like bsm_debug_krylov_lsq_host); none needs a device ----------------------------
// eig_jacobi of bsm_eig.h on T (m x m, column-major, ldt >= m; not written): theta ascending, S (m x m) the eigenvectors
extern "C" int bsm_debug_eig_jacobi(int32_t m, const double *T, int64_t ldt, double *theta, double *S) {
    if (m < 1 || m > 4096 || !T || ldt < m || !theta || !S) return fail(BSM_ERR_INVALID, "bad argument");
    BSM_GUARDED({
        std::vector<double> work((size_t)m * m);
        for (int c = 0; c < m; c++)
            for (int r = 0; r < m; r++) work[(size_t)r + (size_t)c * m] = T[(size_t)r + (size_t)c * ldt];
        eig_jacobi(m, work.data(), theta, S);
        return BSM_OK;
    })
}
// eig_select: the `count` of theta[0 .. m) (ascending) that `which` wants, in its order -> idx (0-based)
extern "C" int bsm_debug_eig_select(int which, int32_t m, const double *theta, int32_t count, int32_t *idx) {
    if (which < kEigLA || which > kEigLM || m < 0 || !theta || count < 0 || count > m || !idx) return fail(BSM_ERR_INVALID, "bad argument");
    eig_select(which, m, theta, count, idx);
    return BSM_OK;
}
extern "C" int bsm_debug_eig_keep(int32_t nev, int32_t ncv) { return eig_keep(nev, ncv); }
