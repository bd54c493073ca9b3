// bsm_lobpcg.cpp -- bsm_block_gram, bsm_block_combine, the bsm_lobpcg_* solver object and the test hooks bsm_debug_lobpcg_rr /
// bsm_debug_eig_jacobi_h (include/bsm_rocm.h): the host side of LOBPCG for a few extreme eigenpairs of a symmetric / Hermitian
// op(A) with an optional preconditioner.  An iteration is enqueued without a host read -- residual pass, the products with M
// and A on the whole block through bsm_mul_multi, ONE Gram matrix of the basis against [S | AS] -- and ends with one copy of
// that matrix and the residual norms and one synchronisation; the host then runs the Rayleigh-Ritz step on at most 48 basis
// columns (bsm_lobpcg.h), uploads the coefficients, and two in-place combinations move the basis on.
#include <hip/hip_runtime_api.h>

#include <cmath>
#include <complex>
#include <cstdint>
#include <cstring>
#include <limits>
#include <new>
#include <string>
#include <vector>

#define BSM_KRYLOV_LAUNCH
#include "bsm_internal.h"
#include "bsm_lockstep.h"
#include "bsm_lobpcg.h"

using namespace bsm;

namespace {

// the launches of bsm_block_* go to the device of `stream` when one is given (nothing is allocated, so this is capture-safe)
int enter_stream_device(DeviceGuard &guard, hipStream_t st) {
    int dev = -1;
    if (st && hipStreamGetDevice(st, &dev) == hipSuccess) {
        const hipError_t g = guard.enter(dev);
        if (g != hipSuccess) return hip_fail(g, "hipSetDevice");
    } else {
        (void)hipGetLastError();
    }
    return BSM_OK;
}

int64_t gram_work_bytes(int dtype, int64_t n, int64_t p, int64_t q) {
    return ((int64_t)gram_grid(dtype, n) * p * q * elem_bytes(dtype) + 15) / 16 * 16;
}

// Out = V C for any vector type: the real types run the kernel of bsm_krylov_combine
hipError_t combine_any(int dtype, int64_t n, int p, int q, const void *V, int64_t ldv, const void *Cm, int64_t ldc, void *Out, int64_t ldo,
                       hipStream_t st) {
    if (dtype == BSM_F32 || dtype == BSM_F64) return launch_eig_combine(dtype, n, p, q, V, ldv, Cm, ldc, Out, ldo, -1, st);
    return launch_block_combine_complex(dtype, n, p, q, V, ldv, Cm, ldc, Out, ldo, st);
}

}  // namespace

// ---- bsm_block_gram ---------------------------------------------------------------------------------------------------------
extern "C" int64_t bsm_block_gram_grid(int dtype, int64_t n) {
    if (!is_vec_type(dtype) || n < 0) return (int64_t)fail(BSM_ERR_INVALID, "bad argument");
    return gram_grid(dtype, n);
}

extern "C" int64_t bsm_block_gram_work(int dtype, int64_t n, int64_t p, int64_t q) {
    if (!is_vec_type(dtype) || n < 0 || p < 1 || p > kGramMaxP || q < 1 || q > kGramMaxQ) return (int64_t)fail(BSM_ERR_INVALID, "bad argument");
    return gram_work_bytes(dtype, n, p, q);
}

extern "C" int bsm_block_gram(int dtype, int64_t n, int64_t p, const void *U, int64_t ldu, int64_t q, const void *W, int64_t ldw, void *G,
                              int64_t ldg, void *work, void *stream) {
    const std::string why = vec_type_refusal("bsm_block_gram", dtype);
    if (!why.empty()) return fail(BSM_ERR_INVALID, why);
    if (n < 0 || p < 1 || p > kGramMaxP || q < 1 || q > kGramMaxQ) return fail(BSM_ERR_INVALID, "n < 0, or p outside 1 .. 48, or q outside 1 .. 96");
    if (ldu < std::max<int64_t>(n, 1) || ldw < std::max<int64_t>(n, 1) || ldg < p) return fail(BSM_ERR_INVALID, "ldu / ldw < max(n, 1), or ldg < p");
    if (!G || !work || (n > 0 && (!U || !W))) return fail(BSM_ERR_INVALID, "null argument");
    if ((uintptr_t)work % 16 != 0) return fail(BSM_ERR_INVALID, "work must be 16-byte aligned");
    const size_t es = (size_t)elem_bytes(dtype), ws = 2 * (size_t)real_bytes(dtype) == es ? 16 : 8;
    const size_t ubytes = n > 0 ? ((size_t)(p - 1) * (size_t)ldu + (size_t)n) * es : 0, wbytes = n > 0 ? ((size_t)(q - 1) * (size_t)ldw + (size_t)n) * es : 0;
    const size_t gbytes = ((size_t)(q - 1) * (size_t)ldg + (size_t)p) * ws, kbytes = (size_t)gram_work_bytes(dtype, n, p, q);
    if (overlap(G, gbytes, work, kbytes)) return fail(BSM_ERR_INVALID, "G overlaps work");
    for (const void *out : {(const void *)G, (const void *)work}) {
        const size_t ob = out == G ? gbytes : kbytes;
        if ((ubytes && overlap(U, ubytes, out, ob)) || (wbytes && overlap(W, wbytes, out, ob)))
            return fail(BSM_ERR_INVALID, "G or work overlaps U or W");
    }
    const hipStream_t st = (hipStream_t)stream;
    DeviceGuard guard;
    RC_TRY(enter_stream_device(guard, st));
    const hipError_t e = launch_block_gram(dtype, n, (int)p, U, ldu, (int)q, W, ldw, G, ldg, work, st);
    if (e != hipSuccess) return hip_fail(e, "Gram launch");
    return BSM_OK;
}

// ---- bsm_block_combine ------------------------------------------------------------------------------------------------------
extern "C" int64_t bsm_block_combine_tile(int dtype, int64_t p) {
    if (!is_vec_type(dtype) || p < 1 || p > kGramMaxP) return (int64_t)fail(BSM_ERR_INVALID, "bad argument");
    if (dtype == BSM_F32 || dtype == BSM_F64) return combine_tile_reals(p, real_bytes(dtype));
    return block_combine_tile_complex(p, elem_bytes(dtype));
}

extern "C" int bsm_block_combine(int dtype, int64_t n, int64_t p, int64_t q, const void *V, int64_t ldv, const void *Cm, int64_t ldc, void *Out,
                                 int64_t ldo, void *stream) {
    const std::string why = vec_type_refusal("bsm_block_combine", dtype);
    if (!why.empty()) return fail(BSM_ERR_INVALID, why);
    if (n < 0 || p < 1 || p > kGramMaxP) return fail(BSM_ERR_INVALID, "n < 0, or p outside 1 .. 48");
    if (q < 0 || q > p) return fail(BSM_ERR_INVALID, "q outside 0 .. p");
    if (ldv < std::max<int64_t>(n, 1) || ldo < std::max<int64_t>(n, 1) || ldc < p) return fail(BSM_ERR_INVALID, "ldv / ldo < max(n, 1), or ldc < p");
    if ((q > 0 && !Cm) || (n > 0 && (!V || !Out))) return fail(BSM_ERR_INVALID, "null argument");
    const size_t es = (size_t)elem_bytes(dtype);
    if (n > 0 && q > 0) {
        const size_t vbytes = ((size_t)(p - 1) * (size_t)ldv + (size_t)n) * es, obytes = ((size_t)(q - 1) * (size_t)ldo + (size_t)n) * es;
        if (!(Out == V && ldo == ldv) && overlap(V, vbytes, Out, obytes))
            return fail(BSM_ERR_INVALID, "Out overlaps V (only Out == V with ldo == ldv works in place)");
        if (overlap(Cm, ((size_t)(q - 1) * (size_t)ldc + (size_t)p) * es, Out, obytes))
            return fail(BSM_ERR_INVALID, "C overlaps Out (other workgroups would read it while it is written)");
    }
    const hipStream_t st = (hipStream_t)stream;
    DeviceGuard guard;
    RC_TRY(enter_stream_device(guard, st));
    const hipError_t e = combine_any(dtype, n, (int)p, (int)q, V, ldv, Cm, ldc, Out, ldo, st);
    if (e != hipSuccess) return hip_fail(e, "combine launch");
    return BSM_OK;
}

// ---- bsm_lobpcg_* -----------------------------------------------------------------------------------------------------------
struct bsm_lobpcg_s {
    bsm_matrix_s *A = nullptr, *M = nullptr;
    int opA = 0, opM = 0, vt = 0, nev = 0, k = 0, device = 0, G = 1;
    bool m_cvec = false;
    int64_t n = 0, ld = 0;
    // ONE device allocation: Z = [X | P | W | AX | AP | AW] (ld x 6 k), T (ld x k, with M), the partials of the Gram, G (3 k x
    // 6 k wide) with the k residual norms behind it, CC (3 k x 2 k), theta, the partials of the residual pass and of a norm
    void *ws = nullptr;
    int64_t ws_bytes = 0;
    char *Z = nullptr, *T = nullptr, *gpart = nullptr, *Gm = nullptr, *CC = nullptr, *theta = nullptr, *rpart = nullptr, *nrmpart = nullptr,
         *slot = nullptr;
    double *tres = nullptr;
    // pinned: G and the norms as they arrive, CC and theta as they leave, the true residuals
    char *pinned = nullptr, *h_G = nullptr, *h_CC = nullptr, *h_theta = nullptr;
    double *h_tres = nullptr;
    int64_t g_bytes = 0;  // of G alone; the norms follow
    // BSM_MEM_HOST solves: device copies of X0 (n x k) and X (n x nev), allocated at the first one
    void *hx0 = nullptr, *hx = nullptr;

    void release() {
        if (ws) (void)hipFree(ws);
        if (hx0) (void)hipFree(hx0);
        if (hx) (void)hipFree(hx);
        if (pinned) (void)hipHostFree(pinned);
        ws = hx0 = hx = nullptr;
        pinned = nullptr;
    }
    void layout(Carve &cv) {
        const int64_t es = elem_bytes(vt), rs = real_bytes(vt), p = 3 * k, wide = 8 * (es / rs);
        Z = cv.take(ld * es * 6 * k);
        T = M ? cv.take(ld * es * k) : nullptr;
        gpart = cv.take(gram_work_bytes(vt, n, p, 2 * p));
        g_bytes = p * 2 * p * wide;
        Gm = cv.take(g_bytes + k * (int64_t)sizeof(double));
        CC = cv.take(p * 2 * k * es);
        theta = cv.take(k * rs);
        rpart = cv.take((int64_t)k * G * rs);
        nrmpart = cv.take(G * rs);
        slot = cv.take(rs);
        tres = (double *)cv.take(k * (int64_t)sizeof(double));
    }
};

extern "C" int bsm_lobpcg_create(bsm_matrix_t A, int opA, bsm_matrix_t M, int opM, int vdtype, int32_t nev, int32_t block,
                                 struct bsm_lobpcg_s **out) {
    if (!out) return fail(BSM_ERR_INVALID, "out is null");
    *out = nullptr;
    if (!A) return fail(BSM_ERR_INVALID, "null handle");
    if (opA < 0 || opA > 2 || (M && (opM < 0 || opM > 2))) return fail(BSM_ERR_INVALID, "bad op");
    if (!is_vec_type(vdtype)) return fail(BSM_ERR_INVALID, "vdtype must be a vector type (BSM_F32 .. BSM_C128)");
    if (A->poly) return fail(BSM_ERR_UNSUPPORTED, "bsm_lobpcg: a composed handle (bsm_poly_create) is accepted as M, not as A");
    if (A->an.nrows != A->an.ncols) return fail(BSM_ERR_INVALID, "op(A) is not square");
    if (A->an.dtype < 0 || A->an.dtype > 5 || vec_type(A->an.dtype) != vdtype)
        return fail(BSM_ERR_INVALID, "vdtype must be the handle's own vector type (a real handle under a complex vdtype has no use here)");
    if (M && (M->an.nrows != A->an.nrows || M->an.ncols != A->an.ncols)) return fail(BSM_ERR_INVALID, "M has another order than A");
    const int pm = M ? pairing(M, vdtype) : 0;
    if (pm < 0) return fail(BSM_ERR_INVALID, "M's vector type must be vdtype, or real and unmixed of the same precision under a complex vdtype");
    if (A->dist || (M && M->dist)) return fail(BSM_ERR_UNSUPPORTED, "multi-device handles are not supported by bsm_lobpcg");
    if (!A->on_device || (M && !M->on_device)) return fail(BSM_ERR_DEVICE, "handle has no device image (created with BSM_DEVICE_NONE)");
    for (const bsm_matrix_s *H : {(const bsm_matrix_s *)A, (const bsm_matrix_s *)M})
        if (H && (H->img.own_lo > 0 || H->img.own_hi < H->img.nrows))
            return fail(BSM_ERR_UNSUPPORTED, "handles that own a row range only (bsm_options.own_lo / own_hi) are not supported by bsm_lobpcg");
    if (M && M->img.device != A->img.device) return fail(BSM_ERR_INVALID, "A and M live on different devices");
    const int64_t n = A->an.nrows;
    if (nev < 1 || block < nev || block > BSM_CG_MAX_RHS || 3 * (int64_t)block > n)
        return fail(BSM_ERR_INVALID, "nev < 1, or block outside nev .. BSM_CG_MAX_RHS, or 3 block > n");
    bsm_lobpcg_s *S = new (std::nothrow) bsm_lobpcg_s;
    if (!S) return fail(BSM_ERR_ALLOC, "out of host memory");
    const int64_t es = elem_bytes(vdtype), rs = real_bytes(vdtype);
    S->A = A, S->M = M, S->opA = opA, S->opM = opM, S->vt = vdtype, S->nev = nev, S->k = block, S->device = A->img.device, S->n = n;
    S->m_cvec = pm == 1;
    S->ld = (std::max<int64_t>(n, 1) * es + 15) / 16 * 16 / es;
    S->G = krylov_grid(n, (int)es);
    Carve size;
    S->layout(size);
    S->ws_bytes = size.off;
    const int64_t p = 3 * block;
    const int64_t pin_g = S->g_bytes + block * 8, pin_cc = p * 2 * block * es, pin_th = (block * rs + 15) / 16 * 16;
    DeviceGuard guard;
    hipError_t e = guard.enter(S->device);
    if (e == hipSuccess) e = hipMalloc(&S->ws, (size_t)size.off);
    if (e == hipSuccess) e = hipMemset(S->ws, 0, (size_t)size.off);
    if (e == hipSuccess) e = hipHostMalloc((void **)&S->pinned, (size_t)(pin_g + pin_cc + pin_th + block * 8), hipHostMallocDefault);
    if (e != hipSuccess) {
        S->release();
        delete S;
        return e == hipErrorOutOfMemory ? fail(BSM_ERR_ALLOC, "out of device memory for the LOBPCG workspace") : hip_fail(e, "LOBPCG workspace");
    }
    Carve cv{(char *)S->ws};
    S->layout(cv);
    S->h_G = S->pinned;
    S->h_CC = S->h_G + pin_g;
    S->h_theta = S->h_CC + pin_cc;
    S->h_tres = (double *)(S->h_theta + pin_th);
    *out = S;
    return BSM_OK;
}

extern "C" int bsm_lobpcg_destroy(struct bsm_lobpcg_s *S) {
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

template <typename T> void put_elem(int vt, const T &v, char *dst);
template <> void put_elem<double>(int vt, const double &v, char *dst) {
    if (real_bytes(vt) == 4) *(float *)dst = (float)v;
    else *(double *)dst = v;
}
template <> void put_elem<std::complex<double>>(int vt, const std::complex<double> &v, char *dst) {
    if (real_bytes(vt) == 4) ((float *)dst)[0] = (float)v.real(), ((float *)dst)[1] = (float)v.imag();
    else ((double *)dst)[0] = v.real(), ((double *)dst)[1] = v.imag();
}

// The Rayleigh-Ritz step on the G that has arrived in h_G: -> the status of lob_rr; with 0, h_CC = [C | C_P] and h_theta are
// filled in the type of the vectors, theta[0 .. k) and anorm updated, drops added.
template <typename T>
int rr_step(bsm_lobpcg_s *E, int which, const unsigned char *use, double *theta, double &anorm, int &drops) {
    const int k = E->k, p = 3 * k, vt = E->vt;
    const size_t es = (size_t)elem_bytes(vt);
    const T *G = (const T *)E->h_G;
    const double eps = real_bytes(vt) == 4 ? (double)std::numeric_limits<float>::epsilon() : std::numeric_limits<double>::epsilon();
    std::vector<T> Cm((size_t)p * k);
    int dr = 0;
    double big = 0;
    const int status = lob_rr<T>(p, k, which, G, p, G + (size_t)p * p, p, use, 64.0 * p * eps, theta, Cm.data(), &dr, &big);
    drops += dr;
    if (status != 0) return status;
    anorm = std::max(anorm, big);
    for (int c = 0; c < k; c++)
        for (int i = 0; i < p; i++) {
            const T v = Cm[(size_t)i + (size_t)c * p];
            put_elem<T>(vt, v, E->h_CC + ((size_t)i + (size_t)c * p) * es);
            put_elem<T>(vt, i < k ? T(0) : v, E->h_CC + ((size_t)i + (size_t)(k + c) * p) * es);
        }
    for (int c = 0; c < k; c++) put_elem<double>(vt, theta[c], E->h_theta + (size_t)c * real_bytes(vt));
    return 0;
}

// the solve on device operands (arguments checked)
int solve_device(bsm_lobpcg_s *E, const void *X0, int64_t ldx0, void *X, int64_t ldx, const bsm_lobpcg_params &prm, bsm_lobpcg_info &info,
                 bsm_eigsh_pair *pairs, double *history, int64_t hist_cap, hipStream_t st) {
    const int vt = E->vt, k = E->k, p = 3 * k, nev = E->nev, G = E->G;
    const int64_t n = E->n, ld = E->ld, es = elem_bytes(vt), rs = real_bytes(vt);
    const bool cplx = es != rs;
    char *const S = E->Z, *const AS = E->Z + ld * es * p;
    auto scol = [&](int j) { return S + (int64_t)j * ld * es; };
    auto ascol = [&](int j) { return AS + (int64_t)j * ld * es; };
    double *const d_res = (double *)(E->Gm + E->g_bytes);
    const double *const h_res = (const double *)(E->h_G + E->g_bytes);
    const double nan = std::numeric_limits<double>::quiet_NaN();
    for (int i = 0; i < nev; i++) pairs[i].value = pairs[i].estimate = pairs[i].residual = nan;
    std::vector<unsigned char> use((size_t)p, 0), live((size_t)k, 0), wlive((size_t)k, 0);  // wlive: the columns whose W the last step used
    std::vector<double> theta((size_t)k, 0.0);
    double anorm = 0;
    int drops = 0;
    auto gram_and_wait = [&]() -> int {
        HIP_TRY(launch_block_gram(vt, n, p, S, ld, 2 * p, E->Z, ld, E->Gm, p, E->gpart, st));
        HIP_TRY(hipMemcpyAsync(E->h_G, E->Gm, (size_t)E->g_bytes + (size_t)k * sizeof(double), hipMemcpyDeviceToHost, st));
        HIP_TRY(hipStreamSynchronize(st));
        return BSM_OK;
    };
    auto rayleigh_ritz = [&]() {
        return cplx ? rr_step<std::complex<double>>(E, prm.which, use.data(), theta.data(), anorm, drops)
                    : rr_step<double>(E, prm.which, use.data(), theta.data(), anorm, drops);
    };
    auto move_on = [&]() -> int {  // [X | P] = S CC and [AX | AP] = AS CC, in place
        HIP_TRY(hipMemcpyAsync(E->CC, E->h_CC, (size_t)p * 2 * k * es, hipMemcpyHostToDevice, st));
        HIP_TRY(hipMemcpyAsync(E->theta, E->h_theta, (size_t)k * rs, hipMemcpyHostToDevice, st));
        HIP_TRY(combine_any(vt, n, p, 2 * k, S, ld, E->CC, p, S, ld, st));
        HIP_TRY(combine_any(vt, n, p, 2 * k, AS, ld, E->CC, p, AS, ld, st));
        return BSM_OK;
    };
    auto first_not_live = [&](const double *nrm) {
        const double tol = std::max(prm.rtol * anorm, prm.atol);
        bool all = true;
        for (int c = 0; c < k; c++) {
            live[c] = nrm[c] > tol;
            if (c < nev) all = all && !live[c];
        }
        return all;
    };
    auto record = [&](int64_t row, const double *nrm) {
        if (history && row < hist_cap)
            for (int c = 0; c < nev; c++) history[row * nev + c] = nrm[c];
    };
    // ---- the start: X = X0, AX = op(A) X, the Rayleigh-Ritz step on X alone
    HIP_TRY(hipMemsetAsync(E->Z, 0, (size_t)(ld * es * 6 * k), st));
    HIP_TRY(hipMemsetAsync(d_res, 0, (size_t)k * sizeof(double), st));
    const CgDims dk{vt, n, ld, G, k, true};
    HIP_TRY(launch_cg_copy(dk, true, const_cast<void *>(X0), ldx0, S, st));
    RC_TRY(apply(E->A, E->opA, false, k, ld, ld, vt, S, AS, st));
    info.a_products = 1;
    RC_TRY(gram_and_wait());
    for (int c = 0; c < k; c++) use[c] = 1;
    int status = rayleigh_ritz();
    bool have_p = false, pending = false;
    int64_t it = 0;
    std::vector<double> last((size_t)k, nan);
    if (status == 0) {
        status = -1;
        RC_TRY(move_on());
        for (;;) {
            char *const dest = E->M ? E->T : scol(2 * k);
            HIP_TRY(launch_lob_resid(vt, n, k, ascol(0), ld, scol(0), ld, E->theta, dest, ld, E->rpart, d_res, st));
            if (pending || it >= prm.maxiter) {
                // the carried norms of the X an update has just left: they confirm convergence, or end the solve at maxiter
                HIP_TRY(hipMemcpyAsync(E->h_G + E->g_bytes, d_res, (size_t)k * sizeof(double), hipMemcpyDeviceToHost, st));
                HIP_TRY(hipStreamSynchronize(st));
                bool finite = true;
                for (int c = 0; c < k; c++) finite = finite && std::isfinite(h_res[c]);
                if (!finite) {
                    status = 2;
                    break;
                }
                const bool conv = first_not_live(h_res);
                if (conv || it >= prm.maxiter) {
                    record(it, h_res);
                    std::copy(h_res, h_res + k, last.begin());
                    status = conv ? 0 : 1;
                    break;
                }
                pending = false;
            }
            if (E->M) {
                RC_TRY(apply(E->M, E->opM, E->m_cvec, k, ld, ld, vt, E->T, scol(2 * k), st));
                info.m_products++;
            }
            RC_TRY(apply(E->A, E->opA, false, k, ld, ld, vt, scol(2 * k), ascol(2 * k), st));
            info.a_products++;
            RC_TRY(gram_and_wait());
            bool finite = true;
            for (int c = 0; c < k; c++) finite = finite && std::isfinite(h_res[c]);
            if (!finite) {
                status = 2;
                break;
            }
            record(it, h_res);
            pending = first_not_live(h_res);
            for (int c = 0; c < k; c++) {
                use[k + c] = have_p && wlive[c];
                use[2 * k + c] = live[c];
            }
            const int rr = rayleigh_ritz();
            if (rr != 0) {
                status = rr;
                break;
            }
            RC_TRY(move_on());
            wlive = live;
            have_p = true;
            it++;
        }
    }
    info.status = status;
    info.iterations = (int32_t)it;
    info.drops = drops;
    info.anorm = anorm;
    if (status > 1) return BSM_OK;
    // ---- the end: X[:, :nev] of norm one into the caller's matrix, then the TRUE residuals
    const double tol = std::max(prm.rtol * anorm, prm.atol);
    for (int c = 0; c < nev; c++) {
        pairs[c].value = theta[c];
        pairs[c].estimate = pairs[c].residual = last[c];
        info.nconv += last[c] <= tol;
    }
    const CgDims dn{vt, n, ld, G, nev, true};
    HIP_TRY(launch_cg_copy(dn, false, X, ldx, S, st));
    for (int c = 0; c < nev; c++) {
        char *xc = (char *)X + (int64_t)c * ldx * es;
        HIP_TRY(launch_krylov_update(vt, n, 0, S, ld, xc, E->rpart, nullptr, E->nrmpart, st));
        HIP_TRY(launch_krylov_norm(vt, G, E->nrmpart, E->slot, st));
        HIP_TRY(launch_eig_scale(vt, n, xc, E->slot, st));
    }
    RC_TRY(apply(E->A, E->opA, false, nev, ldx, ld, vt, X, ascol(2 * k), st));
    info.a_products++;
    HIP_TRY(launch_eig_resid(vt, n, nev, ascol(2 * k), ld, X, ldx, E->theta, E->rpart, E->tres, st));
    HIP_TRY(hipMemcpyAsync(E->h_tres, E->tres, sizeof(double) * (size_t)nev, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    for (int c = 0; c < nev; c++) pairs[c].residual = E->h_tres[c];
    return BSM_OK;
}

}  // namespace

extern "C" int bsm_lobpcg_solve(struct bsm_lobpcg_s *S, const void *X0, int64_t ldx0, void *X, int64_t ldx, const bsm_lobpcg_params *p,
                                bsm_lobpcg_info *info, bsm_eigsh_pair *pairs, double *history, int64_t history_capacity, int memspace,
                                void *stream) {
    if (!S || !p || !info || !pairs || !X0 || !X) return fail(BSM_ERR_INVALID, "null argument");
    if (p->struct_size != (int32_t)sizeof(bsm_lobpcg_params)) return fail(BSM_ERR_INVALID, "bsm_lobpcg_params.struct_size mismatch");
    if (memspace != BSM_MEM_HOST && memspace != BSM_MEM_DEVICE) return fail(BSM_ERR_INVALID, "bad memspace");
    if (p->which != kEigLA && p->which != kEigSA) return fail(BSM_ERR_INVALID, "which must be BSM_EIGSH_LA or BSM_EIGSH_SA");
    if (!(p->rtol >= 0) || !(p->atol >= 0) || p->maxiter < 1) return fail(BSM_ERR_INVALID, "rtol and atol must be >= 0, maxiter >= 1");
    if (history_capacity < 0 || (history_capacity > 0 && !history)) return fail(BSM_ERR_INVALID, "history_capacity < 0, or no history array");
    const int64_t n = S->n;
    const size_t es = (size_t)elem_bytes(S->vt);
    if (ldx < std::max<int64_t>(n, 1) || ldx0 < std::max<int64_t>(n, 1)) return fail(BSM_ERR_INVALID, "ldx / ldx0 < max(n, 1)");
    if (overlap(X0, ((size_t)(S->k - 1) * (size_t)ldx0 + (size_t)n) * es, X, ((size_t)(S->nev - 1) * (size_t)ldx + (size_t)n) * es))
        return fail(BSM_ERR_INVALID, "X must not overlap X0");
    const hipStream_t st = (hipStream_t)stream;
    if (capturing(st)) return fail(BSM_ERR_INVALID, "bsm_lobpcg_solve must not be graph-captured");
    std::memset(info, 0, sizeof(*info));
    info->workspace_bytes = S->ws_bytes;
    DeviceGuard guard;
    hipError_t e = guard.enter(S->device);
    if (e != hipSuccess) return hip_fail(e, "hipSetDevice");
    BSM_GUARDED({
        if (memspace == BSM_MEM_DEVICE) return solve_device(S, X0, ldx0, X, ldx, *p, *info, pairs, history, history_capacity, st);
        // host operands: staged through dense buffers the solver keeps
        const size_t colb = (size_t)n * es;
        if (!S->hx0) e = hipMalloc(&S->hx0, colb * (size_t)S->k + 16);
        if (e == hipSuccess && !S->hx) e = hipMalloc(&S->hx, colb * (size_t)S->nev + 16);
        if (e != hipSuccess) {
            if (e != hipErrorOutOfMemory) return hip_fail(e, "staging buffers");
            (void)hipGetLastError();
            return fail(BSM_ERR_ALLOC, "out of device memory for the staging buffers");
        }
        for (int c = 0; c < S->k && e == hipSuccess; c++)
            e = hipMemcpyAsync((char *)S->hx0 + c * colb, (const char *)X0 + (size_t)c * (size_t)ldx0 * es, colb, hipMemcpyHostToDevice, st);
        if (e != hipSuccess) return hip_fail(e, "host-staged solve");
        const int rc = solve_device(S, S->hx0, n, S->hx, n, *p, *info, pairs, history, history_capacity, st);
        if (rc != BSM_OK) return rc;
        if (info->status <= 1) {
            for (int c = 0; c < S->nev && e == hipSuccess; c++)
                e = hipMemcpyAsync((char *)X + (size_t)c * (size_t)ldx * es, (char *)S->hx + c * colb, colb, hipMemcpyDeviceToHost, st);
            if (e == hipSuccess) e = hipStreamSynchronize(st);
            if (e != hipSuccess) return hip_fail(e, "host-staged solve");
        }
        return BSM_OK;
    })
}

// ---- test hooks (unexported in the header, like bsm_debug_eig_jacobi); none needs a device ----------------------------------
// eig_jacobi_h of bsm_lobpcg.h on the Hermitian A (m x m, column-major, lda >= m; not written; cplx: interleaved (re, im) doubles):
// theta ascending, Q (m x m, leading dimension m) the eigenvectors.  Returns the sweeps taken through *sweeps (may be null).
extern "C" int bsm_debug_eig_jacobi_h(int32_t cplx, int32_t m, const double *A, int64_t lda, double *theta, double *Q, int32_t *sweeps) {
    if (m < 1 || m > 4096 || !A || lda < m || !theta || !Q) return fail(BSM_ERR_INVALID, "bad argument");
    BSM_GUARDED({
        int sw = 0;
        if (cplx) {
            using Z = std::complex<double>;
            std::vector<Z> work((size_t)m * m);
            for (int c = 0; c < m; c++)
                for (int r = 0; r < m; r++) work[(size_t)r + (size_t)c * m] = ((const Z *)A)[(size_t)r + (size_t)c * lda];
            sw = eig_jacobi_h<Z>(m, work.data(), theta, (Z *)Q);
        } else {
            std::vector<double> work((size_t)m * m);
            for (int c = 0; c < m; c++)
                for (int r = 0; r < m; r++) work[(size_t)r + (size_t)c * m] = A[(size_t)r + (size_t)c * lda];
            sw = eig_jacobi_h<double>(m, work.data(), theta, Q);
        }
        if (sweeps) *sweeps = sw;
        return BSM_OK;
    })
}
// lob_rr of bsm_lobpcg.h, the host step of one iteration: GB, GA p x p (leading dimension p; cplx: interleaved doubles), use: p
// flags, tau -> *status (0, 2, 3), theta (k), C (p x k, leading dimension p), *drops
extern "C" int bsm_debug_lobpcg_rr(int32_t cplx, int32_t p, int32_t k, int32_t which, const double *GB, const double *GA, const uint8_t *use,
                                   double tau, int32_t *status, double *theta, double *C, int32_t *drops) {
    if (p < 1 || p > 4096 || k < 1 || k > p || (which != kEigLA && which != kEigSA) || !GB || !GA || !use || !status || !theta || !C || !drops)
        return fail(BSM_ERR_INVALID, "bad argument");
    BSM_GUARDED({
        int dr = 0;
        double big = 0;
        if (cplx) {
            using Z = std::complex<double>;
            *status = lob_rr<Z>(p, k, which, (const Z *)GB, p, (const Z *)GA, p, use, tau, theta, (Z *)C, &dr, &big);
        } else {
            *status = lob_rr<double>(p, k, which, GB, p, GA, p, use, tau, theta, C, &dr, &big);
        }
        *drops = dr;
        return BSM_OK;
    })
}
