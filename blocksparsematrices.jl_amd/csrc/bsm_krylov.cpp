// bsm_krylov.cpp -- bsm_krylov_orth, the test hook bsm_debug_krylov_lsq_host and the bsm_gmres_* solver object (include/bsm_rocm.h): the host
// side of restarted GMRES.  The products go through the public bsm_mul / bsm_mul_cvec, the vector work through the
// kernels of bsm_krylov.hip; the host only enqueues, and reads one double per iteration from a pinned slot, one
// iteration late (the look-ahead).
#include <hip/hip_runtime_api.h>

#include <algorithm>
#include <cmath>
#include <cstring>
#include <new>
#include <string>
#include <vector>

#define BSM_KRYLOV_LAUNCH
#include "bsm_internal.h"
#include "bsm_krylov.h"

using namespace bsm;

namespace {

// bytes of the partials of one pass: k columns of G elements, then G reals (the norm shares), each part 16-byte aligned
int64_t orth_work_bytes(int dtype, int64_t n, int64_t k) {
    const int64_t G = krylov_grid(n, elem_bytes(dtype));
    return (k * G * elem_bytes(dtype) + 15) / 16 * 16 + (G * real_bytes(dtype) + 15) / 16 * 16;
}

// one element holding the real value v
struct Scalar {
    double d[2] = {0, 0};
    float f[2] = {0, 0};
    int dtype;
    Scalar(int dt, double v) : dtype(dt) {
        d[0] = v;
        f[0] = (float)v;
    }
    const void *ptr() const { return real_bytes(dtype) == 4 ? (const void *)f : (const void *)d; }
};

}  // namespace

extern "C" int64_t bsm_krylov_orth_work(int dtype, int64_t n, int64_t k) {
    if (!is_vec_type(dtype) || n < 0 || k < 0 || k > BSM_GMRES_MAX_RESTART) return (int64_t)fail(BSM_ERR_INVALID, "bad argument");
    return orth_work_bytes(dtype, n, k);
}

extern "C" int bsm_krylov_orth(int dtype, int64_t n, int64_t k, const void *V, int64_t ldv, void *w, void *hsum, void *nrm,
                               void *work, void *stream) {
    const std::string why = vec_type_refusal("bsm_krylov_orth", dtype);
    if (!why.empty()) return fail(BSM_ERR_INVALID, why);
    if (n < 0 || k < 0 || k > BSM_GMRES_MAX_RESTART) return fail(BSM_ERR_INVALID, "n < 0, or k outside 0 .. BSM_GMRES_MAX_RESTART");
    if (k > 0 && ldv < std::max<int64_t>(n, 1)) return fail(BSM_ERR_INVALID, "ldv < max(n, 1)");
    if (!nrm || !work || (n > 0 && !w) || (k > 0 && !hsum) || (k > 0 && n > 0 && !V)) return fail(BSM_ERR_INVALID, "null argument");
    if ((uintptr_t)work % 16 != 0) return fail(BSM_ERR_INVALID, "work must be 16-byte aligned");
    const hipStream_t st = (hipStream_t)stream;
    // the launches go to the device of `stream` when one is given (nothing is allocated, so this is capture-safe)
    DeviceGuard guard;
    int dev = -1;
    if (st && hipStreamGetDevice(st, &dev) == hipSuccess) {
        const hipError_t g = guard.enter(dev);
        if (g != hipSuccess) return hip_fail(g, "hipSetDevice");
    } else {
        (void)hipGetLastError();
    }
    const int es = elem_bytes(dtype), G = krylov_grid(n, es);
    void *nrmpart = (char *)work + (k * G * es + 15) / 16 * 16;
    hipError_t e = launch_krylov_dot(dtype, n, (int)k, V, ldv, w, work, st);
    if (e == hipSuccess) e = krylov_orth_update(dtype, n, (int)k, V, ldv, w, work, hsum, nrmpart, st);
    if (e == hipSuccess) e = launch_krylov_norm(dtype, G, nrmpart, nrm, st);
    if (e != hipSuccess) return hip_fail(e, "orthogonalisation launch");
    return BSM_OK;
}

// test hook (unexported in the header, like bsm_debug_move_image_array): min || beta e_1 - H y ||_2 for a (k + 1) x k upper
// Hessenberg H (column-major, ldh >= k + 1, element type dtype) whose subdiagonal is real and >= 0, by krylov_lsq_host --
// the rotations and the back substitution the one-wave kernels run.  H is overwritten by the triangular factor; y: k
// elements; res (may be NULL): k doubles, the residual norm after every column.  Needs no device.
extern "C" int bsm_debug_krylov_lsq_host(int dtype, int32_t k, void *H, int64_t ldh, double beta, void *y, double *res) {
    if (!is_vec_type(dtype)) return fail(BSM_ERR_INVALID, "bad dtype");
    if (k < 1 || k > BSM_GMRES_MAX_RESTART || ldh < (int64_t)k + 1 || !H || !y) return fail(BSM_ERR_INVALID, "bad argument");
    try {
        std::vector<double> r((size_t)k);
        std::vector<double> work((size_t)(3 * k + 1) * 2);
        with_types(dtype, [&](auto t, auto, auto nc) {
            using R = decltype(t);
            krylov_lsq_host<R, decltype(nc)::value>(k, (R *)H, ldh, (R)beta, (R *)y, r.data(), (R *)work.data());
        });
        if (res) std::copy(r.begin(), r.end(), res);
    } catch (const std::bad_alloc &) {
        return fail(BSM_ERR_ALLOC, "out of host memory");
    }
    return BSM_OK;
}

// ---- the solver object ---------------------------------------------------------------------------------------------------
struct bsm_gmres_s {
    bsm_matrix_s *A = nullptr, *M = nullptr;
    int opA = 0, opM = 0, vt = 0, m = 0, device = 0;
    bool a_cvec = false, m_cvec = false;  // a real handle under complex vectors: bsm_mul_cvec
    int64_t n = 0;
    // ONE device allocation (info.workspace): V (n x (m + 2), ldv = n rounded up to whole 16-byte groups), w, z, the small
    // arrays, the partials of a pass
    void *ws = nullptr;
    int64_t ws_bytes = 0, ldv = 0;
    char *V = nullptr, *w = nullptr, *z = nullptr, *part = nullptr;
    KrylovSmall sm{};
    double *slots = nullptr;  // pinned: m + 1 doubles (KrylovSmall::res mirrored)
    std::vector<hipEvent_t> ev;  // m + 1
    // BSM_MEM_HOST solves: device copies of b and x, allocated at the first one
    void *hb = nullptr, *hx = nullptr;

    char *col(int64_t j) const { return V + j * ldv * elem_bytes(vt); }
    void release() {
        if (ws) (void)hipFree(ws);
        if (hb) (void)hipFree(hb);
        if (hx) (void)hipFree(hx);
        if (slots) (void)hipHostFree(slots);
        for (hipEvent_t e : ev)
            if (e) (void)hipEventDestroy(e);
        ws = hb = hx = nullptr;
        slots = nullptr;
        ev.clear();
    }
};

namespace {

// how `H` is applied to vectors of type vt: 0 bsm_mul, 1 bsm_mul_cvec, -1 not at all
int pairing(const bsm_matrix_s *H, int vt) {
    const int dt = H->an.dtype;
    if (dt < 0 || dt > 5) return -1;
    if (vec_type(dt) == vt) return 0;
    if ((dt == BSM_F32 && vt == BSM_C64) || (dt == BSM_F64 && vt == BSM_C128)) return 1;
    return -1;
}

// y = alpha * op(H) x + beta * y on the device
int apply(bsm_matrix_s *H, int op, bool cvec, const void *x, void *y, const Scalar &alpha, const Scalar *beta, hipStream_t st) {
    auto fn = cvec ? bsm_mul_cvec : bsm_mul;
    return fn(H, op, x, y, alpha.ptr(), beta ? beta->ptr() : nullptr, beta ? 0 : 1, BSM_MEM_DEVICE, (void *)st);
}

bool overlap(const void *a, const void *b, size_t bytes) {
    const uintptr_t p = (uintptr_t)a, q = (uintptr_t)b;
    return p < q + bytes && q < p + bytes;
}

}  // namespace

extern "C" int bsm_gmres_create(bsm_matrix_t A, int opA, bsm_matrix_t M, int opM, int vdtype, int32_t restart, bsm_gmres_t *out) {
    if (!out) return fail(BSM_ERR_INVALID, "out is null");
    *out = nullptr;
    if (!A) return fail(BSM_ERR_INVALID, "null handle");
    if (opA < 0 || opA > 2 || (M && (opM < 0 || opM > 2))) return fail(BSM_ERR_INVALID, "bad op");
    if (!is_vec_type(vdtype)) return fail(BSM_ERR_INVALID, "vdtype must be a vector type (BSM_F32 .. BSM_C128)");
    if (restart < 1 || restart > BSM_GMRES_MAX_RESTART) return fail(BSM_ERR_INVALID, "restart outside 1 .. BSM_GMRES_MAX_RESTART");
    if (A->an.nrows != A->an.ncols) return fail(BSM_ERR_INVALID, "op(A) is not square");
    if (M && (M->an.nrows != A->an.nrows || M->an.ncols != A->an.ncols)) return fail(BSM_ERR_INVALID, "M has another order than A");
    const int pa = pairing(A, vdtype), pm = M ? pairing(M, vdtype) : 0;
    if (pa < 0 || pm < 0)
        return fail(BSM_ERR_INVALID, "a handle's vector type must be vdtype, or real and unmixed of the same precision under a complex vdtype");
    if (A->dist || (M && M->dist)) return fail(BSM_ERR_UNSUPPORTED, "multi-device handles are not supported by bsm_gmres");
    if (!A->on_device || (M && !M->on_device)) return fail(BSM_ERR_DEVICE, "handle has no device image (created with BSM_DEVICE_NONE)");
    if (M && M->img.device != A->img.device) return fail(BSM_ERR_INVALID, "A and M live on different devices");
    bsm_gmres_s *S = new (std::nothrow) bsm_gmres_s;
    if (!S) return fail(BSM_ERR_ALLOC, "out of host memory");
    S->A = A, S->M = M, S->opA = opA, S->opM = opM, S->vt = vdtype, S->m = restart, S->device = A->img.device;
    S->a_cvec = pa == 1, S->m_cvec = pm == 1;
    S->n = A->an.nrows;
    const int64_t es = elem_bytes(vdtype), rs = real_bytes(vdtype), m = restart, n = S->n;
    S->ldv = (std::max<int64_t>(n, 1) * es + 15) / 16 * 16 / es;
    auto pad = [](int64_t b) { return (b + 63) / 64 * 64; };
    const int64_t vec = pad(S->ldv * es);
    // offsets of the pieces
    int64_t off = 0;
    auto take = [&](int64_t bytes) {
        const int64_t o = off;
        off += pad(bytes);
        return o;
    };
    const int64_t oV = take(S->ldv * es * (m + 2)), ow = take(vec), oz = take(vec), opart = take(orth_work_bytes(vdtype, n, m));
    const int64_t oH = take((m + 1) * m * es), ocs = take(m * rs), osn = take(m * es), og = take((m + 1) * es), oy = take(m * es);
    const int64_t ohs = take(m * es), oinv = take(rs), ores = take((m + 1) * 8), onp = take(kKrylovMaxGrid * rs);
    S->ws_bytes = off;
    DeviceGuard guard;
    hipError_t e = guard.enter(S->device);
    if (e == hipSuccess) e = hipMalloc(&S->ws, (size_t)off);
    if (e == hipSuccess) e = hipMemset(S->ws, 0, (size_t)off);
    if (e == hipSuccess) e = hipHostMalloc((void **)&S->slots, (size_t)(m + 1) * 8, hipHostMallocDefault);
    S->ev.assign((size_t)m + 1, nullptr);
    for (size_t i = 0; i < S->ev.size() && e == hipSuccess; i++) e = hipEventCreateWithFlags(&S->ev[i], hipEventDisableTiming);
    if (e != hipSuccess) {
        S->release();
        delete S;
        return e == hipErrorOutOfMemory ? fail(BSM_ERR_ALLOC, "out of device memory for the GMRES workspace") : hip_fail(e, "GMRES workspace");
    }
    char *b = (char *)S->ws;
    S->V = b + oV, S->w = b + ow, S->z = b + oz, S->part = b + opart;
    S->sm.Hm = b + oH, S->sm.cs = b + ocs, S->sm.sn = b + osn, S->sm.g = b + og, S->sm.y = b + oy, S->sm.hsum = b + ohs;
    S->sm.inv = b + oinv, S->sm.res = (double *)(b + ores), S->sm.nrmpart = b + onp;
    *out = S;
    return BSM_OK;
}

extern "C" int bsm_gmres_destroy(bsm_gmres_t S) {
    if (!S) return BSM_OK;
    DeviceGuard guard;
    (void)guard.enter(S->device);
    S->release();
    delete S;
    return BSM_OK;
}

namespace {

// the solve on device vectors b, x (arguments checked)
int solve_device(bsm_gmres_s *S, const void *b, void *x, const bsm_gmres_params &p, bsm_gmres_info &info, double *history,
                 hipStream_t st) {
    const int vt = S->vt, m = S->m, es = elem_bytes(vt);
    const int64_t n = S->n;
    const int G = krylov_grid(n, es);
    const KrylovSmall &sm = S->sm;
    const Scalar one(vt, 1.0), minus(vt, -1.0);
    char *const r = S->col(m + 1);  // the residual lives in the spare column
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
    // the norm that start_kernel left in res[m], on the host
    auto read_start = [&](double &v) -> hipError_t {
        hipError_t q = hipMemcpyAsync(S->slots + m, sm.res + m, 8, hipMemcpyDeviceToHost, st);
        if (q == hipSuccess) q = hipStreamSynchronize(st);
        v = S->slots[m];
        return q;
    };
    // || b ||: r = b on the way (the first cycle of a solve from zero starts there)
    HIP_TRY(krylov_copy_norm(vt, n, b, r, sm.nrmpart, st));
    HIP_TRY(launch_krylov_start(vt, G, m, sm, st));
    double bnorm = 0;
    HIP_TRY(read_start(bnorm));
    info.bnorm = bnorm;
    if (!p.use_x0) HIP_TRY(hipMemsetAsync(x, 0, (size_t)n * es, st));
    if (!std::isfinite(bnorm)) {
        info.status = 2;
        info.residual = bnorm;
        HIP_TRY(hipStreamSynchronize(st));
        return BSM_OK;
    }
    const double tol = std::max(p.rtol * bnorm, p.atol);
    bool first = true;
    double beta = bnorm;
    for (;;) {
        // ---- the true residual and the first basis vector
        if (!(first && !p.use_x0)) {
            HIP_TRY(krylov_copy_norm(vt, n, b, r, nullptr, st));
            RC_TRY(apply(S->A, S->opA, S->a_cvec, x, r, minus, &one, st));
            info.a_products++;
            HIP_TRY(krylov_copy_norm(vt, n, r, r, sm.nrmpart, st));
            HIP_TRY(launch_krylov_start(vt, G, m, sm, st));
            HIP_TRY(read_start(beta));
        }
        first = false;
        info.residual = beta;
        if (!std::isfinite(beta)) {
            info.status = 2;
            break;
        }
        if (beta <= tol) {  // (b = 0, or x0 solves the system, or the last cycle got there)
            info.status = 0;
            break;
        }
        if (info.iterations >= p.maxiter) {
            info.status = 1;
            break;
        }
        info.cycles++;
        HIP_TRY(krylov_scale_store(vt, n, r, S->col(0), sm.inv, st));
        // ---- the iterations of this cycle, checked one behind the enqueue
        const int jmax = (int)std::min<int64_t>(m, p.maxiter - info.iterations);
        int k = 0;          // iterations the answer uses
        int status = 1;     // of this cycle: 1 = ran to its end
        int enq = 0, chk = 0;
        auto check = [&](int j) -> hipError_t {  // estimate of iteration j -> k / status; true when the cycle ends there
            const hipError_t q = hipEventSynchronize(S->ev[(size_t)j]);
            if (q != hipSuccess) return q;
            const double est = S->slots[j];
            if (history && info.iterations + j < p.history_capacity) history[info.iterations + j] = est;
            info.residual = est;
            k = j + 1;
            if (!std::isfinite(est))
                status = 2;
            else if (est <= tol)
                status = 0;
            return hipSuccess;
        };
        while (chk < jmax && status == 1) {
            if (enq < jmax) {
                const int j = enq;
                const char *vj = S->col(j);
                if (S->M) {
                    RC_TRY(apply(S->M, S->opM, S->m_cvec, vj, S->z, one, nullptr, st));
                    RC_TRY(apply(S->A, S->opA, S->a_cvec, S->z, S->w, one, nullptr, st));
                } else {
                    RC_TRY(apply(S->A, S->opA, S->a_cvec, vj, S->w, one, nullptr, st));
                }
                for (int pass = 0; pass < 2; pass++) {
                    HIP_TRY(launch_krylov_dot(vt, n, j + 1, S->V, S->ldv, S->w, S->part, st));
                    HIP_TRY(krylov_orth_update(vt, n, j + 1, S->V, S->ldv, S->w, S->part, sm.hsum, sm.nrmpart, st));
                }
                HIP_TRY(launch_krylov_hess(vt, G, m, j, sm, st));
                HIP_TRY(krylov_scale_store(vt, n, S->w, S->col(j + 1), sm.inv, st));
                HIP_TRY(hipMemcpyAsync(S->slots + j, sm.res + j, 8, hipMemcpyDeviceToHost, st));
                HIP_TRY(hipEventRecord(S->ev[(size_t)j], st));
                enq++;
                if (enq < jmax && enq - chk < 2) continue;  // one iteration ahead of the check
            }
            HIP_TRY(check(chk));
            chk++;
        }
        // (iterations enqueued beyond k ran on workspace the answer does not read: column k + 1 .. of V and of the
        // Hessenberg factor, g[k + 1 ..]; their products are not counted)
        info.iterations += k;
        info.a_products += k;
        if (S->M) info.m_products += k;
        if (status == 2) {
            info.status = 2;
            break;
        }
        // ---- x += M V[:, 0:k] y
        HIP_TRY(launch_krylov_trsolve(vt, m, k, sm, st));
        HIP_TRY(krylov_combine(vt, n, k, S->V, S->ldv, sm.y, S->w, st));
        if (S->M) {
            RC_TRY(apply(S->M, S->opM, S->m_cvec, S->w, x, one, &one, st));
            info.m_products++;
        } else {
            HIP_TRY(launch_vec_add(vt, x, S->w, n, st));
        }
        if (status == 0) {
            info.status = 0;
            break;
        }
        // maxiter reached at the end of this cycle: report it without another residual product
        if (info.iterations >= p.maxiter) {
            info.status = 1;
            break;
        }
    }
    HIP_TRY(hipStreamSynchronize(st));
#undef HIP_TRY
#undef RC_TRY
    return BSM_OK;
}

}  // namespace

extern "C" int bsm_gmres_solve(bsm_gmres_t S, const void *b, void *x, const bsm_gmres_params *p, bsm_gmres_info *info,
                               double *history, int memspace, void *stream) {
    if (!S || !p || !info) return fail(BSM_ERR_INVALID, "null argument");
    if (p->struct_size != (int32_t)sizeof(bsm_gmres_params)) return fail(BSM_ERR_INVALID, "bsm_gmres_params.struct_size mismatch");
    if (memspace != BSM_MEM_HOST && memspace != BSM_MEM_DEVICE) return fail(BSM_ERR_INVALID, "bad memspace");
    if (!(p->rtol >= 0) || !(p->atol >= 0) || p->maxiter < 0 || p->history_capacity < 0)
        return fail(BSM_ERR_INVALID, "rtol, atol, maxiter and history_capacity must be >= 0");
    const size_t bytes = (size_t)S->n * elem_bytes(S->vt);
    if (S->n > 0 && (!b || !x)) return fail(BSM_ERR_INVALID, "null vector");
    if (S->n > 0 && overlap(b, x, bytes)) return fail(BSM_ERR_INVALID, "x must not alias b");
    const hipStream_t st = (hipStream_t)stream;
    if (capturing(st)) return fail(BSM_ERR_INVALID, "bsm_gmres_solve must not be graph-captured");
    std::memset(info, 0, sizeof(*info));
    info->workspace_bytes = S->ws_bytes;
    info->workspace = (uint64_t)(uintptr_t)S->ws;
    if (S->n == 0) return BSM_OK;  // nothing to solve: status 0, no iteration, b and x (which may be null) untouched
    DeviceGuard guard;
    hipError_t e = guard.enter(S->device);
    if (e != hipSuccess) return hip_fail(e, "hipSetDevice");
    if (memspace == BSM_MEM_DEVICE) return solve_device(S, b, x, *p, *info, history, st);
    // host vectors: staged like bsm_mul's, through buffers the solver keeps
    if (!S->hb) {
        e = hipMalloc(&S->hb, bytes + 16);
        if (e == hipSuccess) e = hipMalloc(&S->hx, bytes + 16);
        if (e != hipSuccess) return hip_fail(e, "staging buffers");
    }
    e = hipMemcpyAsync(S->hb, b, bytes, hipMemcpyHostToDevice, st);
    if (e == hipSuccess && p->use_x0) e = hipMemcpyAsync(S->hx, x, bytes, hipMemcpyHostToDevice, st);
    if (e != hipSuccess) return hip_fail(e, "host-staged solve");
    const int rc = solve_device(S, S->hb, S->hx, *p, *info, history, st);
    if (rc != BSM_OK) return rc;
    e = hipMemcpyAsync(x, S->hx, bytes, hipMemcpyDeviceToHost, st);
    if (e == hipSuccess) e = hipStreamSynchronize(st);
    if (e != hipSuccess) return hip_fail(e, "host-staged solve");
    return BSM_OK;
}
