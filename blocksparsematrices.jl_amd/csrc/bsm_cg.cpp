// bsm_cg.cpp -- the bsm_cg_* solver object (include/bsm_rocm.h): the host side of preconditioned CG / COCG on up to
// BSM_CG_MAX_RHS right-hand sides in lockstep.  The products go through the public bsm_mul_multi / bsm_mul_multi_cvec, the
// vector work through the kernels of bsm_cg.hip.  Every decision of the method is taken on the device; the host only
// enqueues, and reads one record per iteration from a pinned slot, one iteration late (the look-ahead), to know when to
// stop enqueuing.
#include <hip/hip_runtime_api.h>

#include <algorithm>
#include <cmath>
#include <cstdint>
#include <cstring>
#include <new>

#define BSM_KRYLOV_LAUNCH
#include "bsm_internal.h"
#include "bsm_cg.h"

using namespace bsm;

namespace {
constexpr int kRing = 4;  // pinned record slots and events: at most two records are in flight
}

struct bsm_cg_s {
    bsm_matrix_s *A = nullptr, *M = nullptr;
    int opA = 0, opM = 0, vt = 0, kmax = 0, device = 0;
    bool a_cvec = false, m_cvec = false, conj = true;
    int64_t n = 0, ld = 0;
    int G = 1;
    // ONE device allocation (info.workspace): X, R, P, Q (and Z with M) as ld x kmax, the partials, the state
    void *ws = nullptr;
    int64_t ws_bytes = 0;
    char *X = nullptr, *R = nullptr, *P = nullptr, *Q = nullptr, *Z = nullptr;
    char *ppq = nullptr, *prz = nullptr, *pnn = nullptr, *pbb = nullptr;
    CgState *state = nullptr;
    CgRecord *slots = nullptr;  // pinned, kRing of them
    hipEvent_t ev[kRing] = {};
    // BSM_MEM_HOST solves: device copies of B and X (n x kmax), allocated at the first one
    void *hb = nullptr, *hx = nullptr;

    void release() {
        if (ws) (void)hipFree(ws);
        if (hb) (void)hipFree(hb);
        if (hx) (void)hipFree(hx);
        if (slots) (void)hipHostFree(slots);
        for (hipEvent_t &e : ev) {
            if (e) (void)hipEventDestroy(e);
            e = nullptr;
        }
        ws = hb = hx = nullptr;
        slots = nullptr;
    }
};

namespace {

// how `H` is applied to vectors of type vt: 0 bsm_mul_multi, 1 bsm_mul_multi_cvec, -1 not at all (as bsm_gmres_create)
int pairing(const bsm_matrix_s *H, int vt) {
    const int dt = H->an.dtype;
    if (dt < 0 || dt > 5) return -1;
    if (vec_type(dt) == vt) return 0;
    if ((dt == BSM_F32 && vt == BSM_C64) || (dt == BSM_F64 && vt == BSM_C128)) return 1;
    return -1;
}

// Y = op(H) X on nrhs columns of the workspace (leading dimension ld), Y overwritten
int apply(bsm_matrix_s *H, int op, bool cvec, int nrhs, int64_t ld, int vt, const void *X, void *Y, hipStream_t st) {
    const double one_d[2] = {1, 0}, zero_d[2] = {0, 0};
    const float one_f[2] = {1, 0}, zero_f[2] = {0, 0};
    const bool f = real_bytes(vt) == 4;
    auto fn = cvec ? bsm_mul_multi_cvec : bsm_mul_multi;
    return fn(H, op, nrhs, X, ld, Y, ld, f ? (const void *)one_f : (const void *)one_d, f ? (const void *)zero_f : (const void *)zero_d, 1,
              BSM_MEM_DEVICE, (void *)st);
}

bool overlap(const void *a, size_t abytes, const void *b, size_t bbytes) {
    const uintptr_t p = (uintptr_t)a, q = (uintptr_t)b;
    return p < q + bbytes && q < p + abytes;
}

}  // namespace

extern "C" int bsm_cg_create(bsm_matrix_t A, int opA, bsm_matrix_t M, int opM, int vdtype, int32_t nrhs_max, int32_t method,
                             struct bsm_cg_s **out) {
    if (!out) return fail(BSM_ERR_INVALID, "out is null");
    *out = nullptr;
    if (!A) return fail(BSM_ERR_INVALID, "null handle");
    if (opA < 0 || opA > 2 || (M && (opM < 0 || opM > 2))) return fail(BSM_ERR_INVALID, "bad op");
    if (!is_vec_type(vdtype)) return fail(BSM_ERR_INVALID, "vdtype must be a vector type (BSM_F32 .. BSM_C128)");
    if (method != BSM_CG_METHOD_CG && method != BSM_CG_METHOD_COCG) return fail(BSM_ERR_INVALID, "method must be BSM_CG_METHOD_CG or BSM_CG_METHOD_COCG");
    if (nrhs_max < 1 || nrhs_max > BSM_CG_MAX_RHS) return fail(BSM_ERR_INVALID, "nrhs_max outside 1 .. BSM_CG_MAX_RHS");
    if (A->an.nrows != A->an.ncols) return fail(BSM_ERR_INVALID, "op(A) is not square");
    if (M && (M->an.nrows != A->an.nrows || M->an.ncols != A->an.ncols)) return fail(BSM_ERR_INVALID, "M has another order than A");
    const int pa = pairing(A, vdtype), pm = M ? pairing(M, vdtype) : 0;
    if (pa < 0 || pm < 0)
        return fail(BSM_ERR_INVALID, "a handle's vector type must be vdtype, or real and unmixed of the same precision under a complex vdtype");
    if (A->dist || (M && M->dist)) return fail(BSM_ERR_UNSUPPORTED, "multi-device handles are not supported by bsm_cg");
    if (!A->on_device || (M && !M->on_device)) return fail(BSM_ERR_DEVICE, "handle has no device image (created with BSM_DEVICE_NONE)");
    if (M && M->img.device != A->img.device) return fail(BSM_ERR_INVALID, "A and M live on different devices");
    bsm_cg_s *S = new (std::nothrow) bsm_cg_s;
    if (!S) return fail(BSM_ERR_ALLOC, "out of host memory");
    S->A = A, S->M = M, S->opA = opA, S->opM = opM, S->vt = vdtype, S->kmax = nrhs_max, S->device = A->img.device;
    S->a_cvec = pa == 1, S->m_cvec = pm == 1, S->conj = method == BSM_CG_METHOD_CG;
    S->n = A->an.nrows;
    const int64_t es = elem_bytes(vdtype), rs = real_bytes(vdtype), K = nrhs_max;
    S->ld = (std::max<int64_t>(S->n, 1) * es + 15) / 16 * 16 / es;
    S->G = krylov_grid(S->n, (int)es);
    int64_t off = 0;
    auto take = [&](int64_t bytes) {
        const int64_t o = off;
        off += (bytes + 63) / 64 * 64;
        return o;
    };
    const int64_t vec = S->ld * es * K;
    const int64_t oX = take(vec), oR = take(vec), oP = take(vec), oQ = take(vec), oZ = M ? take(vec) : 0;
    const int64_t opq = take(K * S->G * es), orz = take(K * S->G * es), onn = take(K * S->G * rs), obb = take(K * S->G * rs);
    const int64_t ost = take((int64_t)sizeof(CgState));
    S->ws_bytes = off;
    DeviceGuard guard;
    hipError_t e = guard.enter(S->device);
    if (e == hipSuccess) e = hipMalloc(&S->ws, (size_t)off);
    if (e == hipSuccess) e = hipMemset(S->ws, 0, (size_t)off);  // the padding of the vectors is zero from here on (bsm_cg.h)
    if (e == hipSuccess) e = hipHostMalloc((void **)&S->slots, sizeof(CgRecord) * kRing, hipHostMallocDefault);
    for (int i = 0; i < kRing && e == hipSuccess; i++) e = hipEventCreateWithFlags(&S->ev[i], hipEventDisableTiming);
    if (e != hipSuccess) {
        S->release();
        delete S;
        return e == hipErrorOutOfMemory ? fail(BSM_ERR_ALLOC, "out of device memory for the CG workspace") : hip_fail(e, "CG workspace");
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
    DeviceGuard guard;
    (void)guard.enter(S->device);
    S->release();
    delete S;
    return BSM_OK;
}

namespace {

// the solve on device matrices B, X (arguments checked)
int solve_device(bsm_cg_s *S, int nrhs, const void *B, int64_t ldb, void *X, int64_t ldx, const bsm_cg_params &p, bsm_cg_info &info,
                 bsm_cg_column *cols, double *history, hipStream_t st) {
    const int vt = S->vt, es = elem_bytes(vt);
    const CgDims d{vt, S->n, S->ld, S->G, nrhs, S->conj};
    const int64_t maxiter = std::min<int64_t>(p.maxiter, INT32_MAX);
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
    // record k (0: the start, j + 1: iteration j) -> its pinned slot, behind its event
    auto post = [&](int64_t k) -> hipError_t {
        hipError_t q = hipMemcpyAsync(S->slots + k % kRing, &S->state->rec, sizeof(CgRecord), hipMemcpyDeviceToHost, st);
        if (q == hipSuccess) q = hipEventRecord(S->ev[k % kRing], st);
        return q;
    };
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
    HIP_TRY(post(0));
    // ---- the iterations, their records read one behind the enqueue
    int64_t enq = 0, rd = 0;
    const CgRecord *last = nullptr;
    for (;;) {
        if (enq < maxiter) {
            const int par = (int)(enq & 1);
            RC_TRY(apply(S->A, S->opA, S->a_cvec, nrhs, S->ld, vt, S->P, S->Q, st));
            HIP_TRY(launch_cg_dot(d, par, S->P, S->Q, S->ppq, S->state, st));
            HIP_TRY(launch_cg_update(d, par, S->ppq, S->P, S->Q, S->X, S->R, S->pnn, prz_fused, S->state, st));
            RC_TRY(precondition(par));
            HIP_TRY(launch_cg_dir(d, false, par, enq + 1, p.rtol, p.atol, S->pbb, S->pnn, S->prz, Zv, S->P, S->state, st));
            enq++;
            HIP_TRY(post(enq));
        }
        HIP_TRY(hipEventSynchronize(S->ev[rd % kRing]));
        last = S->slots + rd % kRing;
        int running = 0;
        for (int c = 0; c < nrhs; c++) {
            running += last->status[c] == kCgRun;
            if (history && rd >= 1 && rd - 1 < p.history_capacity) history[(rd - 1) * nrhs + c] = last->rn[c];
        }
        if (running == 0 || rd == maxiter) break;
        rd++;
    }
    // (an iteration enqueued beyond record rd found every column frozen: it wrote nothing)
    CgRecord fin = *last;
    HIP_TRY(launch_cg_copy(d, false, X, ldx, S->X, st));
    HIP_TRY(hipStreamSynchronize(st));
    for (int c = 0; c < nrhs; c++) {
        const int status = fin.status[c] == kCgRun ? 1 : fin.status[c];
        const int64_t its = fin.done[c];
        info.status = std::max(info.status, status);
        info.iterations = std::max(info.iterations, its);
        info.columns_converged += status == 0;
        if (cols) {
            cols[c].status = status;
            cols[c].reserved = 0;
            cols[c].iterations = its;
            cols[c].residual = fin.rn[c];
            cols[c].bnorm = fin.bnorm[c];
        }
    }
    info.a_products = info.iterations + (p.use_x0 ? 1 : 0);
    info.m_products = S->M ? info.iterations + 1 : 0;
#undef HIP_TRY
#undef RC_TRY
    return BSM_OK;
}

}  // namespace

extern "C" int bsm_cg_solve(struct bsm_cg_s *S, int32_t nrhs, const void *B, int64_t ldb, void *X, int64_t ldx, const bsm_cg_params *p,
                            bsm_cg_info *info, bsm_cg_column *cols, double *history, int memspace, void *stream) {
    if (!S || !p || !info) return fail(BSM_ERR_INVALID, "null argument");
    if (p->struct_size != (int32_t)sizeof(bsm_cg_params)) return fail(BSM_ERR_INVALID, "bsm_cg_params.struct_size mismatch");
    if (memspace != BSM_MEM_HOST && memspace != BSM_MEM_DEVICE) return fail(BSM_ERR_INVALID, "bad memspace");
    if (!(p->rtol >= 0) || !(p->atol >= 0) || p->maxiter < 0 || p->history_capacity < 0)
        return fail(BSM_ERR_INVALID, "rtol, atol, maxiter and history_capacity must be >= 0");
    if (nrhs < 1 || nrhs > S->kmax) return fail(BSM_ERR_INVALID, "nrhs outside 1 .. nrhs_max");
    const int64_t n = S->n, lmin = std::max<int64_t>(n, 1);
    if (ldb < lmin || ldx < lmin) return fail(BSM_ERR_INVALID, "ldb / ldx < max(n, 1)");
    const size_t es = (size_t)elem_bytes(S->vt);
    const size_t bbytes = ((size_t)(nrhs - 1) * (size_t)ldb + (size_t)n) * es, xbytes = ((size_t)(nrhs - 1) * (size_t)ldx + (size_t)n) * es;
    if (n > 0 && (!B || !X)) return fail(BSM_ERR_INVALID, "null matrix");
    if (n > 0 && overlap(B, bbytes, X, xbytes)) return fail(BSM_ERR_INVALID, "X must not overlap B");
    const hipStream_t st = (hipStream_t)stream;
    if (capturing(st)) return fail(BSM_ERR_INVALID, "bsm_cg_solve must not be graph-captured");
    std::memset(info, 0, sizeof(*info));
    info->workspace_bytes = S->ws_bytes;
    info->workspace = (uint64_t)(uintptr_t)S->ws;
    if (n == 0) {  // nothing to solve: status 0, no iteration, B and X (which may be null) untouched
        info->columns_converged = nrhs;
        if (cols) std::memset(cols, 0, sizeof(*cols) * (size_t)nrhs);
        return BSM_OK;
    }
    DeviceGuard guard;
    hipError_t e = guard.enter(S->device);
    if (e != hipSuccess) return hip_fail(e, "hipSetDevice");
    if (memspace == BSM_MEM_DEVICE) return solve_device(S, nrhs, B, ldb, X, ldx, *p, *info, cols, history, st);
    // host matrices: staged column by column through dense buffers the solver keeps
    const size_t col = (size_t)n * es;
    if (!S->hb || !S->hx) {
        if (!S->hb) e = hipMalloc(&S->hb, col * (size_t)S->kmax + 16);
        if (e == hipSuccess && !S->hx) e = hipMalloc(&S->hx, col * (size_t)S->kmax + 16);
        if (e != hipSuccess) {  // (a buffer that was obtained is kept; the next host solve asks for the other again)
            if (e != hipErrorOutOfMemory) return hip_fail(e, "staging buffers");
            (void)hipGetLastError();
            return fail(BSM_ERR_ALLOC, "out of device memory for the staging buffers");
        }
    }
    for (int c = 0; c < nrhs && e == hipSuccess; c++) {
        e = hipMemcpyAsync((char *)S->hb + c * col, (const char *)B + (size_t)c * (size_t)ldb * es, col, hipMemcpyHostToDevice, st);
        if (e == hipSuccess && p->use_x0)
            e = hipMemcpyAsync((char *)S->hx + c * col, (const char *)X + (size_t)c * (size_t)ldx * es, col, hipMemcpyHostToDevice, st);
    }
    if (e != hipSuccess) return hip_fail(e, "host-staged solve");
    const int rc = solve_device(S, nrhs, S->hb, n, S->hx, n, *p, *info, cols, history, st);
    if (rc != BSM_OK) return rc;
    for (int c = 0; c < nrhs && e == hipSuccess; c++)
        e = hipMemcpyAsync((char *)X + (size_t)c * (size_t)ldx * es, (char *)S->hx + c * col, col, hipMemcpyDeviceToHost, st);
    if (e == hipSuccess) e = hipStreamSynchronize(st);
    if (e != hipSuccess) return hip_fail(e, "host-staged solve");
    return BSM_OK;
}
