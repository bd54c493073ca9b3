// bsm_krylov.cpp -- bsm_krylov_orth and the test hook bsm_debug_krylov_lsq_host (include/bsm_rocm.h): one Gram-Schmidt pass
// for a caller's Krylov method through the kernels of bsm_krylov.hip, and the host form of the small dense step of restarted
// GMRES (bsm_krylov.h).  The GMRES solvers themselves are bsm_gmres_multi.cpp.
#include <hip/hip_runtime_api.h>

#include <algorithm>
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
    if (e == hipSuccess) e = launch_krylov_update(dtype, n, (int)k, V, ldv, w, work, hsum, nrmpart, st);
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
