// bsm_poly.h -- what bsm_poly.hip (the kernels), bsm_poly.cpp (bsm_poly_create / bsm_poly_info and the product of a composed
// handle; include/bsm_rocm.h) and the units that own a handle's life (bsm_capi.cpp, bsm_dist.cpp) share: the state a
// polynomial preconditioner keeps beside the fields of bsm_matrix_s, and the launch interface.
// (No counterpart in the reference: its operators are LinearMaps handed to a Julia solver package.)
//
// The handle is z = p(A) x by the s-step recurrence of include/bsm_rocm.h over an operator handle A and an optional inner
// preconditioner handle D (absent: the identity), with REAL coefficients a[0 .. s), b[0 .. s):
//     r_0 = x,  d_0 = b_0 D r_0;   r_{k+1} = r_k - A d_k,  d_{k+1} = a_{k+1} d_k + b_{k+1} D r_{k+1};   p(A) x = d_0 + .. + d_{s-1}
// The vectors R, d, acc, Q (and T = D R with D) are n x nrhs_max column-major in ONE allocation with the layout of bsm_cg.h:
// the leading dimension rounded up to whole 16-byte groups, the padding zero from create on.  Only the caller's X and Y are
// touched element by element under a guard.
#pragma once
#include <hip/hip_runtime_api.h>

#include <cstdint>

#include "../../include/bsm_rocm.h"
#include "bsm_cg.h"

struct bsm_matrix_s;

namespace bsm {

struct PolyState {
    bsm_matrix_s *A = nullptr, *D = nullptr;  // held, not owned: they outlive the composed handle
    int opA = 0, opD = 0, vt = 0, kmax = 0, steps = 0;
    bool a_cvec = false, d_cvec = false;  // a real handle under a complex vdtype goes through bsm_mul_multi_cvec
    double a[BSM_POLY_MAX_STEPS] = {}, b[BSM_POLY_MAX_STEPS] = {};
    int64_t n = 0, ld = 0;
    int G = 1;
    void *ws = nullptr;  // the one allocation: R, d, acc, Q (, T), each ld x kmax
    int64_t ws_bytes = 0;
    char *R = nullptr, *d = nullptr, *acc = nullptr, *Q = nullptr, *T = nullptr;
};

#if defined(__HIPCC__) || defined(BSM_KRYLOV_LAUNCH)
// R = X (any ldx, any element alignment) with the padding zeroed;  d (may be null) = b0 R
hipError_t launch_poly_load(const CgDims &dm, const void *X, long long ldx, void *R, void *d, double b0, hipStream_t stream);
// without D, one pass:  acc += d (first: acc = d);  R -= Q;  d = a d + b R
hipError_t launch_poly_step(const CgDims &dm, bool first, double a, double b, void *acc, void *R, const void *Q, void *d, hipStream_t stream);
// with D, in front of T = D R:  acc += d (first: acc = d);  R -= Q
hipError_t launch_poly_resid(const CgDims &dm, bool first, void *acc, const void *d, void *R, const void *Q, hipStream_t stream);
// with D, behind T = D R:  d = a d + b T  (first: d = b T, d is not read)
hipError_t launch_poly_dir(const CgDims &dm, bool first, double a, double b, const void *T, void *d, hipStream_t stream);
// Y = alpha (acc + d) + beta Y on n rows of nrhs columns of the caller's Y (any ldy, any element alignment) and nothing else;
// acc null: p(A) x = d (one step);  strong_zero: Y is overwritten without being read.  alpha, beta: (re, im)
hipError_t launch_poly_store(const CgDims &dm, const double *alpha, const double *beta, bool strong_zero, const void *acc, const void *d,
                             void *Y, long long ldy, hipStream_t stream);
#endif

}  // namespace bsm
