// bsm_lsqr.h -- what bsm_lsqr.hip (the kernels) and bsm_lsqr.cpp (bsm_lsqr_*, bsm_debug_lsqr_step; include/bsm_rocm.h) share:
// the arithmetic of one LSQR step of one column in plain C++, compiled for the host (the test hook) and for the kernels
// alike, the device-side state of a multi-column LSQR solve and the launch interface.
// (No counterpart in the reference: its operators are LinearMaps handed to a Julia solver package.)
//
// The vectors of a solve have TWO lengths.  U and Q (the product op(A) V) have the m = rows(op(A)) rows of B; X, V, W and P
// (the product op(A)^H U) the n = cols(op(A)) rows of X.  Each is laid out and walked as bsm_cg.h describes -- the leading
// dimension rounded up to whole 16-byte groups, the padding zero from the allocation on, one partial per workgroup and
// column that every consumer adds for itself in one fixed order --, the m-row vectors on a (krylov_grid(m, es), columns)
// grid and the n-row ones on a (krylov_grid(n, es), columns) grid.  A kernel of one grid that needs a norm the other grid
// left (ls_v and ls_update: ||u||^2) adds the OTHER grid's partials.  Every scalar of the method is REAL, so a complex
// column is walked as reals: the kernels but ls_start do not know the element type.
#pragma once
#include <cmath>
#include <cstdint>

#include "bsm_cg.h"

namespace bsm {

// the scalars one column carries from one iteration to the next (include/bsm_rocm.h states the method)
template <typename R> struct LsqrScalars {
    R alpha, beta;      // ||v~||, ||u~||: the norms of the unnormalised Lanczos vectors
    R phibar, rhobar;
    R res2;             // sum of psi^2: what damp leaves in the residual
    R anorm;            // running Frobenius norm of the bidiagonal factor
};
// what one step derives from them and from the two new norms
template <typename R> struct LsqrStep {
    LsqrScalars<R> next;
    R cx, cw;           // x += cx w;  w = v~ / alpha' - cw w
    R rnorm, arnorm;
    int32_t status;     // kCgRun, 0 or 2
};

BSM_HD float ls_sqrt(float a) { return ::sqrtf(a); }
BSM_HD double ls_sqrt(double a) { return ::sqrt(a); }
#if defined(__HIP_DEVICE_COMPILE__)
BSM_HD bool ls_finite(float a) { return isfinite(a); }
BSM_HD bool ls_finite(double a) { return isfinite(a); }
#else
BSM_HD bool ls_finite(float a) { return std::isfinite(a); }
BSM_HD bool ls_finite(double a) { return std::isfinite(a); }
#endif

// The decision of a column from its two estimates and its two newest norms, in the order the header states: not finite
// -> 2;  rnorm <= tol -> 0;  arnorm <= ntol anorm rnorm -> 0;  alpha == 0 or beta == 0 (the Krylov space ended: the iterate
// IS the solution) -> 0;  else the column runs on.
template <typename R> BSM_HD int32_t lsqr_decide(R rnorm, R arnorm, R anorm, R alpha, R beta, double tol, double ntol) {
    if (!ls_finite(rnorm) || !ls_finite(arnorm)) return 2;
    if ((double)rnorm <= tol) return 0;
    if ((double)arnorm <= ntol * (double)anorm * (double)rnorm) return 0;
    if (alpha == R(0) || beta == R(0)) return 0;
    return kCgRun;
}

// One step of one column: the two plane rotations (the first removes damp, the second the subdiagonal beta'), the
// coefficients of the x and w updates, the estimates and the decision.  betan = ||u~_new||, alphan = ||v~_new|| (0 when
// betan == 0).  No division by zero and no root of a negative number is executed.
template <typename R> BSM_HD void lsqr_step(const LsqrScalars<R> &in, R betan, R alphan, R damp, double tol, double ntol, LsqrStep<R> &out) {
    const R anorm = ls_sqrt(((in.anorm * in.anorm + in.alpha * in.alpha) + betan * betan) + damp * damp);
    const R rhobar1 = ls_sqrt(in.rhobar * in.rhobar + damp * damp);
    const bool z1 = rhobar1 == R(0);
    const R cs1 = z1 ? R(1) : in.rhobar / rhobar1, sn1 = z1 ? R(0) : damp / rhobar1;
    const R psi = sn1 * in.phibar, phibar1 = cs1 * in.phibar;
    const R rho = ls_sqrt(rhobar1 * rhobar1 + betan * betan);
    const bool z = rho == R(0);
    const R c = z ? R(1) : rhobar1 / rho, s = z ? R(0) : betan / rho;
    const R theta = s * alphan, phi = c * phibar1, tau = s * phi;
    out.next.alpha = alphan, out.next.beta = betan;
    out.next.rhobar = -c * alphan;
    out.next.phibar = s * phibar1;
    out.next.res2 = in.res2 + psi * psi;
    out.next.anorm = anorm;
    out.cx = z ? R(0) : phi / rho;
    out.cw = z ? R(0) : theta / rho;
    out.rnorm = ls_sqrt(out.next.phibar * out.next.phibar + out.next.res2);
    out.arnorm = alphan * (tau < R(0) ? -tau : tau);
    out.status = lsqr_decide(out.rnorm, out.arnorm, anorm, alphan, betan, tol, ntol);
}

// state of the columns between two iterations.  The launches of iteration j read slot j & 1; ls_decide writes the other
// one: no launch reads a scalar that the same launch replaces.
struct LsSlot {
    double alpha[kCgMaxRhs], beta[kCgMaxRhs], phibar[kCgMaxRhs], rhobar[kCgMaxRhs], res2[kCgMaxRhs], anorm[kCgMaxRhs];
    double rnorm[kCgMaxRhs], arnorm[kCgMaxRhs];
    int32_t status[kCgMaxRhs];
    int32_t done[kCgMaxRhs];  // iterations the column's x holds
};
// what ls_update derived in this iteration (its workgroup 0 writes it, ls_decide moves it into the other slot), so that
// the rotation is computed by one kernel only
struct LsStepState {
    double alpha[kCgMaxRhs], beta[kCgMaxRhs], phibar[kCgMaxRhs], rhobar[kCgMaxRhs], res2[kCgMaxRhs], anorm[kCgMaxRhs];
    double rnorm[kCgMaxRhs], arnorm[kCgMaxRhs];
    int32_t status[kCgMaxRhs];
};
struct LsState {
    LsSlot slot[2];
    LsStepState step;
    double tol[kCgMaxRhs];  // max(rtol ||b_c||, atol): written by the first ls_decide of a solve
    CgRecord rec;           // what the host reads, one iteration late (the record of bsm_cg.h; rn = rnorm)
};

#if defined(__HIPCC__) || defined(BSM_KRYLOV_LAUNCH)
// m-grid.  u = B - q (q null: B), padding zeroed;  pbb / pu = the shares of ||b||^2 / ||u||^2.  B: any ldb >= m, any
// element alignment.  (CgDims.conj is not read by this unit.)
hipError_t launch_ls_start(const CgDims &dm, const void *B, long long ldb, const void *q, void *u, void *pbb, void *pu, hipStream_t stream);
// n-grid, once per solve.  beta = sqrt(sum of pu), Gm shares;  v = p / beta (beta not a positive finite number: v = p, the first
// decision freezes the column);  pv = the shares of ||v||^2
hipError_t launch_ls_begin(const CgDims &dn, int Gm, const void *pu, const void *p, void *v, void *pv, hipStream_t stream);
// m-grid, running columns of slot `par`: u = q / alpha - (alpha / beta) u;  pu = the shares of ||u||^2
hipError_t launch_ls_u(const CgDims &dm, int par, const void *q, void *u, void *pu, const LsState *st, hipStream_t stream);
// n-grid, running columns of slot `par`: beta' = sqrt(sum of pu), Gm shares;  first (iteration 0): w = v / alpha;
// v = p / beta' - (beta' / alpha) v  (beta' == 0: v = 0);  pv = the shares of ||v||^2
hipError_t launch_ls_v(const CgDims &dn, bool first, int par, int Gm, const void *pu, const void *p, void *v, void *w, void *pv,
                       const LsState *st, hipStream_t stream);
// n-grid, running columns of slot `par`: alpha' from pv, beta' from pu (Gm shares), lsqr_step by every workgroup for itself;
// x += cx w;  w = v / alpha' - cw w  (alpha' == 0: w = -cw w, it is not needed again);  workgroup 0 leaves the step
hipError_t launch_ls_update(const CgDims &dn, int par, int Gm, double damp, double ntol, const void *pu, const void *pv, const void *v,
                            void *w, void *x, LsState *st, hipStream_t stream);
// the decision, one wave per column.  first: tol from pbb, beta from pu (Gm shares each), alpha from pv (Gn shares), slot 0
// written from nothing (it = 0); else slot `par` and the step are read and slot par ^ 1 is written.  it: the iterations x
// holds after this launch.
hipError_t launch_ls_decide(const CgDims &dn, bool first, int par, long long it, int Gm, double rtol, double atol, double ntol,
                            const void *pbb, const void *pu, const void *pv, LsState *st, hipStream_t stream);
#endif

}  // namespace bsm
