// bsm_bicgstab.h -- what bsm_bicgstab.hip (the kernels) and bsm_bicgstab.cpp (bsm_bicgstab_*; include/bsm_rocm.h) share: the
// launch interface of a multi-column BiCGSTAB solve.
// (No counterpart in the reference: its operators are LinearMaps handed to a Julia solver package.)
//
// Layout, launch shape and partial sums are those of bsm_cg.h: the vectors X, R, Rhat, P, V, T (and Z with M) are n x K
// column-major with the leading dimension `ld` in whole 16-byte groups, padding zero and staying zero; every launch is
// (krylov_grid(n, es), columns); a reduction leaves one partial per workgroup and column, which every consumer adds in the
// same fixed order.  The device state is a CgState: CgSlot::rz holds rho = <rhat, r>, CgState::brk is not used -- there is
// no flag between the launches of an iteration: alpha, omega and every decision are RE-DERIVED by each consumer (bicg_half,
// bicg_update, bicg_dir) from the same partials and the same slot, so all of them take the same branch.
//
// The partials of one iteration (P below), all of them written before they are read by a later launch of the same
// iteration and never by the launch that reads them:
//   sig  <rhat, v>  (element)     ss  ||s||^2  (real)      ts  <t, s>  (element)     tt  ||t||^2  (real)
//   nn   ||r||^2    (real)        rho <rhat, r> (element)  bb  ||b||^2 (real; the start only)
// The decisions of an iteration on a column that runs in slot `par`, in this order (include/bsm_rocm.h):
//   rho == 0 or sigma == 0          breakdown, nothing written, the count stays           (bicg_half, _update, _dir)
//   sn not finite                   status 2 with residual sn, x holds the half step      (bicg_update, _dir)
//   sn <= tol                       status 0 with residual sn, x holds the half step      (bicg_update, _dir)
//   tt == 0 or ts == 0              breakdown with residual sn, x holds the half step     (bicg_update, _dir)
//   rn not finite / rn <= tol       status 2 / 0 with residual rn                         (bicg_dir)
#pragma once
#include "bsm_cg.h"

namespace bsm {

#if defined(__HIPCC__) || defined(BSM_KRYLOV_LAUNCH)
// the partial sums of a solver, device pointers: K * G elements or reals each
struct BicgPartials {
    void *sig, *ss, *ts, *tt, *nn, *rho, *bb;
};
// r = rhat = B - q (q null: B), padding zeroed;  bb / nn = the shares of ||b||^2 / ||r||^2 (rho = <rhat, r> IS ||r||^2 at
// the start: computed once).  B: any ldb >= n, any element alignment.  (CgDims::conj is not read: the form is conjugated.)
hipError_t launch_bicg_start(const CgDims &d, const void *B, long long ldb, const void *q, void *r, void *rhat, const BicgPartials &P,
                             hipStream_t stream);
// running columns of slot `par`: part = the shares of <u_c, v_c>, and with `nrm` those of ||u_c||^2
hipError_t launch_bicg_dot(const CgDims &d, int par, const void *u, const void *v, void *part, void *nrm, const CgState *st,
                           hipStream_t stream);
// alpha = rho / sigma;  x += alpha phat;  r -= alpha v (r holds s);  P.ss
hipError_t launch_bicg_half(const CgDims &d, int par, const BicgPartials &P, const void *phat, const void *v, void *x, void *r,
                            const CgState *st, hipStream_t stream);
// omega = ts / tt;  x += omega shat;  r -= omega t;  P.nn, P.rho.  shat null: shat is r (no preconditioner)
hipError_t launch_bicg_update(const CgDims &d, int par, const BicgPartials &P, const void *shat, const void *t, const void *rhat,
                              void *x, void *r, const CgState *st, hipStream_t stream);
// the decision and the new direction.  first: tol from P.bb, rho and rn from P.nn, p = r, slot 0 written from nothing
// (it = 0); else slot `par` is read, slot par ^ 1 written, running columns get p = r + beta (p - omega v).  it: the
// iterations x holds after this launch.
hipError_t launch_bicg_dir(const CgDims &d, bool first, int par, long long it, double rtol, double atol, const BicgPartials &P,
                           const void *r, const void *v, void *p, CgState *st, hipStream_t stream);
#endif

}  // namespace bsm
