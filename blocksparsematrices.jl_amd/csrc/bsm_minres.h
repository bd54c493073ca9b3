// bsm_minres.h -- what bsm_minres.hip (the kernels) and bsm_minres.cpp (bsm_minres_*; include/bsm_rocm.h) share: the
// device-side state of a multi-column MINRES solve and the launch interface.
// (No counterpart in the reference: its operators are LinearMaps handed to a Julia solver package.)
//
// The vectors X, R, V0, V1, W0, W1, Q (and Z0, Z1 with M) of a solver are n x K column-major in its own workspace, laid
// out and walked as bsm_cg.h describes: the leading dimension rounded up to whole 16-byte groups, the padding zero from
// the allocation on, every launch a (krylov_grid(n, es), columns) grid, one partial per workgroup and column that every
// consumer adds for itself in one fixed order.  Every scalar of the method is REAL (the forms are the real parts of
// sum conj(u) v), so a complex column is walked as 2 n reals: the kernels but mr_start do not know the element type.
#pragma once
#include <cstdint>

#include "bsm_cg.h"

namespace bsm {

// state of the columns between two iterations.  The launches of iteration j read slot j & 1; mr_decide writes the other
// one: no launch reads a scalar that the same launch replaces.
struct MrSlot {
    double gamma[kCgMaxRhs], gamma_old[kCgMaxRhs];  // sqrt<v, z> of the current and of the previous Lanczos vector
    double eta[kCgMaxRhs];
    double c[kCgMaxRhs], c_old[kCgMaxRhs], s[kCgMaxRhs], s_old[kCgMaxRhs];  // the last two rotations
    double rn[kCgMaxRhs];                                                    // ||r||
    int32_t status[kCgMaxRhs];
    int32_t done[kCgMaxRhs];  // iterations the column's x holds
};
// what mr_update derived in this iteration (its workgroup 0 writes it, mr_decide moves it into the other slot), so that
// the rotation is computed by one kernel only
struct MrStep {
    double gamma[kCgMaxRhs], eta[kCgMaxRhs], c[kCgMaxRhs], s[kCgMaxRhs];
    int32_t brk[kCgMaxRhs];  // <v_new, z_new> negative or not finite, or a1 not a positive finite number: nothing else was written
};
struct MrState {
    MrSlot slot[2];
    MrStep step;
    double tol[kCgMaxRhs];  // max(rtol ||b_c||, atol): written by the first mr_decide of a solve
    CgRecord rec;           // what the host reads, one iteration late (the record of bsm_cg.h)
};

#if defined(__HIPCC__) || defined(BSM_KRYLOV_LAUNCH)
// r = v = B - q (q null: B), padding zeroed;  vold = w0 = w1 = 0;  pbb / pnn = the shares of ||b||^2 / ||r||^2.
// B: any ldb >= n, any element alignment.  (CgDims.conj is not read by this unit.)
hipError_t launch_mr_start(const CgDims &d, const void *B, long long ldb, const void *q, void *r, void *v, void *vold, void *w0, void *w1,
                           void *pbb, void *pnn, hipStream_t stream);
// part = the shares of Re <u_c, v_c>; columns frozen in slot `par` are skipped (par < 0: none is)
hipError_t launch_mr_dot(const CgDims &d, int par, const void *u, const void *v, void *part, const MrState *st, hipStream_t stream);
// running columns of slot `par`: delta = zq / gamma^2 (zq from pzq);  vold = q / gamma - (delta / gamma) v -
// (gamma / gamma_old) vold, which is v_new;  pvz (may be null) = the shares of ||v_new||^2
hipError_t launch_mr_lanczos(const CgDims &d, int par, const void *pzq, const void *q, const void *v, void *vold, void *pvz,
                             const MrState *st, hipStream_t stream);
// running columns of slot `par`: gamma_new = sqrt(vz) (vz from pvz) and the rotation;  wold = (z / gamma - a3 wold -
// a2 w) / a1, which is w_new;  x += c_new eta w_new;  r = s_new^2 r + (c_new eta_new / gamma_new) vnew;  pnn = the shares of
// ||r||^2;  the step of the state.  A breakdown writes step.brk[c] and nothing else.
hipError_t launch_mr_update(const CgDims &d, int par, const void *pzq, const void *pvz, const void *z, void *wold, const void *w, void *x,
                            void *r, const void *vnew, void *pnn, MrState *st, hipStream_t stream);
// the decision, one wave per column.  first: tol from pbb, gamma from pvz, slot 0 written from nothing (it = 0); else slot
// `par` and the step are read and slot par ^ 1 is written.  it: the iterations x holds after this launch.
hipError_t launch_mr_decide(const CgDims &d, bool first, int par, long long it, double rtol, double atol, const void *pbb, const void *pnn,
                            const void *pvz, MrState *st, hipStream_t stream);
#endif

}  // namespace bsm
