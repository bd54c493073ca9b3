// bsm_gmres_multi.h -- what bsm_gmres_multi.hip (the kernels) and bsm_gmres_multi.cpp (bsm_gmres_multi_*, bsm_gmres_*;
// include/bsm_rocm.h) share: the device-side state of a multi-column restarted GMRES solve and the launch interface.
// (No counterpart in the reference: its operators are LinearMaps handed to a Julia solver package.)
//
// The vectors are those of bsm_cg.h: ld x K column-major in the solver's workspace, ld rounded up to whole 16-byte groups,
// the padding zero and staying zero, every launch (krylov_grid(n, es), columns).  Basis vector i of ALL columns is one
// ld x kmax matrix V_i, so op(A) V_j is a plain multi-column product; the basis of column c is V_0[:, c], V_1[:, c], .. at
// a stride of vs = kmax * ld elements.  Inside a cycle every column has its own small arrays (GmSmall) and its own partials: part[(c * m + i) * G + wg] for basis vector i, nrm[c * G + wg].
#pragma once
#include <cstdint>

#include "bsm_cg.h"

namespace bsm {

// State of the columns between two launches.  The launches that decide (gm_begin, gm_hess) read slot `par` and write slot
// par ^ 1; the vector launches between them read the slot written last: no launch reads a scalar that the same launch
// replaces.
struct GmSlot {
    double rn[kCgMaxRhs];      // the last estimate, or the true residual norm of the last start
    int32_t status[kCgMaxRhs]; // kCgRun, or the bsm_cg_column.status the column froze with (0, 2)
    int32_t done[kCgMaxRhs];   // iterations the column's answer uses
    int32_t kc[kCgMaxRhs];     // of them, those of the open cycle
    int32_t owed[kCgMaxRhs];   // the open cycle's update x += M V y is still to come (set by gm_hess, dropped by gm_begin)
};
struct GmState {
    GmSlot slot[2];
    double tol[kCgMaxRhs];    // max(rtol ||b_c||, atol): written by the first gm_begin of a solve
    double bnorm[kCgMaxRhs];
    CgRecord rec;             // what the host reads, one step late: written by gm_begin and gm_hess
};

#if defined(__HIPCC__) || defined(BSM_KRYLOV_LAUNCH)
// the small arrays of the cycles, each once per column: column c at c * (the size given) from the pointer
struct GmSmall {
    void *Hm;    // m * (m + 1) elements: the rotated Hessenberg matrix
    void *cs;    // m reals
    void *sn;    // m elements
    void *g;     // m + 1 elements
    void *y;     // m elements
    void *hsum;  // m elements: the column the two passes accumulate; zero between iterations
    void *inv;   // 1 real: 1 / ||w|| of the last gm_hess (0 for a zero norm)
    void *part;  // m * G elements: the partials of a pass; the first G reals double as the shares of ||b||^2 at the start
    void *nrm;   // G reals: the shares of ||w||^2 (of ||r||^2 at a start)
};
struct GmDims {
    CgDims d;      // conj unused
    int m, kmax;   // restart; columns of the workspace matrices
};
// r = B - q (q null: r = B) -> V_0 unnormalised, padding zeroed; the shares of ||r||^2, on the first start of a solve
// those of ||b||^2 too.  first: every column runs; else columns frozen in slot `par` are skipped.
hipError_t launch_gm_start(const GmDims &g, bool first, int par, const void *B, long long ldb, const void *q, void *V0,
                           const GmSmall &s, const GmState *st, hipStream_t stream);
// beta = ||r||; V_0 *= 1 / beta; workgroup 0 of a column: g = beta e_1, hsum = 0, tol_c (first), the decision (non-finite:
// 2, beta <= tol: 0) into slot par ^ 1 (first: slot 0, from nothing) and the record
hipError_t launch_gm_begin(const GmDims &g, bool first, int par, double rtol, double atol, void *V0, const GmSmall &s, GmState *st,
                           hipStream_t stream);
// one classical Gram-Schmidt pass of W against V_0 .. V_{k-1}, per running column of slot `par`
hipError_t launch_gm_dot(const GmDims &g, int par, int k, const void *V, const void *W, const GmSmall &s, const GmState *st,
                         hipStream_t stream);
hipError_t launch_gm_update(const GmDims &g, int par, int k, const void *V, void *W, const GmSmall &s, const GmState *st,
                            hipStream_t stream);
// iteration j of the cycle, one wave per column: Hessenberg column, rotation, estimate, the decision, 1 / ||w||; slot par ->
// par ^ 1, the record
hipError_t launch_gm_hess(const GmDims &g, int par, int j, const GmSmall &s, GmState *st, hipStream_t stream);
// Vn[:, c] = W[:, c] * inv_c on running columns of slot `par`
hipError_t launch_gm_scale(const GmDims &g, int par, const void *W, void *Vn, const GmSmall &s, const GmState *st, hipStream_t stream);
// the end of a cycle on the columns that owe an update in slot `par`: y_c = R^-1 g[0 : k_c);  U[:, c] = V[:, 0 : k_c] y_c
// (zeros where nothing is owed);  X[:, c] += Z[:, c]
hipError_t launch_gm_trsolve(const GmDims &g, int par, const GmSmall &s, const GmState *st, hipStream_t stream);
hipError_t launch_gm_combine(const GmDims &g, int par, const void *V, void *U, const GmSmall &s, const GmState *st, hipStream_t stream);
hipError_t launch_gm_axpy(const GmDims &g, int par, const void *Z, void *X, const GmState *st, hipStream_t stream);
#endif

}  // namespace bsm
