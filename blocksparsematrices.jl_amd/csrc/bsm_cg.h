// bsm_cg.h -- what bsm_cg.hip (the kernels) and bsm_cg.cpp (bsm_cg_*; include/bsm_rocm.h) share: the device-side state of
// a multi-column CG / COCG solve and the launch interface.
// (No counterpart in the reference: its operators are LinearMaps handed to a Julia solver package.)
//
// The vectors X, R, P, Q, Z of a solver are n x K column-major in its own workspace with the leading dimension `ld`
// rounded up to whole 16-byte groups; the elements n .. ld - 1 of every column are ZERO and stay zero (the products
// write n rows, the kernels write whole groups computed from whole groups), so every kernel walks ld / VE unguarded
// 16-byte groups and the padding adds nothing to a sum.  Only the caller's B and X are read and written element by
// element under a guard (cg_start, cg_copy).
//
// Every launch is (krylov_grid(n, es), columns): workgroup (g, c) owns one row range of column c.  A reduction leaves one
// partial per workgroup and column, part[(c * G + g) * NC ..]; its consumers -- every workgroup of the column, each for
// itself -- add the G partials in one fixed order (lane-strided, then xor-shuffles), so all of them hold the same bits.
#pragma once
#include <cstdint>

#include "bsm_krylov.h"

namespace bsm {

constexpr int kCgMaxRhs = 16;
// column status on the device: kCgRun while the column iterates, else the bsm_cg_column.status it froze with
constexpr int kCgRun = -1;

// state of the columns between two launches.  cg_dir reads slot `in` and its workgroup 0 writes slot `out` (the slots
// alternate by iteration parity): no launch reads a scalar that the same launch replaces.
struct CgSlot {
    double rz[kCgMaxRhs][2];  // <r, z> (re, im)
    double rn[kCgMaxRhs];     // ||r||
    int32_t status[kCgMaxRhs];
    int32_t done[kCgMaxRhs];  // iterations the column's x holds
};
// what the host reads, one iteration late: copied to a pinned slot after every cg_dir
struct CgRecord {
    double rn[kCgMaxRhs];
    double bnorm[kCgMaxRhs];
    int32_t status[kCgMaxRhs];
    int32_t done[kCgMaxRhs];
};
struct CgState {
    CgSlot slot[2];
    double tol[kCgMaxRhs];   // max(rtol ||b_c||, atol): written by the first cg_dir of a solve
    int32_t brk[kCgMaxRhs];  // cg_update found pq == 0 or rz == 0 on a running column (cleared by cg_start)
    CgRecord rec;
};

#if defined(__HIPCC__) || defined(BSM_KRYLOV_LAUNCH)
// what every launch needs to know about the vectors
struct CgDims {
    int dtype;
    long long n, ld;  // rows, leading dimension of the workspace vectors (elements)
    int G, nrhs;      // krylov_grid(n, es), columns of this solve
    bool conj;        // BSM_CG_METHOD_CG: <u, v> = sum conj(u) v;  false: sum u v
};
// r = B - q (q null: r = B), padding zeroed;  pbb / pnn = the shares of ||b||^2 / ||r||^2;  prz (may be null) = the shares
// of <r, r> in the method's form;  brk cleared.  B: any ldb >= n, any element alignment.
hipError_t launch_cg_start(const CgDims &d, const void *B, long long ldb, const void *q, void *r, void *pbb, void *pnn, void *prz,
                           CgState *st, hipStream_t stream);
// the strided, guarded copy between the caller's X (ldx) and the workspace X: to_ws -- X -> ws with the padding zeroed;
// else ws -> X, n rows of nrhs columns and nothing else
hipError_t launch_cg_copy(const CgDims &d, bool to_ws, void *X, long long ldx, void *ws, hipStream_t stream);
// part = the shares of <u_c, v_c>; columns frozen in slot `par` are skipped
hipError_t launch_cg_dot(const CgDims &d, int par, const void *u, const void *v, void *part, const CgState *st, hipStream_t stream);
// running columns of slot `par`: alpha = rz / pq (pq from ppq);  x += alpha p;  r -= alpha q;  pnn, prz (may be null) as in
// cg_start.  pq == 0 or rz == 0: nothing is written but brk[c].
hipError_t launch_cg_update(const CgDims &d, int par, const void *ppq, const void *p, const void *q, void *x, void *r, void *pnn,
                            void *prz, CgState *st, hipStream_t stream);
// the decision and the new direction.  first: tol from pbb, p = z, slot 0 written from nothing (it = 0); else slot `par`
// is read, slot par ^ 1 written, running columns get p = z + (rz' / rz) p.  it: the iterations x holds after this launch.
hipError_t launch_cg_dir(const CgDims &d, bool first, int par, long long it, double rtol, double atol, const void *pbb, const void *pnn,
                         const void *prz, const void *z, void *p, CgState *st, hipStream_t stream);
#endif

}  // namespace bsm
