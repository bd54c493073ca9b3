// bsm_entries.cpp -- reading entries of an operator out of its packed image (include/bsm_rocm.h): bsm_rowcolvals (every
// stored entry as a COO triple, export_coo_kernel of bsm_util.hip), bsm_submatrices and bsm_diag (A[I, J] and diag(A),
// bsm_extract.hip; analysis-only handles answer from their host image by a plain loop over the same wave records).
#include <hip/hip_runtime_api.h>

#include <algorithm>
#include <cstring>
#include <string>
#include <vector>

#include "bsm_internal.h"

using namespace bsm;

namespace {
// The columns of the piece of wave record W in order, f(w, ci, off): piece column w is column ci of the operator; off:
// it is KIND_OFF, its entries stand at (ci, row) as well.  The host twin of col_decode (bsm_device.h): the cols pool with
// its sign bit (a column taken out of the piece's kind), else up to three inline segments with two kind bits each.
template <typename F> void for_each_column(const Analysis &an, const WaveWork &W, F &&f) {
    const Piece &P = W.first;
    for (int32_t w = 0; w < P.ncols; w++) {
        if (P.xbase < 0) {
            const int32_t raw = an.cols[(size_t)P.col_off + w];
            f(w, (int64_t)(raw & 0x7fffffff), raw >= 0 && (P.kind & 3) == KIND_OFF);
        } else {
            const int sh = w < W.seg1_w ? 0 : (w < W.seg2_w ? 2 : 4);
            const int64_t ci = w < W.seg1_w ? P.xbase + w : (w < W.seg2_w ? W.seg1_x + (w - W.seg1_w) : P.seg2_x + (w - W.seg2_w));
            f(w, ci, ((P.kind >> sh) & 3) == KIND_OFF);
        }
    }
}

// the images a handle is made of: one per device part that holds blocks, a single one for ordinary handles
std::vector<ImageRef> image_list(bsm_matrix_s *A) { return A->dist ? dist_images(A) : std::vector<ImageRef>{{&A->an, &A->img}}; }

// triples of one packed image -> device buffers of its device (orow / ocol int64, oval element type)
int export_image(const Analysis &an, const DeviceImage &img, void *orow, void *ocol, void *oval, hipStream_t st) {
    const long long nw = (long long)an.waves.size();
    std::vector<long long> off((size_t)nw + 1, 0);
    for (long long w = 0; w < nw; w++) {
        const WaveWork &W = an.waves[w];
        long long cnt = 0;
        if (W.work == WORK_PANEL && W.npieces > 0) {
            long long noff = 0;  // a KIND_OFF column leaves twice
            for_each_column(an, W, [&](int32_t, int64_t, bool off) { noff += off; });
            cnt = (long long)W.m * (W.first.ncols + noff);
        }
        off[w + 1] = off[w] + cnt;
    }
    if (off[nw] != an.nnz) return fail(BSM_ERR_DEVICE, "rowcolvals: image / nnz mismatch");
    if (nw == 0 || an.nnz == 0) return BSM_OK;
    DevBuf d_off;
    hipError_t e = d_off.alloc(off.size() * sizeof(long long));
    if (e == hipSuccess) e = hipMemcpyAsync(d_off.p, off.data(), off.size() * sizeof(long long), hipMemcpyHostToDevice, st);
    if (e == hipSuccess)
        e = launch_export_coo(an.dtype, img.d_waves, nw, d_off.p, img.d_values, img.d_rows, img.d_cols, orow, ocol, oval, st);
    if (e == hipSuccess) e = hipStreamSynchronize(st);
    if (e != hipSuccess) return hip_fail(e, "rowcolvals");
    return BSM_OK;
}
}  // namespace

extern "C" int bsm_rowcolvals(bsm_matrix_t A, int64_t *rows, int64_t *cols, void *vals, int64_t *count,
                              int memspace, void *stream) {
    BSM_GUARDED(
        if (!A || !count) return fail(BSM_ERR_INVALID, "null argument");
        if (int rc = poly_refusal(A, "bsm_rowcolvals")) return rc;
        if (!rows || !cols || !vals) {
            *count = A->an.nnz;
            return BSM_OK;
        }
        if (*count < A->an.nnz) return fail(BSM_ERR_INVALID, "output buffers too small");
        if (!A->on_device) return fail(BSM_ERR_DEVICE, "handle has no device image (created with BSM_DEVICE_NONE)");
        if (memspace != BSM_MEM_HOST && memspace != BSM_MEM_DEVICE) return fail(BSM_ERR_INVALID, "bad memspace");
        const size_t es = (size_t)A->an.vs;  // the stored values leave widened to the vector type
        // one image per device part (a single one for ordinary handles); parts are written one after another
        int64_t done = 0;
        for (auto &pi : image_list(A)) {
            const Analysis &an = *pi.first;
            const DeviceImage &img = *pi.second;
            const int64_t n = an.nnz;
            if (n == 0) continue;
            DeviceGuard g;
            hipError_t e = g.enter(img.device);
            if (e != hipSuccess) return hip_fail(e, "hipSetDevice");
            // staged through buffers on the image's device unless the caller's arrays already live there
            const bool direct = memspace == BSM_MEM_DEVICE && !A->dist;
            void *const orow = rows + done, *const ocol = cols + done, *const oval = (char *)vals + (size_t)done * es;
            if (direct) {
                const int rc = export_image(an, img, orow, ocol, oval, (hipStream_t)stream);
                if (rc != BSM_OK) return rc;
            } else {
                DevBuf r, c, v;
                e = r.alloc((size_t)n * 8);
                if (e == hipSuccess) e = c.alloc((size_t)n * 8);
                if (e == hipSuccess) e = v.alloc((size_t)n * es);
                if (e != hipSuccess) return hip_fail(e, "rowcolvals staging");
                const int rc = export_image(an, img, r.p, c.p, v.p, nullptr);
                if (rc != BSM_OK) return rc;
                e = hipMemcpy(orow, r.p, (size_t)n * 8, hipMemcpyDefault);
                if (e == hipSuccess) e = hipMemcpy(ocol, c.p, (size_t)n * 8, hipMemcpyDefault);
                if (e == hipSuccess) e = hipMemcpy(oval, v.p, (size_t)n * es, hipMemcpyDefault);
                if (e != hipSuccess) return hip_fail(e, "rowcolvals copy");
            }
            done += n;
        }
        *count = done;
        return BSM_OK;)
}

// ---- bsm_submatrices / bsm_diag: entries of the operator read out of its image -------------------------------------------
namespace {
// one output window: ni x nj entries of the vector type at `out`, leading dimension ld (elements).  diag(A) is one
// window of min(nrows, ncols) x 1
struct Window {
    int64_t ni, nj, ld;
    void *out;
};

// The host image of an analysis-only handle, by a plain loop over the wave records the kernel walks (bsm_extract.hip:
// same decode, same conditions, same addresses).  R / RS: real type of the vector / stored type, NC: 2 for complex.
// maps: rset, rpos (nrows each), cset, cpos (ncols each); null: diag(A) into win[0].  The windows are zero beforehand.
template <typename R, typename RS, int NC>
void extract_host(const Analysis &an, const int32_t *maps, const std::vector<Window> &win, bool opT, bool conj) {
    const int32_t *rset = maps, *rpos = maps ? maps + an.nrows : nullptr;
    const int32_t *cset = maps ? maps + 2 * an.nrows : nullptr, *cpos = maps ? maps + 2 * an.nrows + an.ncols : nullptr;
    auto add = [&](void *base, int64_t idx, const RS *v) {
        R *p = (R *)base + idx * NC;
        p[0] += (R)v[0];
        if (NC == 2) p[NC - 1] += conj ? -(R)v[NC - 1] : (R)v[NC - 1];
    };
    const int E = an.E;
    for (const WaveWork &W : an.waves) {
        if (W.work != WORK_PANEL || W.npieces == 0) continue;
        const int64_t m = W.m;
        const RS *vb = (const RS *)(an.values.data() + W.first.val_off * 16);
        for_each_column(an, W, [&](int32_t w, int64_t ci, bool off) {
            const int64_t s = w / E, e = w % E;
            for (int64_t i = 0; i < m; i++) {
                const int64_t ri = (W.rbase >= 0) ? (int64_t)W.rbase + i : an.rows[(size_t)W.row_off + i];
                const RS *v = vb + ((s * m + i) * E + e) * NC;
                if (!maps) {
                    if (ri == ci) {
                        add(win[0].out, ri, v);
                        if (off) add(win[0].out, ri, v);
                    }
                    continue;
                }
                const int32_t fs = rset[ri];
                if (fs >= 0 && cset[ci] == fs) {
                    const Window &o = win[(size_t)fs];
                    add(o.out, opT ? cpos[ci] + o.ld * rpos[ri] : rpos[ri] + o.ld * cpos[ci], v);
                }
                if (off && ci < an.nrows && ri < an.ncols) {  // the transposed copy sits at (ci, ri)
                    const int32_t us = rset[ci];
                    if (us >= 0 && cset[ri] == us) {
                        const Window &o = win[(size_t)us];
                        add(o.out, opT ? cpos[ri] + o.ld * rpos[ci] : rpos[ci] + o.ld * cpos[ri], v);
                    }
                }
            }
        });
    }
}

// one packed image -> windows in the memory of its device (current): uploads the maps and the table of windows, zeroes
// the windows when `shape` says which they are, runs the kernel on `st` and waits for it
int extract_image(const Analysis &an, const DeviceImage &img, const std::vector<int32_t> *maps, const std::vector<ExtractOut> &table,
                  const std::vector<long long> *shape, void *d_diag, bool opT, bool conj, hipStream_t st) {
    // one allocation: the maps, behind them the table of windows and their shapes (16-byte aligned)
    DevBuf db;
    ExtractMaps mp{nullptr, nullptr, nullptr, nullptr};
    void *d_table = nullptr;
    hipError_t e = hipSuccess;
    if (maps) {
        const size_t mb = (maps->size() * 4 + 15) / 16 * 16, tb = table.size() * sizeof(ExtractOut);
        e = db.alloc(mb + tb + (shape ? shape->size() * 8 : 0));
        if (e == hipSuccess) e = hipMemcpyAsync(db.p, maps->data(), maps->size() * 4, hipMemcpyHostToDevice, st);
        d_table = (char *)db.p + mb;
        if (e == hipSuccess && !table.empty()) e = hipMemcpyAsync(d_table, table.data(), tb, hipMemcpyHostToDevice, st);
        const int *b = (const int *)db.p;
        mp = ExtractMaps{b, b + an.nrows, b + 2 * an.nrows, b + 2 * an.nrows + an.ncols};
        if (e == hipSuccess && shape) {
            long long largest = 0;
            for (size_t s = 0; s < table.size(); s++) largest = std::max(largest, (*shape)[2 * s] * (*shape)[2 * s + 1]);
            void *d_shape = (char *)d_table + tb;
            if (!shape->empty()) e = hipMemcpyAsync(d_shape, shape->data(), shape->size() * 8, hipMemcpyHostToDevice, st);
            if (e == hipSuccess)
                e = launch_zero_windows(vec_type(an.dtype), d_table, d_shape, (long long)table.size(), largest, st);
        }
    }
    if (e == hipSuccess)
        e = launch_extract(an.dtype, img.d_waves, (long long)an.waves.size(), img.d_values, img.d_rows, img.d_cols,
                           maps ? &mp : nullptr, d_table, d_diag, an.nrows, an.ncols, opT, conj, st);
    if (e == hipSuccess) e = hipStreamSynchronize(st);
    if (e != hipSuccess) return hip_fail(e, "extract");
    return BSM_OK;
}

// the checked request (maps == nullptr: diag(A), win[0] = d) on whatever the handle is made of
int extract_run(bsm_matrix_s *A, int op, const std::vector<int32_t> *maps, const std::vector<Window> &win, int memspace,
                hipStream_t stream) {
    const Analysis &an0 = A->an;
    const size_t vs = (size_t)an0.vs;
    const int vt = vec_type(an0.dtype);
    const bool opT = op != BSM_OP_N, conj = op == BSM_OP_C;
    if (!A->on_device) {  // analysis-only handle, host windows: zeroed, then summed
        for (const Window &w : win)
            for (int64_t b = 0; b < w.nj; b++) std::memset((char *)w.out + (size_t)(b * w.ld) * vs, 0, (size_t)w.ni * vs);
        const int32_t *mp = maps ? maps->data() : nullptr;
        const bool known = with_types(an0.dtype, [&](auto r, auto rs, auto nc) {
            extract_host<decltype(r), decltype(rs), decltype(nc)::value>(an0, mp, win, opT, conj);
        });
        return known ? BSM_OK : fail(BSM_ERR_INVALID, "bad dtype");
    }
    if (memspace == BSM_MEM_DEVICE && !A->dist) {  // straight into the caller's windows
        DeviceGuard g;
        hipError_t e = g.enter(A->img.device);
        if (e != hipSuccess) return hip_fail(e, "hipSetDevice");
        if (!maps) {
            if (win[0].ni == 0) return BSM_OK;
            e = hipMemsetAsync(win[0].out, 0, (size_t)win[0].ni * vs, stream);
            if (e != hipSuccess) return hip_fail(e, "hipMemsetAsync");
            return extract_image(A->an, A->img, nullptr, {}, nullptr, win[0].out, opT, conj, stream);
        }
        std::vector<ExtractOut> table(win.size());
        std::vector<long long> shape(2 * win.size());
        for (size_t s = 0; s < win.size(); s++) {
            table[s] = ExtractOut{(uint64_t)(uintptr_t)win[s].out, (long long)win[s].ld};
            shape[2 * s] = win[s].ni;
            shape[2 * s + 1] = win[s].nj;
        }
        return extract_image(A->an, A->img, maps, table, &shape, nullptr, opT, conj, stream);
    }
    // host windows, or a multi-device handle: every image adds into a zeroed, compact staging buffer on its own device;
    // the buffers come back to the host, are summed there (an entry lives in exactly one part) and delivered
    std::vector<size_t> off(win.size() + 1, 0);
    for (size_t s = 0; s < win.size(); s++) off[s + 1] = off[s] + (size_t)win[s].ni * (size_t)win[s].nj;
    const size_t total = off[win.size()];
    if (total == 0) return BSM_OK;
    std::vector<char> sum(total * vs, 0), part;
    bool first = true;
    for (auto &pi : image_list(A)) {
        DeviceGuard g;
        hipError_t e = g.enter(pi.second->device);
        if (e != hipSuccess) return hip_fail(e, "hipSetDevice");
        DevBuf stg;
        e = stg.alloc(total * vs);
        if (e == hipSuccess) e = hipMemsetAsync(stg.p, 0, total * vs, nullptr);
        if (e != hipSuccess) return hip_fail(e, "extract staging");
        std::vector<ExtractOut> table(maps ? win.size() : 0);
        for (size_t s = 0; s < table.size(); s++)
            table[s] = ExtractOut{(uint64_t)(uintptr_t)((char *)stg.p + off[s] * vs), (long long)std::max<int64_t>(win[s].ni, 1)};
        const int rc = extract_image(*pi.first, *pi.second, maps, table, nullptr, stg.p, opT, conj, nullptr);
        if (rc != BSM_OK) return rc;
        std::vector<char> &dst = first ? sum : part;
        dst.resize(total * vs);
        e = hipMemcpy(dst.data(), stg.p, total * vs, hipMemcpyDeviceToHost);
        if (e != hipSuccess) return hip_fail(e, "extract copy");
        if (!first)
            with_types(vt, [&](auto r, auto, auto) {
                using R = decltype(r);
                R *a = (R *)sum.data();
                const R *b = (const R *)part.data();
                for (size_t k = 0; k < total * vs / sizeof(R); k++) a[k] += b[k];
            });
        first = false;
    }
    for (size_t s = 0; s < win.size(); s++) {
        const Window &w = win[s];
        if (w.ni == 0 || w.nj == 0) continue;
        const char *src = sum.data() + off[s] * vs;
        if (memspace == BSM_MEM_HOST) {
            for (int64_t b = 0; b < w.nj; b++)
                std::memcpy((char *)w.out + (size_t)(b * w.ld) * vs, src + (size_t)(b * w.ni) * vs, (size_t)w.ni * vs);
        } else {
            const hipError_t e = hipMemcpy2D(w.out, (size_t)w.ld * vs, src, (size_t)w.ni * vs, (size_t)w.ni * vs, (size_t)w.nj,
                                             hipMemcpyHostToDevice);
            if (e != hipSuccess) return hip_fail(e, "extract delivery");
        }
    }
    return BSM_OK;
}
}  // namespace

extern "C" int bsm_submatrices(bsm_matrix_t A, int op, int64_t nsets, const int64_t *const *I, const int64_t *ni,
                               const int64_t *const *J, const int64_t *nj, void *const *out, const int64_t *ldo, int memspace,
                               void *stream) {
    BSM_GUARDED(
        if (!A) return fail(BSM_ERR_INVALID, "null handle");
        if (int rc = poly_refusal(A, "bsm_submatrices")) return rc;
        if (op != BSM_OP_N && op != BSM_OP_T && op != BSM_OP_C) return fail(BSM_ERR_INVALID, "bad op");
        if (memspace != BSM_MEM_HOST && memspace != BSM_MEM_DEVICE) return fail(BSM_ERR_INVALID, "bad memspace");
        if (memspace == BSM_MEM_DEVICE && !A->on_device)
            return fail(BSM_ERR_INVALID, "BSM_MEM_DEVICE windows need a device image (handle created with BSM_DEVICE_NONE)");
        if (nsets < 0 || nsets > INT32_MAX) return fail(BSM_ERR_INVALID, "bad number of sets");
        if (nsets > 0 && (!I || !ni || !J || !nj || !out || !ldo)) return fail(BSM_ERR_INVALID, "null argument");
        const Analysis &an = A->an;
        if (an.nrows > INT32_MAX || an.ncols > INT32_MAX) return fail(BSM_ERR_UNSUPPORTED, "operator too large for int32 maps");
        // the four maps over the rows and columns of the STORED operator: I indexes the rows of op(A), i.e. the columns
        // of A for op T / C.  Filling them is the duplicate check: an index is written once.
        std::vector<int32_t> maps((size_t)(2 * an.nrows + 2 * an.ncols), 0);
        int32_t *rset = maps.data(), *rpos = rset + an.nrows, *cset = rpos + an.nrows, *cpos = cset + an.ncols;
        std::fill(rset, rset + an.nrows, -1);
        std::fill(cset, cset + an.ncols, -1);
        const bool opT = op != BSM_OP_N;
        std::vector<Window> win((size_t)nsets);
        for (int64_t s = 0; s < nsets; s++) {
            const std::string set = "set " + std::to_string(s + 1) + ": ";
            if (ni[s] < 0 || nj[s] < 0 || ni[s] > INT32_MAX || nj[s] > INT32_MAX) return fail(BSM_ERR_INVALID, set + "bad size");
            if ((ni[s] > 0 && !I[s]) || (nj[s] > 0 && !J[s])) return fail(BSM_ERR_INVALID, set + "null index list");
            if (ldo[s] < std::max<int64_t>(ni[s], 1)) return fail(BSM_ERR_INVALID, set + "ldo < max(ni, 1)");
            if (ni[s] > 0 && nj[s] > 0 && !out[s]) return fail(BSM_ERR_INVALID, set + "null output window");
            for (int side = 0; side < 2; side++) {
                const int64_t *idx = side ? J[s] : I[s];
                const int64_t cnt = side ? nj[s] : ni[s];
                const bool stored_rows = (side == 0) != opT;  // this list names rows of the stored operator
                const int64_t dim = stored_rows ? an.nrows : an.ncols;
                int32_t *sm = stored_rows ? rset : cset, *pm = stored_rows ? rpos : cpos;
                for (int64_t k = 0; k < cnt; k++) {
                    const int64_t v = idx[k];
                    if (v < 1 || v > dim)
                        return fail(BSM_ERR_INVALID, set + (side ? "column" : "row") + " index " + std::to_string(v) + " outside 1.." + std::to_string(dim));
                    if (sm[v - 1] >= 0)
                        return fail(BSM_ERR_INVALID, set + (side ? "column" : "row") + " index " + std::to_string(v) +
                                                         " is listed twice (the sets must be disjoint and free of repeats)");
                    sm[v - 1] = (int32_t)s;
                    pm[v - 1] = (int32_t)k;
                }
            }
            win[(size_t)s] = Window{ni[s], nj[s], ldo[s], out[s]};
        }
        if (nsets == 0) return BSM_OK;
        return extract_run(A, op, &maps, win, memspace, (hipStream_t)stream);)
}

extern "C" int bsm_diag(bsm_matrix_t A, void *d, int memspace, void *stream) {
    BSM_GUARDED(
        if (!A) return fail(BSM_ERR_INVALID, "null handle");
        if (int rc = poly_refusal(A, "bsm_diag")) return rc;
        if (memspace != BSM_MEM_HOST && memspace != BSM_MEM_DEVICE) return fail(BSM_ERR_INVALID, "bad memspace");
        if (memspace == BSM_MEM_DEVICE && !A->on_device)
            return fail(BSM_ERR_INVALID, "a BSM_MEM_DEVICE result needs a device image (handle created with BSM_DEVICE_NONE)");
        const int64_t n = std::min(A->an.nrows, A->an.ncols);
        if (n > 0 && !d) return fail(BSM_ERR_INVALID, "d is null");
        if (n == 0) return BSM_OK;
        const std::vector<Window> win{Window{n, 1, n, d}};
        return extract_run(A, BSM_OP_N, nullptr, win, memspace, (hipStream_t)stream);)
}
