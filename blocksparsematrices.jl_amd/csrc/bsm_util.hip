// bsm_util.hip -- the kernels around the products (launchers declared in bsm_kernels.h): the vector helpers of the
// multi-device fan-out, COO export, device-side packing, synthetic operators and the bare streaming read.
#include "bsm_device.h"

namespace bsm {

// ---- vector helpers of the multi-device fan-out (bsm_dist.cpp) ---------------------------------
// dst[i] += src[i]: a halo segment received from a peer is added to the local result
template <typename T>
__global__ void __launch_bounds__(256) vec_add_kernel(T *__restrict__ dst, const T *__restrict__ src, long long n) {
    long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    const long long stride = (long long)gridDim.x * blockDim.x;
    for (; i < n; i += stride) dst[i] = add(dst[i], src[i]);
}
// y[i] = beta * y[i] + r[i]: the delivered segment meets the caller's y (numeric beta)
template <typename T>
__global__ void __launch_bounds__(256) vec_axpby_kernel(T *__restrict__ y, const T *__restrict__ r, long long n, T beta) {
    long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    const long long stride = (long long)gridDim.x * blockDim.x;
    for (; i < n; i += stride) y[i] = madd(r[i], beta, y[i]);
}
// ---- fused fan-out kernels of multi-device handles (bsm_dist.cpp) ------------------------------------
// The devices of a context can read each other's memory over xGMI (peer access), so the vector traffic of
// a product needs no copy engine and no staging buffer: ONE launch per device gathers the x pieces the
// device's blocks read (from the caller's x or from the x parts of its peers), ONE launch adds the y
// segments the peers produced for its rows to its own and writes the result to the caller's y (beta fused).
// Every pointer is a "virtual base": element i of the global vector lives at base + i.
template <typename T>
__global__ void __launch_bounds__(256) vec_fetch_kernel(T *__restrict__ dst, long long ld_dst, VecPieces pc, long long ld_src) {
    const int c = blockIdx.y;
    const T *__restrict__ src = reinterpret_cast<const T *>(pc.base[c]) + (long long)blockIdx.z * (pc.strided[c] ? ld_src : 0);
    T *__restrict__ d = dst + (long long)blockIdx.z * ld_dst;
    const long long lo = pc.lo[c], hi = pc.hi[c];
    for (long long i = lo + (long long)blockIdx.x * blockDim.x + threadIdx.x; i < hi; i += (long long)gridDim.x * blockDim.x)
        d[i] = src[i];
}

// y[i] = (strong ? 0 : beta * y[i]) + w[i] + sum over the pieces that cover i;  accumulate_only: w[i] += ... (no y).
// rezero: zeros are written behind everything that is read (own work vector and the peers' segments, over xGMI where
// they are remote), so the work vectors are zero again when the launch is over -- the next product accumulates into
// them without a `w = 0` launch in front (bsm_dist.cpp: DistState::w_clean)
template <typename T>
__global__ void __launch_bounds__(256) vec_finish_kernel(T *__restrict__ y, long long ldy, T *__restrict__ w, long long ldw,
                                                         VecPieces pc, int npieces, long long lo, long long hi, T beta,
                                                         int strong_zero, int accumulate_only, int rezero) {
    const long long k = blockIdx.y;
    T *__restrict__ wk = w + k * ldw;
    for (long long i = lo + (long long)blockIdx.x * blockDim.x + threadIdx.x; i < hi; i += (long long)gridDim.x * blockDim.x) {
        T v = wk[i];
        for (int c = 0; c < npieces; ++c)
            if (i >= pc.lo[c] && i < pc.hi[c]) {
                T *pe = const_cast<T *>(reinterpret_cast<const T *>(pc.base[c])) + k * ldw + i;
                v = add(v, *pe);
                if (rezero) *pe = zero_of(T{});
            }
        if (accumulate_only) {
            wk[i] = v;
        } else {
            if (rezero) wk[i] = zero_of(T{});
            T *__restrict__ yk = y + k * ldy;
            yk[i] = strong_zero ? v : madd(v, beta, yk[i]);
        }
    }
}

template <typename T>
static hipError_t fetch_typed(void *dst, long long ld_dst, const VecPieces &pc, int npieces, long long ld_src, int K,
                              hipStream_t stream) {
    long long longest = 0;
    for (int c = 0; c < npieces; ++c) longest = longest > pc.hi[c] - pc.lo[c] ? longest : pc.hi[c] - pc.lo[c];
    if (npieces <= 0 || longest <= 0) return hipSuccess;
    long long nblk = (longest + 255) / 256;
    if (nblk > 1024) nblk = 1024;
    hipLaunchKernelGGL((vec_fetch_kernel<T>), dim3((unsigned)nblk, (unsigned)npieces, (unsigned)K), dim3(256), 0, stream, (T *)dst,
                       ld_dst, pc, ld_src);
    return hipGetLastError();
}
hipError_t launch_vec_fetch(int dtype, void *dst, long long ld_dst, const VecPieces &pc, int npieces, long long ld_src, int K,
                            hipStream_t stream) {
    switch (dtype) {
        case 0: return fetch_typed<float>(dst, ld_dst, pc, npieces, ld_src, K, stream);
        case 1: return fetch_typed<double>(dst, ld_dst, pc, npieces, ld_src, K, stream);
        case 2: return fetch_typed<c64>(dst, ld_dst, pc, npieces, ld_src, K, stream);
        case 3: return fetch_typed<c128>(dst, ld_dst, pc, npieces, ld_src, K, stream);
    }
    return hipErrorInvalidValue;
}
template <typename T>
static hipError_t finish_typed(void *y, long long ldy, void *w, long long ldw, const VecPieces &pc, int npieces, long long lo,
                               long long hi, const void *beta_p, int strong_zero, int accumulate_only, int rezero, int K,
                               hipStream_t stream) {
    if (hi <= lo) return hipSuccess;
    long long nblk = (hi - lo + 255) / 256;
    if (nblk > 2048) nblk = 2048;
    hipLaunchKernelGGL((vec_finish_kernel<T>), dim3((unsigned)nblk, (unsigned)K), dim3(256), 0, stream, (T *)y, ldy, (T *)w, ldw, pc,
                       npieces, lo, hi, load_scalar<T>(beta_p, 0.0), strong_zero, accumulate_only, rezero);
    return hipGetLastError();
}
hipError_t launch_vec_finish(int dtype, void *y, long long ldy, void *w, long long ldw, const VecPieces &pc, int npieces,
                             long long lo, long long hi, const void *beta, int strong_zero, int accumulate_only, int rezero, int K,
                             hipStream_t stream) {
    switch (dtype) {
        case 0: return finish_typed<float>(y, ldy, w, ldw, pc, npieces, lo, hi, beta, strong_zero, accumulate_only, rezero, K, stream);
        case 1: return finish_typed<double>(y, ldy, w, ldw, pc, npieces, lo, hi, beta, strong_zero, accumulate_only, rezero, K, stream);
        case 2: return finish_typed<c64>(y, ldy, w, ldw, pc, npieces, lo, hi, beta, strong_zero, accumulate_only, rezero, K, stream);
        case 3: return finish_typed<c128>(y, ldy, w, ldw, pc, npieces, lo, hi, beta, strong_zero, accumulate_only, rezero, K, stream);
    }
    return hipErrorInvalidValue;
}

// y[lo_c + i] += src_c[i], i < hi_c - lo_c, for up to kMaxVecPieces DISJOINT segments in one launch (blockIdx.y = segment):
// the delivery of a row-partitioned product in the process-per-GPU layer (distributed.py: own rows of the boundary
// blocks' sums + every received partial-y segment) -- one launch behind the join instead of one per segment.
// Here pc.base[c] is the segment's own first element (not a virtual base), lo / hi its range in y.
template <typename T>
__global__ void __launch_bounds__(256) vec_add_segments_kernel(T *__restrict__ y, VecPieces pc) {
    const int c = blockIdx.y;
    const T *__restrict__ src = reinterpret_cast<const T *>(pc.base[c]);
    const long long lo = pc.lo[c], n = pc.hi[c] - lo;
    for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (long long)gridDim.x * blockDim.x)
        y[lo + i] = add(y[lo + i], src[i]);
}
template <typename T>
static hipError_t add_segments_typed(void *y, const VecPieces &pc, int npieces, hipStream_t stream) {
    long long longest = 0;
    for (int c = 0; c < npieces; ++c) longest = longest > pc.hi[c] - pc.lo[c] ? longest : pc.hi[c] - pc.lo[c];
    if (npieces <= 0 || longest <= 0) return hipSuccess;
    long long nblk = (longest + 255) / 256;
    if (nblk > 1024) nblk = 1024;
    hipLaunchKernelGGL((vec_add_segments_kernel<T>), dim3((unsigned)nblk, (unsigned)npieces), dim3(256), 0, stream, (T *)y, pc);
    return hipGetLastError();
}
hipError_t launch_vec_add_segments(int dtype, void *y, const VecPieces &pc, int npieces, hipStream_t stream) {
    switch (dtype) {
        case 0: return add_segments_typed<float>(y, pc, npieces, stream);
        case 1: return add_segments_typed<double>(y, pc, npieces, stream);
        case 2: return add_segments_typed<c64>(y, pc, npieces, stream);
        case 3: return add_segments_typed<c128>(y, pc, npieces, stream);
    }
    return hipErrorInvalidValue;
}

template <typename T>
static hipError_t vec_launch(int which, void *dst, const void *src, long long n, const void *beta_p, hipStream_t stream) {
    if (n <= 0) return hipSuccess;
    long long nblk = (n + 255) / 256;
    if (nblk > 4096) nblk = 4096;
    if (which == 0)
        hipLaunchKernelGGL((vec_add_kernel<T>), dim3((unsigned)nblk), dim3(256), 0, stream, (T *)dst, (const T *)src, n);
    else
        hipLaunchKernelGGL((vec_axpby_kernel<T>), dim3((unsigned)nblk), dim3(256), 0, stream, (T *)dst, (const T *)src, n,
                           load_scalar<T>(beta_p, 0.0));
    return hipGetLastError();
}
hipError_t launch_vec_add(int dtype, void *dst, const void *src, long long n, hipStream_t stream) {
    switch (dtype) {
        case 0: return vec_launch<float>(0, dst, src, n, nullptr, stream);
        case 1: return vec_launch<double>(0, dst, src, n, nullptr, stream);
        case 2: return vec_launch<c64>(0, dst, src, n, nullptr, stream);
        case 3: return vec_launch<c128>(0, dst, src, n, nullptr, stream);
    }
    return hipErrorInvalidValue;
}
hipError_t launch_vec_axpby(int dtype, void *y, const void *r, long long n, const void *beta, hipStream_t stream) {
    switch (dtype) {
        case 0: return vec_launch<float>(1, y, r, n, beta, stream);
        case 1: return vec_launch<double>(1, y, r, n, beta, stream);
        case 2: return vec_launch<c64>(1, y, r, n, beta, stream);
        case 3: return vec_launch<c128>(1, y, r, n, beta, stream);
    }
    return hipErrorInvalidValue;
}

// ========================================================================================
// rowcolvals(A) from the packed image (reference src/sparse.jl:17-123): every stored entry leaves as
// a COO triple (1-based), the off-diagonal columns of a symmetric operator a second time transposed.
// One wave per WaveWork descriptor; its output offset was summed up on the host (no atomics, the
// order of the triples is fixed).  HBM-bound, one-off.
// ========================================================================================
// S: the stored type; a mixed-precision image's values leave widened to T
template <typename T, typename S = T>
__global__ void __launch_bounds__(64 * kWavesPerWg) export_coo_kernel(const WaveWork *__restrict__ waves, long long nwaves,
                                                         const long long *__restrict__ out_off,
                                                         const uint4 *__restrict__ values, const int *__restrict__ rows,
                                                         const int *__restrict__ cols, long long *__restrict__ orow,
                                                         long long *__restrict__ ocol, T *__restrict__ oval) {
    constexpr int E = TT<S>::E;
    const long long wv = (long long)blockIdx.x * kWavesPerWg + (threadIdx.x >> 6);
    if (wv >= nwaves) return;
    const int lane = threadIdx.x & 63;
    const WaveD wd = load_wave(waves + wv);
    if (wd.work != WORK_PANEL || wd.npieces == 0) return;
    const PieceD pc = wd.first;
    const int m = wd.m, ncols = pc.ncols, kinds = pc.kind;
    const S *__restrict__ vb = reinterpret_cast<const S *>(values + (((uint64_t)pc.val_hi << 32) | pc.val_lo));
    const int s1w = wd.seg1_w, s1x = wd.seg1_x - wd.seg1_w;
    const int s2w = wd.seg2_w, s2x = pc.seg2_x - wd.seg2_w;
    const long long base = out_off[wv];
    const long long tbase = base + (long long)m * ncols;  // transposed copies follow the forward triples
    // t-th KIND_OFF column of the piece gets the t-th transposed slot: count them in order per lane
    // group is not needed -- the host laid the transposed region out per column index w as well, with
    // holes squeezed out by its own prefix; here the prefix over columns is recomputed by lane 0..63
    // cooperatively in chunks of 64 columns
    int toff = 0;  // number of KIND_OFF columns in front of the current chunk
    for (int w0 = 0; w0 < ncols; w0 += 64) {
        const int w = w0 + lane;
        bool off = false;
        int ci = 0;
        if (w < ncols) {
            if (pc.xbase < 0) {
                const int raw = cols[pc.col_off + w];
                off = raw >= 0 && (kinds & 3) == KIND_OFF;
                ci = raw & 0x7fffffff;
            } else {
                const int sh = w < s1w ? 0 : (w < s2w ? 2 : 4);
                off = ((kinds >> sh) & 3) == KIND_OFF;
                ci = w + (w < s1w ? pc.xbase : (w < s2w ? s1x : s2x));
            }
        }
        const unsigned long long mask = __ballot(off);
        const int rank = __popcll(mask & ((1ull << lane) - 1ull));
        if (w < ncols) {
            const int s = w / E, e = w % E;
            for (int i = 0; i < m; ++i) {
                const int ri = (wd.rbase >= 0) ? wd.rbase + i : rows[wd.row_off + i];
                const T v = widen(T{}, vb[((long long)s * m + i) * E + e]);
                const long long o = base + (long long)w * m + i;
                orow[o] = ri + 1;
                ocol[o] = ci + 1;
                oval[o] = v;
                if (off) {
                    const long long t = tbase + (long long)(toff + rank) * m + i;
                    orow[t] = ci + 1;
                    ocol[t] = ri + 1;
                    oval[t] = v;
                }
            }
        }
        toff += __popcll(mask);
    }
}

hipError_t launch_export_coo(int dtype, const void *d_waves, long long nwaves, const void *d_out_off,
                             const void *d_values, const void *d_rows, const void *d_cols, void *orow, void *ocol,
                             void *oval, hipStream_t stream) {
    if (nwaves <= 0) return hipSuccess;
    const dim3 grid((unsigned)((nwaves + kWavesPerWg - 1) / kWavesPerWg)), block(64 * kWavesPerWg);
#define BSM_EXPORT(T, S)                                                                                          \
    hipLaunchKernelGGL((export_coo_kernel<T, S>), grid, block, 0, stream, (const WaveWork *)d_waves, nwaves,         \
                       (const long long *)d_out_off, (const uint4 *)d_values, (const int *)d_rows,                \
                       (const int *)d_cols, (long long *)orow, (long long *)ocol, (T *)oval)
    switch (dtype) {
        case 0: BSM_EXPORT(float, float); break;
        case 1: BSM_EXPORT(double, double); break;
        case 2: BSM_EXPORT(c64, c64); break;
        case 3: BSM_EXPORT(c128, c128); break;
        case 4: BSM_EXPORT(double, float); break;
        case 5: BSM_EXPORT(c128, c64); break;
        default: return hipErrorInvalidValue;
    }
#undef BSM_EXPORT
    return hipGetLastError();
}

// ========================================================================================
// device-side repacking (bsm_options.blocks_memspace = BSM_MEM_DEVICE): the caller's blocks already
// live in HBM (e.g. ROCArrays), so the strip layout is written by a kernel instead of the host
// packer -- no matrix byte crosses PCIe.  One workgroup per chunk (<= 64 rows of one block);
// consecutive lanes read consecutive rows of a column (coalesced) and write the same slot of
// consecutive 16-byte units.  HBM-bound, runs once per operator.
// ========================================================================================
template <typename U>
__global__ void __launch_bounds__(256) pack_kernel(const PackChunk *__restrict__ plan, const int *__restrict__ colpos,
                                                   U *__restrict__ values, int E) {
    const PackChunk c = plan[blockIdx.x];
    const U *__restrict__ src = reinterpret_cast<const U *>(c.src);
    U *__restrict__ dst = values + c.dst_unit * (uint64_t)E;
    const int mc = c.mc;
    // lanes run over the rows of the chunk, rounded up to a power of two <= 64 so that a wave covers
    // whole columns
    int rp = 1;
    while (rp < mc) rp <<= 1;
    const int i = threadIdx.x & (rp - 1);
    const int cpw = 256 / rp;  // columns per pass
    if (i >= mc) return;
    for (int w = threadIdx.x / rp; w < c.n; w += cpw) {
        const int q = c.perm_off < 0 ? c.woff + w : colpos[c.perm_off + w];
        const U v = c.trans ? src[(int64_t)w + (int64_t)(c.ra + i) * c.ld] : src[(int64_t)(c.ra + i) + (int64_t)w * c.ld];
        dst[((int64_t)(q / E) * mc + i) * E + (q % E)] = v;
    }
}

// the converting variant of mixed-precision handles: the caller's double / complex double blocks are rounded to the
// stored float / complex float as they are placed -- the round-to-nearest-even conversion (v_cvt_f32_f64 under the
// default rounding mode, f32 denormals not flushed), bit for bit what the host packer's cast gives
__device__ __forceinline__ float narrow(double v) { return (float)v; }
__device__ __forceinline__ c64 narrow(c128 v) { return c64{(float)v.re, (float)v.im}; }
template <typename S, typename T>
__global__ void __launch_bounds__(256) pack_convert_kernel(const PackChunk *__restrict__ plan, const int *__restrict__ colpos,
                                                           S *__restrict__ values) {
    constexpr int E = TT<S>::E;
    const PackChunk c = plan[blockIdx.x];
    const T *__restrict__ src = reinterpret_cast<const T *>(c.src);
    S *__restrict__ dst = values + c.dst_unit * (uint64_t)E;
    const int mc = c.mc;
    int rp = 1;
    while (rp < mc) rp <<= 1;
    const int i = threadIdx.x & (rp - 1);
    const int cpw = 256 / rp;
    if (i >= mc) return;
    for (int w = threadIdx.x / rp; w < c.n; w += cpw) {
        const int q = c.perm_off < 0 ? c.woff + w : colpos[c.perm_off + w];
        const T v = c.trans ? src[(int64_t)w + (int64_t)(c.ra + i) * c.ld] : src[(int64_t)(c.ra + i) + (int64_t)w * c.ld];
        dst[((int64_t)(q / E) * mc + i) * E + (q % E)] = narrow(v);
    }
}

hipError_t launch_pack(int es, int src_es, const void *d_plan, long long nchunks, const void *d_colpos, void *d_values,
                       hipStream_t stream) {
    if (nchunks <= 0) return hipSuccess;
    const PackChunk *plan = (const PackChunk *)d_plan;
    const int *cp = (const int *)d_colpos;
    const dim3 grid((unsigned)nchunks), block(256);
    if (src_es != es) {  // mixed precision: 8 -> 4 bytes (double -> float) or 16 -> 8 (complex double -> complex float)
        if (es == 4)
            hipLaunchKernelGGL((pack_convert_kernel<float, double>), grid, block, 0, stream, plan, cp, (float *)d_values);
        else
            hipLaunchKernelGGL((pack_convert_kernel<c64, c128>), grid, block, 0, stream, plan, cp, (c64 *)d_values);
        return hipGetLastError();
    }
    if (es == 4)
        hipLaunchKernelGGL((pack_kernel<uint32_t>), grid, block, 0, stream, plan, cp, (uint32_t *)d_values, 4);
    else if (es == 8)
        hipLaunchKernelGGL((pack_kernel<uint64_t>), grid, block, 0, stream, plan, cp, (uint64_t *)d_values, 2);
    else
        hipLaunchKernelGGL((pack_kernel<uint4>), grid, block, 0, stream, plan, cp, (uint4 *)d_values, 1);
    return hipGetLastError();
}

// ========================================================================================
// synthetic operators of BASELINE.json generated IN HBM (include/bsm_synth.h): the counter-based
// SplitMix64 streams of blocksparsematrices.jl_amd/synthetic.py, bit-identical to the numpy code.
//   u(s, k) = mix(s + GOLDEN * (k + 1)),  value = (u >> 11) * 2^-53 * 2 - 1  (fp64, then cast)
// ========================================================================================
__host__ __device__ __forceinline__ uint64_t synth_mix(uint64_t z) {
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    return z ^ (z >> 31);
}
__device__ __forceinline__ double synth_unit(uint64_t stream, uint64_t k) {
    const uint64_t u = synth_mix(stream + 0x9E3779B97F4A7C15ull * (k + 1));
    return (double)(u >> 11) * 0x1.0p-53 * 2.0 - 1.0;
}
__device__ __forceinline__ void synth_store(float *p, double v) { *p = (float)v; }
__device__ __forceinline__ void synth_store(double *p, double v) { *p = v; }

struct SynthBlock {
    uint64_t dst;     // device address, column-major m x n, leading dimension m
    uint64_t stream;  // mix(seed ^ mix(b + 1))
    int32_t m, n;
    int32_t symmetrise, pad;  // 1: (D + D^T) / 2 of the m x m draw (diagonal blocks, docs/src/symmetric.md:49-50)
};

template <typename T>
__global__ void __launch_bounds__(256) synth_blocks_kernel(const SynthBlock *__restrict__ blocks) {
    const SynthBlock b = blocks[blockIdx.x];
    T *__restrict__ dst = reinterpret_cast<T *>(b.dst);
    const long long cnt = (long long)b.m * b.n;
    for (long long k = (long long)blockIdx.y * 256 + threadIdx.x; k < cnt; k += (long long)gridDim.y * 256) {
        double v = synth_unit(b.stream, (uint64_t)k);
        if (b.symmetrise) {
            const long long i = k % b.m, j = k / b.m;
            // the reference recipe rounds the draw to T first, then averages in T
            const T a = (T)v, c = (T)synth_unit(b.stream, (uint64_t)(j + i * b.m));
            dst[k] = (a + c) / (T)2;
        } else {
            synth_store(&dst[k], v);
        }
    }
}

template <typename T>
__global__ void __launch_bounds__(256) synth_vector_kernel(T *__restrict__ dst, long long n, uint64_t stream) {
    long long k = (long long)blockIdx.x * 256 + threadIdx.x;
    const long long stride = (long long)gridDim.x * 256;
    for (; k < n; k += stride) synth_store(&dst[k], synth_unit(stream, (uint64_t)k));
}

// ========================================================================================
// Bare streaming read (include/bsm_synth.h: bsm_bench_stream): what the memory system delivers for a
// buffer of a given size with the product kernel's request shape -- 8 independent 16-byte non-temporal
// loads per lane, 8 KB per wave, 4 waves per workgroup -- and nothing else to do.  `hop` adds the one
// dependent scalar load every product wave starts with (its 64-byte descriptor): the wave's offset comes
// out of a table instead of blockIdx.  The floor bench.py prints beside the product's time.
// ========================================================================================
__global__ void __launch_bounds__(256) stream_floor_kernel(const u32x4 *__restrict__ src, double *__restrict__ sink,
                                                           long long total16, const long long *__restrict__ hop) {
    const int lane = threadIdx.x & 63;
    long long wave = (long long)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (hop) wave = __builtin_amdgcn_readfirstlane((int)hop[__builtin_amdgcn_readfirstlane((int)wave) * 8]);  // one 64-byte record per wave
    const long long p = wave * 512 + lane;
    u32x4 v[8];
#pragma unroll
    for (int k = 0; k < 8; k++) v[k] = __builtin_nontemporal_load(src + (p + 64 * k < total16 ? p + 64 * k : 0));
    unsigned acc = 0;
#pragma unroll
    for (int k = 0; k < 8; k++) acc += v[k].x ^ v[k].y ^ v[k].z ^ v[k].w;
    if (acc == 0x9E3779B9u) sink[wave & 1023] = (double)acc;  // keeps the loads alive; practically never taken
}

hipError_t launch_stream_floor(const void *src, long long bytes, void *sink, const void *hop, hipStream_t stream) {
    const long long total16 = bytes / 16;
    if (total16 <= 0) return hipSuccess;
    const unsigned grid = (unsigned)((total16 + 2047) / 2048);
    hipLaunchKernelGGL(stream_floor_kernel, dim3(grid), dim3(256), 0, stream, (const u32x4 *)src, (double *)sink, total16,
                       (const long long *)hop);
    return hipGetLastError();
}

hipError_t launch_synth_blocks(int dtype, const void *d_desc, long long nblocks, int tiles, hipStream_t stream) {
    if (nblocks <= 0) return hipSuccess;
    const dim3 grid((unsigned)nblocks, (unsigned)tiles), block(256);
    if (dtype == 0)
        hipLaunchKernelGGL((synth_blocks_kernel<float>), grid, block, 0, stream, (const SynthBlock *)d_desc);
    else if (dtype == 1)
        hipLaunchKernelGGL((synth_blocks_kernel<double>), grid, block, 0, stream, (const SynthBlock *)d_desc);
    else
        return hipErrorInvalidValue;
    return hipGetLastError();
}

hipError_t launch_synth_vector(int dtype, void *dst, long long n, unsigned long long stream_seed, hipStream_t stream) {
    if (n <= 0) return hipSuccess;
    long long nblk = (n + 255) / 256;
    if (nblk > 8192) nblk = 8192;
    if (dtype == 0)
        hipLaunchKernelGGL((synth_vector_kernel<float>), dim3((unsigned)nblk), dim3(256), 0, stream, (float *)dst, n, (uint64_t)stream_seed);
    else if (dtype == 1)
        hipLaunchKernelGGL((synth_vector_kernel<double>), dim3((unsigned)nblk), dim3(256), 0, stream, (double *)dst, n, (uint64_t)stream_seed);
    else
        return hipErrorInvalidValue;
    return hipGetLastError();
}


}  // namespace bsm
