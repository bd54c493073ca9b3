// bsm_device.h -- what more than one kernel family (bsm_kernels.hip has the index) uses: element types and their
// arithmetic, the 16-byte streaming load, the DPP / butterfly reductions, the flag bits of a launch, the wave / piece
// descriptors, and -- host side -- the frame every product launcher shares (scalars, flags, y range, launch loop, the
// FWD / TRN choice, the (image dtype, vector dtype) switch).  Included by the .hip files only.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdlib>
#include <type_traits>

#include "../../include/bsm_rocm.h"
#include "bsm_analysis.h"
#include "bsm_kernels.h"
#include "bsm_layout.h"

namespace bsm {

// ----------------------------------------------------------------------------------------
// element types
// ----------------------------------------------------------------------------------------
struct c64 {
    float re, im;
};
struct c128 {
    double re, im;
};

template <typename T> struct TT;
template <> struct TT<float> {
    static constexpr int E = 4;
};
template <> struct TT<double> {
    static constexpr int E = 2;
};
template <> struct TT<c64> {
    static constexpr int E = 2;
};
template <> struct TT<c128> {
    static constexpr int E = 1;
};

template <typename T> struct alignas(16) Vec16 {
    T v[TT<T>::E];
};
// N entries of T on a 16-byte boundary (the x entries a strip of a mixed-precision image covers)
template <typename T, int N> struct alignas(16) XVec {
    T v[N];
};

// 16-byte matrix load with the non-temporal hint (global_load_dwordx4 ... nt): every matrix byte
// is used exactly once per launch.  Measured on a bare streaming read of a C2-sized operator out of
// the Infinity Cache (tools/stream_floor.hip, mode 4): 6.65 us with the hint, 8.45 us without.
typedef unsigned int u32x4 __attribute__((ext_vector_type(4)));
template <typename T> __device__ __forceinline__ Vec16<T> load_stream16(const Vec16<T> *p) {
    const u32x4 raw = __builtin_nontemporal_load(reinterpret_cast<const u32x4 *>(p));
    Vec16<T> out;
    __builtin_memcpy(&out, &raw, 16);
    return out;
}

__device__ __forceinline__ float zero_of(float) { return 0.f; }
__device__ __forceinline__ double zero_of(double) { return 0.0; }
__device__ __forceinline__ c64 zero_of(c64) { return c64{0.f, 0.f}; }
__device__ __forceinline__ c128 zero_of(c128) { return c128{0.0, 0.0}; }

__device__ __forceinline__ float add(float a, float b) { return a + b; }
__device__ __forceinline__ double add(double a, double b) { return a + b; }
__device__ __forceinline__ c64 add(c64 a, c64 b) { return c64{a.re + b.re, a.im + b.im}; }
__device__ __forceinline__ c128 add(c128 a, c128 b) { return c128{a.re + b.re, a.im + b.im}; }

__device__ __forceinline__ float mul(float a, float b) { return a * b; }
__device__ __forceinline__ double mul(double a, double b) { return a * b; }
__device__ __forceinline__ c64 mul(c64 a, c64 b) {
    return c64{a.re * b.re - a.im * b.im, a.re * b.im + a.im * b.re};
}
__device__ __forceinline__ c128 mul(c128 a, c128 b) {
    return c128{a.re * b.re - a.im * b.im, a.re * b.im + a.im * b.re};
}

// acc + a*b
__device__ __forceinline__ float madd(float acc, float a, float b) { return fmaf(a, b, acc); }
__device__ __forceinline__ double madd(double acc, double a, double b) { return fma(a, b, acc); }
__device__ __forceinline__ c64 madd(c64 acc, c64 a, c64 b) {
    acc.re = fmaf(a.re, b.re, acc.re);
    acc.re = fmaf(-a.im, b.im, acc.re);
    acc.im = fmaf(a.re, b.im, acc.im);
    acc.im = fmaf(a.im, b.re, acc.im);
    return acc;
}
__device__ __forceinline__ c128 madd(c128 acc, c128 a, c128 b) {
    acc.re = fma(a.re, b.re, acc.re);
    acc.re = fma(-a.im, b.im, acc.re);
    acc.im = fma(a.re, b.im, acc.im);
    acc.im = fma(a.im, b.re, acc.im);
    return acc;
}

__device__ __forceinline__ float cj(float a, bool) { return a; }
__device__ __forceinline__ double cj(double a, bool) { return a; }
__device__ __forceinline__ c64 cj(c64 a, bool c) { return c64{a.re, c ? -a.im : a.im}; }
__device__ __forceinline__ c128 cj(c128 a, bool c) { return c128{a.re, c ? -a.im : a.im}; }

// a stored value in the arithmetic type T: mixed-precision images (BSM_F64_F32, BSM_C128_C64) store S = float / c64
// beside double / c128 vectors, and every stored value is widened in registers before it meets x (exact)
template <typename T> __device__ __forceinline__ T widen(T, T a) { return a; }
__device__ __forceinline__ double widen(double, float a) { return (double)a; }
__device__ __forceinline__ c128 widen(c128, c64 a) { return c128{(double)a.re, (double)a.im}; }
// ... and a real image under complex vectors keeps its value real (madd / mul above take it as it is)
__device__ __forceinline__ double widen(c128, double a) { return a; }
__device__ __forceinline__ float widen(c64, float a) { return a; }

__device__ __forceinline__ float shx(float a, int d) { return __shfl_xor(a, d, 64); }
__device__ __forceinline__ double shx(double a, int d) { return __shfl_xor(a, d, 64); }
__device__ __forceinline__ c64 shx(c64 a, int d) {
    return c64{__shfl_xor(a.re, d, 64), __shfl_xor(a.im, d, 64)};
}
__device__ __forceinline__ c128 shx(c128 a, int d) {
    return c128{__shfl_xor(a.re, d, 64), __shfl_xor(a.im, d, 64)};
}

// a REAL stored value times a complex vector entry (complex vectors under a real image: bsm_mul_cvec): two FMAs, no
// widening of the stored value into a complex number with a zero imaginary part (0 * x is not foldable without
// fast-math: four FMAs per entry)
__device__ __forceinline__ c64 mul(float a, c64 b) { return c64{a * b.re, a * b.im}; }
__device__ __forceinline__ c128 mul(double a, c128 b) { return c128{a * b.re, a * b.im}; }
__device__ __forceinline__ c64 madd(c64 acc, float a, c64 b) {
    acc.re = fmaf(a, b.re, acc.re);
    acc.im = fmaf(a, b.im, acc.im);
    return acc;
}
__device__ __forceinline__ c128 madd(c128 acc, double a, c128 b) {
    acc.re = fma(a, b.re, acc.re);
    acc.im = fma(a, b.im, acc.im);
    return acc;
}
// complex vectors under a real image: S = the real type of T (c128 / double, c64 / float)
template <typename T, typename S> constexpr bool kCvec =
    (std::is_same<T, c128>::value && std::is_same<S, double>::value) || (std::is_same<T, c64>::value && std::is_same<S, float>::value);

// hardware floating-point atomics (global_atomic_add_f32 / _f64; built with
// -munsafe-fp-atomics so no compare-and-swap loop is emitted)
__device__ __forceinline__ void atomic_acc(float *p, float v) { atomicAdd(p, v); }
__device__ __forceinline__ void atomic_acc(double *p, double v) { atomicAdd(p, v); }
__device__ __forceinline__ void atomic_acc(c64 *p, c64 v) {
    atomicAdd(&p->re, v.re);
    atomicAdd(&p->im, v.im);
}
__device__ __forceinline__ void atomic_acc(c128 *p, c128 v) {
    atomicAdd(&p->re, v.re);
    atomicAdd(&p->im, v.im);
}

// LDS accumulation (ds_add_f32 / ds_add_f64): the workgroup's y window
__device__ __forceinline__ void lds_acc(float *p, float v) { atomicAdd(p, v); }
__device__ __forceinline__ void lds_acc(double *p, double v) { atomicAdd(p, v); }
__device__ __forceinline__ void lds_acc(c64 *p, c64 v) {
    atomicAdd(&p->re, v.re);
    atomicAdd(&p->im, v.im);
}
__device__ __forceinline__ void lds_acc(c128 *p, c128 v) {
    atomicAdd(&p->re, v.re);
    atomicAdd(&p->im, v.im);
}
__device__ __forceinline__ bool is_zero(float a) { return a == 0.f; }
__device__ __forceinline__ bool is_zero(double a) { return a == 0.0; }
__device__ __forceinline__ bool is_zero(c64 a) { return a.re == 0.f && a.im == 0.f; }
__device__ __forceinline__ bool is_zero(c128 a) { return a.re == 0.0 && a.im == 0.0; }

// ----------------------------------------------------------------------------------------
// halving butterfly: every lane of a P-lane group holds V partial values; afterwards the group's
// sums are spread over its lanes: lane i keeps max(1, V/P) of them, starting at value index `pos`;
// lanes with (i & dup) != 0 hold duplicates and must not emit.
// The four exchanges inside a 16-lane row are DPP moves (row_mirror = lane^15, row_half_mirror =
// lane^7, quad_perm = lane^3, lane^1: plain VALU, no LDS traffic); only the 16- and 32-lane
// exchanges, which carry the fewest values, go through ds_bpermute.  Each exchange pairs lanes
// that agree on every bit decided so far, so both hold the same value subset.
// ----------------------------------------------------------------------------------------
template <int CTRL> __device__ __forceinline__ int dpp32(int v) {
    return __builtin_amdgcn_update_dpp(0, v, CTRL, 0xF, 0xF, false);
}
template <int CTRL> __device__ __forceinline__ float dppx(float a) {
    return __int_as_float(dpp32<CTRL>(__float_as_int(a)));
}
template <int CTRL> __device__ __forceinline__ double dppx(double a) {
    const long long v = __double_as_longlong(a);
    const int lo = dpp32<CTRL>((int)(v & 0xffffffffll));
    const int hi = dpp32<CTRL>((int)(v >> 32));
    return __longlong_as_double(((long long)hi << 32) | (unsigned int)lo);
}
template <int CTRL> __device__ __forceinline__ c64 dppx(c64 a) { return c64{dppx<CTRL>(a.re), dppx<CTRL>(a.im)}; }
template <int CTRL> __device__ __forceinline__ c128 dppx(c128 a) { return c128{dppx<CTRL>(a.re), dppx<CTRL>(a.im)}; }

constexpr int DPP_ROW_MIRROR = 0x140;       // lane ^ 15
constexpr int DPP_ROW_HALF_MIRROR = 0x141;  // lane ^ 7
constexpr int DPP_QUAD_XOR3 = 0x1B;         // quad_perm [3,2,1,0]
constexpr int DPP_QUAD_XOR1 = 0xB1;         // quad_perm [1,0,3,2]

// one exchange: BIT decides who keeps which half; XCH(v) returns the partner's value
template <typename T, int CUR, int BIT, typename XCH>
__device__ __forceinline__ void bfly_step(T *v, int i, int &pos, int &dup, XCH xch) {
    const bool hi = (i & BIT) != 0;
    if constexpr (CUR >= 2) {
        constexpr int H = CUR / 2;
#pragma unroll
        for (int j = 0; j < H; ++j) {
            const T keep = hi ? v[H + j] : v[j];
            const T send = hi ? v[j] : v[H + j];
            v[j] = add(keep, xch(send));
        }
        if (hi) pos += H;
    } else {
        v[0] = add(v[0], xch(v[0]));
        dup |= BIT;
    }
}

template <typename T, int V, int P> struct Butterfly {
    static constexpr int half(int cur) { return cur >= 2 ? cur / 2 : 1; }
    static __device__ __forceinline__ void run(T *v, int i, int &pos, int &dup) {
        constexpr int C0 = V;
        constexpr int C1 = (P >= 16) ? half(C0) : C0;  // after lane^15 (bit 3)
        constexpr int C2 = half(C1);                   // after lane^7  (bit 2)   (P >= 8 always)
        constexpr int C3 = half(C2);                   // after lane^3  (bit 1)
        constexpr int C4 = half(C3);                   // after lane^1  (bit 0)
        constexpr int C5 = (P >= 32) ? half(C4) : C4;  // after lane^16 (bit 4)
        if constexpr (P >= 16) bfly_step<T, C0, 8>(v, i, pos, dup, [](T a) { return dppx<DPP_ROW_MIRROR>(a); });
        bfly_step<T, C1, 4>(v, i, pos, dup, [](T a) { return dppx<DPP_ROW_HALF_MIRROR>(a); });
        bfly_step<T, C2, 2>(v, i, pos, dup, [](T a) { return dppx<DPP_QUAD_XOR3>(a); });
        bfly_step<T, C3, 1>(v, i, pos, dup, [](T a) { return dppx<DPP_QUAD_XOR1>(a); });
        if constexpr (P >= 32) bfly_step<T, C4, 16>(v, i, pos, dup, [](T a) { return shx(a, 16); });
        if constexpr (P >= 64) bfly_step<T, C5, 32>(v, i, pos, dup, [](T a) { return shx(a, 32); });
    }
};

// halving reduction over the lane bits D, 2D, ... 32 (the lanes that differ only in those bits hold partial
// sums of the same CUR values); afterwards as for Butterfly: lane keeps max(1, CUR * D / 64) values from `pos`
template <typename T, int CUR, int D> struct ReduceAbove {
    static __device__ __forceinline__ void run(T *v, int lane, int &pos, int &dup) {
        if constexpr (D < 64) {
            bfly_step<T, CUR, D>(v, lane, pos, dup, [](T a) { return shx(a, D); });
            ReduceAbove<T, (CUR >= 2 ? CUR / 2 : 1), D * 2>::run(v, lane, pos, dup);
        }
    }
};

#ifdef BSM_TRACE
// developer build (make trace): per-wave phase timestamps for tools/wavetrace.py.  The stamps
// (s_memtime) are parked in LDS and leave the wave once, at its end: a global store per stamp would
// sit in the in-order vmcnt queue in front of the matrix loads and triple the kernel time.
// (no relocatable device code: every translation unit that stamps has its own copy, bsm_debug_set_trace sets them all)
static __device__ unsigned long long *g_trace = nullptr;
static hipError_t set_trace_here(void *buf) { return hipMemcpyToSymbol(HIP_SYMBOL(g_trace), &buf, sizeof(buf)); }
__shared__ unsigned long long t_trace[kWavesPerWg][16];
// s_getreg operands (id | offset << 6 | (size - 1) << 11), all 32 bits: HW_REG_HW_ID = 4, HW_REG_XCC_ID = 20
#define BSM_GETREG_HW_ID (4 | (31 << 11))
#define BSM_GETREG_XCC_ID (20 | (31 << 11))
#define BSM_TSTAMP(slot)                                                  \
    do {                                                                   \
        if (lane == 0) t_trace[threadIdx.x >> 6][(slot)] = clock64();      \
    } while (0)
#else
#define BSM_TSTAMP(slot) \
    do {                 \
    } while (0)
#endif

constexpr int FLAG_STRONG_ZERO = 1;
constexpr int FLAG_DIRECT = 2;
constexpr int FLAG_CONJ = 4;
constexpr int FLAG_OPT = 8;
constexpr int FLAG_RMW = 16;     // coloured launch: conflict-free by construction, plain read-modify-write
constexpr int FLAG_GATHER = 32;  // contributions are stored in the workspace, gather_kernel sums them
// multi-RHS kernels: bits 8-11 = number of ACTIVE right-hand sides of a padded batch (0: all K).  Columns past it
// read the last active column of X (valid memory, arithmetic wasted) and are never written.
constexpr int FLAG_KACT_SHIFT = 8;
#ifdef BSM_EXPERIMENT
// developer build (make exp): timing-only ablations of the fused kernel, selected by BSM_DEBUG_FLAGS
// (results are WRONG with any bit set; tools/ablate.py)
constexpr int DBG_NO_GLOBAL_ATOMICS = 1 << 16;  // transposed emission: sums outside the window are dropped
constexpr int DBG_NO_WINDOW_ADD = 1 << 17;      // ... sums inside the window are dropped
constexpr int DBG_NO_BUTTERFLY = 1 << 18;       // lane-local values are parked instead of the group sums
constexpr int DBG_NO_EMISSION = 1 << 19;        // the emission loop is skipped altogether
constexpr int DBG_NO_XGATHER = 1 << 20;         // the x slice is a constant (no column-list / x loads)
constexpr int DBG_NO_FWD_OUT = 1 << 21;         // forward sums are not written
constexpr int DBG_NO_MATRIX = 1 << 22;          // multi-RHS tile pipeline: the matrix loads are not issued
constexpr int DBG_NO_FWD_HALF = 1 << 23;        // ... the forward half of an iteration is skipped
constexpr int DBG_NO_TRN_HALF = 1 << 24;        // ... the transposed half of an iteration is skipped
#define BSM_DBG(bit) ((flags & (bit)) != 0)
#else
#define BSM_DBG(bit) false
#endif

// ----------------------------------------------------------------------------------------
// descriptors: fetched as whole 16-byte words through a wave-uniform address (scalar loads),
// so a wave reaches its matrix bytes after ONE dependent memory round trip.
// ----------------------------------------------------------------------------------------
struct PieceD {
    uint32_t val_lo, val_hi;
    int xbase, col_off, nstrips, ncols, kind, seg2_x;
};
struct WaveD {
    int npieces, row_off, rbase, m, work, grp, lead, wg_sync, seg1_w, seg1_x, seg2_w, win_base, win_n;
    PieceD first;
};

__device__ __forceinline__ PieceD decode_piece(const uint4 a, const uint4 b) {
    PieceD p;
    p.val_lo = a.x;
    p.val_hi = a.y;
    p.xbase = (int)a.z;
    p.col_off = (int)a.w;
    p.nstrips = (int)b.x;
    p.ncols = (int)b.y;
    p.kind = (int)b.z;
    p.seg2_x = (int)b.w;
    return p;
}

__device__ __forceinline__ WaveD load_wave(const WaveWork *__restrict__ wp) {
    const uint4 *__restrict__ q = reinterpret_cast<const uint4 *>(wp);
    const uint4 q0 = q[0], q1 = q[1], q2 = q[2], q3 = q[3];
    WaveD w;
    w.seg1_w = (int)q0.x;
    w.win_base = (int)q0.y;
    w.row_off = (int)q0.z;
    w.rbase = (int)q0.w;
    w.m = (int)(q1.x & 0xffffu);
    w.work = (int)((q1.x >> 16) & 0xffu);
    w.grp = (int)(q1.x >> 24);
    w.lead = (int)(q1.y & 0xffu);
    w.wg_sync = (int)((q1.y >> 8) & 0xffu);
    w.npieces = (int)((q1.y >> 16) & 0xffu);
    w.win_n = (int)(q1.y >> 24) * 8;
    w.seg1_x = (int)q1.z;
    w.seg2_w = (int)q1.w;
    w.first = decode_piece(q2, q3);
    return w;
}

// piece column -> x / y index: up to three inline contiguous runs, else the cols pool.  Per-column kinds: two bits per
// run (the pool: one kind for the piece, a list entry's sign bit takes the column out of it)
struct ColMap {
    int xbase, col_off, kinds, s1w, s1x, s2w, s2x;
};
__device__ __forceinline__ ColMap col_map(const WaveD &wd, const PieceD &pc) {
    return {pc.xbase, pc.col_off, pc.kind, wd.seg1_w, wd.seg1_x - wd.seg1_w, wd.seg2_w, pc.seg2_x - wd.seg2_w};
}
// -> x / y index of piece column w, `raw` its list entry where the piece has a list; `off` tells whether the column is KIND_OFF
// (il_panel.  run_panel, PanelSetup of bsm_multi.hip and export_coo_kernel keep this decode in their own text: hipcc schedules them
// differently around the shared form -- docs/experiments_r12.md)
__device__ __forceinline__ int col_decode(const ColMap &cm, int w, int raw, bool &off) {
    if (cm.xbase < 0) {
        off = raw >= 0 && (cm.kinds & 3) == KIND_OFF;
        return raw & 0x7fffffff;
    }
    const int sh = w < cm.s1w ? 0 : (w < cm.s2w ? 2 : 4);
    off = ((cm.kinds >> sh) & 3) == KIND_OFF;
    return w + (w < cm.s1w ? cm.xbase : (w < cm.s2w ? cm.s1x : cm.s2x));
}
// -> x / y index of row r of the wave's row group: a contiguous run, else the rows pool
__device__ __forceinline__ int row_index(const WaveD &wd, const int *rows, int r) {
    return (wd.rbase >= 0) ? wd.rbase + r : rows[wd.row_off + r];
}

// x slice staged per wave in LDS.  Forward-only kernels: 2 KB (512 fp32 / 256 fp64, complex64 / 128
// complex128 columns): the batched gather keeps one x entry per 64 columns in registers.
// Fused kernels: 2 KB too (512 fp32 ... 128 complex128 columns) -- with the y window and the emission
// staging their occupancy is bounded by LDS and by the registers of the gather.
template <typename T, bool TRN = false> constexpr int x_chunk_cols() {
    return TRN ? 2048 / (int)sizeof(T) : (sizeof(T) >= 16 ? 128 : (sizeof(T) == 8 ? 256 : 512));
}


// the two accumulator shapes of v_mfma_{f64,f32}_16x16x4 (matrix-pipe paths of the multi-RHS family, the interleaved pass)
typedef double v4f64 __attribute__((ext_vector_type(4)));
typedef float v4f32 __attribute__((ext_vector_type(4)));
__device__ __forceinline__ v4f64 mfma16(double a, double b, v4f64 c) { return __builtin_amdgcn_mfma_f64_16x16x4f64(a, b, c, 0, 0, 0); }
__device__ __forceinline__ v4f32 mfma16(float a, float b, v4f32 c) { return __builtin_amdgcn_mfma_f32_16x16x4f32(a, b, c, 0, 0, 0); }

// ----------------------------------------------------------------------------------------
// launchers
// ----------------------------------------------------------------------------------------
template <typename T> static T make_scalar(double v);
template <> inline float make_scalar<float>(double v) { return (float)v; }
template <> inline double make_scalar<double>(double v) { return v; }
template <> inline c64 make_scalar<c64>(double v) { return c64{(float)v, 0.f}; }
template <> inline c128 make_scalar<c128>(double v) { return c128{v, 0.0}; }

template <typename T> static T load_scalar(const void *p, double dflt) {
    return p ? *reinterpret_cast<const T *>(p) : make_scalar<T>(dflt);
}

template <typename T> static bool is_one(T v);
template <> inline bool is_one(float v) { return v == 1.f; }
template <> inline bool is_one(double v) { return v == 1.0; }
template <> inline bool is_one(c64 v) { return v.re == 1.f && v.im == 0.f; }
template <> inline bool is_one(c128 v) { return v.re == 1.0 && v.im == 0.0; }

// Non-temporal matrix loads: every matrix byte is used once per launch, and allocating it in the
// L2 / Infinity Cache like ordinary data costs bandwidth (a bare streaming read of a C2-sized operator
// runs 6.65 us with the hint and 8.45 us without; operators larger than the 256 MiB Infinity Cache gain
// 5-12 %, and a launch that finds the caches full of someone else's dirty lines 40 %).  The exception
// are operators that just fit the Infinity Cache: streamed with the hint they are not retained as
// well between launches (136-298 MB: 2-9 % slower), so they keep ordinary loads; so do tiny ones.
static bool stream_policy(const DeviceImage &img) {
    static const int forced = [] {
        const char *v = std::getenv("BSM_NT");
        return v ? std::atoi(v) : -1;
    }();
    if (forced >= 0) return forced != 0;
    // (operators of a few tens of MB are a single round of resident workgroups bound by one
    // workgroup's dependency chain, where the hint costs ~5 %: 27 MB 5.8 vs 6.3 us)
    const long long mb = img.value_bytes >> 20;
    // One rule for exclusive AND accumulate-mode launches.  (Round 2 kept the hint for every fused operator from 40 MB
    // on: "a 242 MB fused symmetric product runs the same warm either way".  The tiled BEM fixture does not --
    // profiles/r04_nt_sweep.txt, hint / plain in us: fp32 109 MB 30.9 / 29.0, 163 MB 44.2 / 39.8, 218 MB 61.4 / 53.5;
    // fp64 203 MB 50.1 / 42.7, 254 MB 60.7 / 51.1, 305 MB 71.4 / 68.4, 407 MB 85.7 / 85.9; ComplexF64 98 MB 24.1 / 25.8,
    // 196 MB 45.9 / 43.9, 392 MB 81.8 / 85.0, 783 MB 145 / 151: between ~100 and ~320 MB of values the operator stays in
    // the Infinity Cache between two products only when it is loaded like ordinary data.)
    return (mb >= 40 && mb < 100) || mb > 320;  // measured crossovers: ~105 MB and ~310-330 MB of values
}

// ---- the frame every product launcher shares --------------------------------------------------------------------------
// flags of every launch of a product (BSM_EXPERIMENT builds: timing-only ablations from BSM_DEBUG_FLAGS on top)
static int base_flags(bool opT, bool conj, int strong_zero) {
    int flags = 0;
    if (strong_zero) flags |= FLAG_STRONG_ZERO;
    if (conj) flags |= FLAG_CONJ;
    if (opT) flags |= FLAG_OPT;
#ifdef BSM_EXPERIMENT
    if (const char *v = std::getenv("BSM_DEBUG_FLAGS")) flags |= std::atoi(v) << 16;
#endif
    return flags;
}

// bsm_value_passes: one stream of the image's values is about to be enqueued -- called by launch_pair, once per batch
// it executes (launch_typed, launch_typed_multi, launch_il: each streams them once, whatever its colour launches)
static void count_value_pass(const DeviceImage &img) { __atomic_fetch_add(&img.value_passes, 1ll, __ATOMIC_RELAXED); }

// [lo, hi): the y entries an accumulating product scales by beta -- the rows the image owns (all of them for op T / C),
// or zrange when the caller (multi-device fan-out) knows which y entries this image must define
struct YRange {
    long long lo, hi;
};
static YRange y_range(const DeviceImage &img, bool opT, const long long *zrange) {
    if (zrange) return {zrange[0], zrange[1]};
    if (opT) return {0, img.ncols};
    return {img.own_lo, img.own_hi};
}

// Calls launch(waves, grid, wg_base) for every launch of an accumulating product: one launch over every workgroup
// (atomics), or one launch per colour class (plain read-modify-write: the classes touch pairwise disjoint y entries, so
// the result is bitwise reproducible).  multi: the multi-RHS kernels, which walk the coarser split of the panels
// (bsm_analysis.h: Tunables::multi_wave_bytes) where the image has one and is not coloured.
template <typename F> static void for_each_launch(const DeviceImage &img, bool multi, F &&launch) {
    const bool colored = !img.color_wg_ptr.empty();
    const bool coarse = multi && img.d_waves_multi && !colored;
    const WaveWork *waves = (const WaveWork *)(coarse ? img.d_waves_multi : img.d_waves);
    const long long nwg = coarse ? img.nwg_multi : img.nwg_main;
    const size_t nlaunch = colored ? img.color_wg_ptr.size() - 1 : 1;
    for (size_t c = 0; c < nlaunch; ++c) {
        const long long wg0 = colored ? img.color_wg_ptr[c] : 0;
        const long long wg1 = colored ? img.color_wg_ptr[c + 1] : nwg;
        if (wg1 > wg0) launch(waves, dim3((unsigned)(wg1 - wg0)), (unsigned)wg0);
    }
}

// The FWD / TRN instance of a panel kernel, passed to f as two std::bool_constants: the forward half only (op N), both
// halves (SymmetricBlockMatrix off-diagonal pieces: every product is fused), the transposed half only (op T / C)
template <typename F> static void with_halves(bool opT, bool has_off, F &&f) {
    if (has_off)
        f(std::true_type{}, std::true_type{});
    else if (!opT)
        f(std::true_type{}, std::false_type{});
    else
        f(std::false_type{}, std::true_type{});
}

// (image dtype, vector dtype vt) -> f(T{}, S{}) -- T: the type of x, y, alpha, beta; S: the type the image stores: the
// same-type pairs, mixed storage, complex vectors under a real image.  Any other pair: hipErrorInvalidValue.
static constexpr int pair_code(int img_dtype, int vt) { return img_dtype * 4 + vt; }
template <typename F> static hipError_t with_pair(int img_dtype, int vt, F &&f) {
    if (vt < BSM_F32 || vt > BSM_C128) return hipErrorInvalidValue;
    switch (pair_code(img_dtype, vt)) {
        case pair_code(BSM_F32, BSM_F32): return f(float{}, float{});
        case pair_code(BSM_F64, BSM_F64): return f(double{}, double{});
        case pair_code(BSM_C64, BSM_C64): return f(c64{}, c64{});
        case pair_code(BSM_C128, BSM_C128): return f(c128{}, c128{});
        case pair_code(BSM_F64_F32, BSM_F64): return f(double{}, float{});
        case pair_code(BSM_C128_C64, BSM_C128): return f(c128{}, c64{});
        case pair_code(BSM_F32, BSM_C64): return f(c64{}, float{});
        case pair_code(BSM_F64, BSM_C128): return f(c128{}, double{});
    }
    return hipErrorInvalidValue;
}

}  // namespace bsm
