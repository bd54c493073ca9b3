// bsm_types.h -- what the six dtype codes of include/bsm_rocm.h mean, in one place: the code of a handle's vectors, element
// sizes, the refusal of the entry points that take a vector type only, and the switch from a code to template arguments
// on the host.  (The device launchers dispatch on (T, S) pairs: bsm_device.h, with_pair.)  Plain C++17 on the standard
// library, for .cpp, .hip and the stand-alone programs of tools/ alike.
#pragma once
#include <string>
#include <type_traits>

#include "../../include/bsm_rocm.h"

namespace bsm {

constexpr bool is_vec_type(int dtype) { return dtype >= BSM_F32 && dtype <= BSM_C128; }
constexpr bool is_mixed(int dtype) { return dtype == BSM_F64_F32 || dtype == BSM_C128_C64; }
// stored code -> the code of its vectors (double / complex double under the mixed storage codes)
constexpr int vec_type(int dtype) { return dtype == BSM_F64_F32 ? BSM_F64 : dtype == BSM_C128_C64 ? BSM_C128 : dtype; }
// bytes of one element of vector type vt, and of its real components
constexpr int elem_bytes(int vt) { return vt == BSM_F32 ? 4 : vt == BSM_C128 ? 16 : 8; }
constexpr int real_bytes(int vt) { return (vt == BSM_F32 || vt == BSM_C64) ? 4 : 8; }

// why entry point `fn`, which takes a vector type, refuses `dtype` (BSM_ERR_INVALID); empty: it does not
inline std::string vec_type_refusal(const char *fn, int dtype) {
    if (is_mixed(dtype)) return std::string(fn) + " takes a vector type (BSM_F32 .. BSM_C128), not a mixed storage code";
    return is_vec_type(dtype) ? "" : "bad dtype";
}

// dtype -> f(R{}, RS{}, std::integral_constant<int, NC>{}): R the real type of the vectors, RS the real type stored,
// NC = 1 (real) or 2 (re, im) components per element.  false: no such code, f was not called.  A code the caller does
// not accept (a mixed one where vectors are meant) is refused before the call.
template <typename F> bool with_types(int dtype, F &&f) {
    using one = std::integral_constant<int, 1>;
    using two = std::integral_constant<int, 2>;
    switch (dtype) {
        case BSM_F32: f(float{}, float{}, one{}); return true;
        case BSM_F64: f(double{}, double{}, one{}); return true;
        case BSM_C64: f(float{}, float{}, two{}); return true;
        case BSM_C128: f(double{}, double{}, two{}); return true;
        case BSM_F64_F32: f(double{}, float{}, one{}); return true;
        case BSM_C128_C64: f(double{}, float{}, two{}); return true;
    }
    return false;
}

}  // namespace bsm
