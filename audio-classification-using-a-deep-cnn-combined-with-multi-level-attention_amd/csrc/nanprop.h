// nanprop.h -- max, min and ReLU that keep NaN, as torch's relu / max_pool2d / clamp and numpy's maximum do. fmaxf / fminf return
// the OTHER operand when one is NaN, which turns a diverged weight or a NaN sample into a plausible finite score.
//
// On gfx950 these are IEEE 754-2019 maximum / minimum = v_maximum3_f32 / v_minimum3_f32: one VALU instruction per two folds
// (max(max(a, b), c) is one instruction, so a 2x2 pool + ReLU is two), no canonicalising v_max_f32 x, x in front as fmaxf needs,
// and maximum(-0, +0) = +0 as v_max_f32 gave. The host form (the *_hostsim.cpp builds) is plain C++ with the same results.
#ifndef MLA_NANPROP_H
#define MLA_NANPROP_H

#include <cmath>

#if defined(__HIPCC__)
#define MLA_NP_HD __host__ __device__ __forceinline__
#else
#define MLA_NP_HD inline
#endif

namespace mla {

MLA_NP_HD float nan_max(float a, float b) {
#if defined(__HIP_DEVICE_COMPILE__)
    return __builtin_elementwise_maximum(a, b);
#else
    if (a != a || a > b) return a;
    if (b != b || b > a) return b;
    return std::signbit(a) ? b : a;                  // equal: +0 over -0
#endif
}

MLA_NP_HD float nan_min(float a, float b) {
#if defined(__HIP_DEVICE_COMPILE__)
    return __builtin_elementwise_minimum(a, b);
#else
    if (a != a || a < b) return a;
    if (b != b || b < a) return b;
    return std::signbit(a) ? a : b;                  // equal: -0 under +0
#endif
}

MLA_NP_HD float nan_relu(float v) { return nan_max(v, 0.f); }

// ReLU of the maximum of a 2x2 window: the left-to-right chain folds into two three-operand instructions
MLA_NP_HD float nan_pool_relu(float a, float b, float c, float d) { return nan_max(nan_max(nan_max(nan_max(a, b), c), d), 0.f); }

}  // namespace mla

#endif
