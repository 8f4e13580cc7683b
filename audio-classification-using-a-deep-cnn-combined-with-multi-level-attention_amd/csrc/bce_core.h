// bce_core.h -- per-cell and per-thread arithmetic of the binary cross-entropy (bce.hip: bce_rows_kernel, bce_finish_kernel), shared
// with the host simulation csrc/bce_hostsim.cpp, which runs the same functions lane by lane in the kernels' order.
// nn.BCELoss(weight, reduction) on probabilities p (rows, K) with float targets y (rows, K) in [0, 1], as ATen defines it:
//
//   term[b, k] = w_k ( (y - 1) max(log(1 - p), -100)  -  y max(log p, -100) )
//   loss       = s sum term,   s = 1 / (GLOBAL rows * K) for the mean (a launch argument), 1 for the sum
//   dp[b, k]   = ((p - y) / max((1 - p) p, 1e-12)) w_k s                         (ATen's order of the three roundings)
//
// A BAD cell has a target that is NaN or outside [0, 1], or a p outside [0, 1] (torch raises on both): no logarithm is taken of
// it, its dp is an exact zero, it is counted, and the loss of a batch that holds one is NaN. A NaN in p is not bad: it travels
// into the loss and into its own cell of dp (the clamps are written as comparisons, which a NaN fails; fmaxf would drop it).
//
// One wavefront of 64 lanes owns a row: lane l holds cells l + 64 j, j < 16 (K <= 1024). Each lane adds its terms in float32 in
// the order of j, the lanes' sums meet in an xor butterfly over 32, 16, ..., 1 (both partners add the same two values, so all
// lanes end with the same bits), and the row's term goes to the workspace as a double.
#ifndef MLA_BCE_CORE_H
#define MLA_BCE_CORE_H

#include <cmath>
#include <cstdint>

#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#define MLA_BCE_HD __host__ __device__ __forceinline__
#else
#define MLA_BCE_HD inline
#endif

namespace bce {

constexpr int kLanes = 64;                   // one wavefront per row
constexpr int kPerLane = 16;                 // cells of a row per lane at most
constexpr int kMaxK = kLanes * kPerLane;     // 1024 classes
constexpr int kRowsPerWg = 4;                // 256-thread workgroups
constexpr int kThreads = 256;                // of the one-workgroup finish kernel

enum Reduction { kMean = 0, kSum = 1 };

MLA_BCE_HD float fast_log(float v) {
#if defined(__HIP_DEVICE_COMPILE__)
    return __logf(v);
#else
    return logf(v);
#endif
}

// written so that a NaN fails the test: the negation of "inside", not a pair of "outside" comparisons, for the target
MLA_BCE_HD bool bad_cell(float p, float y) { return !(y >= 0.f && y <= 1.f) || p < 0.f || p > 1.f; }

// max(log v, -100) that keeps a NaN; log 0 = -inf becomes -100
MLA_BCE_HD float clamped_log(float v) {
    const float l = fast_log(v);
    return l < -100.f ? -100.f : l;
}

// both sides thresholded at 0.5, and 0.5 itself counts as "at least"
MLA_BCE_HD bool right_side(float p, float y) { return (p >= 0.5f) == (y >= 0.5f); }

struct Cell { float term, grad; int right, bad; };

// one cell; wk = 1 without weights. grad is computed only when asked for (0 otherwise); the term's bits do not depend on that.
MLA_BCE_HD Cell cell(float p, float y, float wk, float s, bool want_grad) {
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
    Cell c = {0.f, 0.f, 0, 0};
    if (bad_cell(p, y)) {
        c.bad = 1;
        return c;
    }
    c.term = wk * ((y - 1.f) * clamped_log(1.f - p) - y * clamped_log(p));
    c.right = right_side(p, y) ? 1 : 0;
    if (want_grad) {
        float d = (1.f - p) * p;
        d = d < 1e-12f ? 1e-12f : d;
        float g = (p - y) / d;
        g = g * wk;
        c.grad = g * s;
    }
    return c;
}

// thread `tid` of kThreads: its share of the row terms and of counts = [rows with all K cells on the right side, bad cells,
// cells on the right side]
MLA_BCE_HD double finish_thread(const double* term, const int32_t* right, const int32_t* bad, int64_t rows, int K, int tid, int* n3) {
    double acc = 0.0;
    n3[0] = n3[1] = n3[2] = 0;
    for (int64_t b = tid; b < rows; b += kThreads) {
        acc += term[b];
        n3[0] += right[b] == K ? 1 : 0;
        n3[1] += bad[b];
        n3[2] += right[b];
    }
    return acc;
}

// NaN with a bad cell, else s * sum
MLA_BCE_HD float finish_loss(double sum, int n_bad, float s) {
    if (n_bad > 0) return NAN;
    return float(sum * double(s));
}

// the scale both kernels use: the caller's under the mean, 1 under the sum
MLA_BCE_HD float scale_of(int reduction, float scale) { return reduction == kMean ? scale : 1.f; }

// workspace of mla_bce: double term[rows] | int32 right[rows] | int32 bad[rows]
inline int64_t workspace_bytes(int64_t rows) { return rows <= 0 ? 0 : rows * 16; }

}  // namespace bce

#endif
