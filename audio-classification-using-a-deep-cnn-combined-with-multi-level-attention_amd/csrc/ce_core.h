// ce_core.h -- per-lane and per-thread arithmetic of the cross-entropy with options (train_kernels.hip: cross_entropy_den_kernel,
// cross_entropy_opts_kernel, cross_entropy_finish_kernel), shared with the host simulation csrc/ce_hostsim.cpp, which runs the
// same functions lane by lane in the kernel's order. nn.CrossEntropyLoss with class weights w, label smoothing e, ignore_index i:
//
//   lse_b  = logsumexp(x_b),  p = softmax(x_b),  W = sum_k w_k,  c_b = (1 - e) w[y_b]
//   loss_b = c_b (lse_b - x[b, y_b]) + (e / K) sum_k w_k (lse_b - x[b, k])              rows with y_b != i ("counted")
//   mean:  loss = sum_b loss_b / den,  den = sum over the counted rows of the GLOBAL batch of w[y_b];   sum: loss = sum_b loss_b
//   dx[b, k] = s [ c_b (p_k - [k == y_b]) + (e / K) (p_k W - w_k) ],  s = 1 / den (mean) | 1 (sum)
//
// The smoothing term is summed as written: every term w_k (lse - x_k) is positive (lse W - sum w_k x_k cancels). The gradient is
// the same sum regrouped so that K = 1 gives exact zeros (p = 1, W = w_0). A row that is not counted, or whose label lies outside
// [0, K) (never used as an index; the loss is NaN then), stores exact zeros -- no product with s, which may be 1 / 0.
//
// One wavefront of 64 lanes owns a row: lane l holds x[b, l + 64 j], j < 16 (K <= 1024). Reductions are xor butterflies over
// 32, 16, ..., 1: both partners add the same two values, so all lanes end with the same bits.
#ifndef MLA_CE_CORE_H
#define MLA_CE_CORE_H

#include <cmath>
#include <cstdint>

#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#define MLA_CE_HD __host__ __device__ __forceinline__
#define MLA_CE_UNROLL _Pragma("unroll")
#else
#define MLA_CE_HD inline
#define MLA_CE_UNROLL
#endif

namespace ce {

constexpr int kLanes = 64;                   // one wavefront per row
constexpr int kPerLane = 16;                 // elements of a row per lane at most
constexpr int kMaxK = kLanes * kPerLane;     // 1024 classes
constexpr int kRowsPerWg = 4;                // 256-thread workgroups
constexpr int kThreads = 256;                // of the one-workgroup denominator and finish kernels

enum Reduction { kMean = 0, kSum = 1 };
enum RowFlags { kHit = 1, kBad = 2, kCounted = 4 };      // what a row adds to counts = [n_correct, n_bad, n_counted]

MLA_CE_HD float fast_exp(float v) {
#if defined(__HIP_DEVICE_COMPILE__)
    return __expf(v);
#else
    return expf(v);
#endif
}

MLA_CE_HD float fast_log(float v) {
#if defined(__HIP_DEVICE_COMPILE__)
    return __logf(v);
#else
    return logf(v);
#endif
}

// kCounted: y != ignore_index; kBad: counted and outside [0, K). Such a label is never used as an index.
MLA_CE_HD int classify(int64_t y, int K, int64_t ignore_index) {
    if (y == ignore_index) return 0;
    return (y >= 0 && y < K) ? kCounted : (kCounted | kBad);
}

struct MaxAt { float m; int i; };

// the larger value, of equal values the smaller index: the FIRST index of the row maximum. A NaN never wins a comparison.
MLA_CE_HD MaxAt max_combine(MaxAt a, MaxAt b) { return (b.m > a.m || (b.m == a.m && b.i < a.i)) ? b : a; }

// lane `lane`'s share of the row: xv[j] = x[lane + 64 j]
MLA_CE_HD MaxAt lane_max(const float* xv, int K, int lane) {
    MaxAt r = {-INFINITY, kMaxK};
    MLA_CE_UNROLL for (int j = 0; j < kPerLane; ++j) {
        const int k = lane + kLanes * j;
        if (k < K && xv[j] > r.m) r = MaxAt{xv[j], k};
    }
    return r;
}

MLA_CE_HD float lane_sum_exp(const float* xv, int K, int lane, float mx) {
    float s = 0.f;
    MLA_CE_UNROLL for (int j = 0; j < kPerLane; ++j)
        if (lane + kLanes * j < K) s += fast_exp(xv[j] - mx);
    return s;
}

// the lane's share of sum_k w_k (lse - x_k) and of W; w == nullptr: all ones
MLA_CE_HD void lane_smooth(const float* xv, const float* w, int K, int lane, float lse, float* t, float* wsum) {
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
    float a = 0.f, b = 0.f;
    MLA_CE_UNROLL for (int j = 0; j < kPerLane; ++j) {
        const int k = lane + kLanes * j;
        if (k < K) {
            const float wk = w ? w[k] : 1.f;
            a += wk * (lse - xv[j]);
            b += wk;
        }
    }
    *t = a;
    *wsum = b;
}

// what the row shares among its elements: c = (1 - e) w[y], ek = e / K, and the reduced sums
struct Row { float lse, c, ek, wsum, s; int y; };

// loss_b; `t` = sum_k w_k (lse - x_k), read only when e > 0
MLA_CE_HD double row_loss(const Row& r, float x_y, float t) {
    double v = double(r.c) * double(r.lse - x_y);
    if (r.ek > 0.f) v += double(r.ek) * double(t);
    return v;
}

MLA_CE_HD float dx_elem(const Row& r, float x, int k, float wk) {
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
    const float p = fast_exp(x - r.lse);
    float g = r.c * (p - (k == r.y ? 1.f : 0.f));
    if (r.ek > 0.f) g = g + r.ek * (p * r.wsum - wk);
    return g * r.s;
}

// thread `tid` of kThreads: its share of den = sum over the counted in-range rows of w[y]
MLA_CE_HD double den_thread(const int64_t* labels, int64_t rows, int K, const float* w, int64_t ignore_index, int tid) {
    double acc = 0.0;
    for (int64_t b = tid; b < rows; b += kThreads) {
        const int64_t y = labels[b];
        if (classify(y, K, ignore_index) == kCounted) acc += w ? double(w[y]) : 1.0;
    }
    return acc;
}

// thread `tid` of kThreads: its share of the row terms and of the three counters
MLA_CE_HD double finish_thread(const double* term, const int32_t* flags, int64_t rows, int tid, int* n3) {
    double acc = 0.0;
    n3[0] = n3[1] = n3[2] = 0;
    for (int64_t b = tid; b < rows; b += kThreads) {
        acc += term[b];
        const int f = flags[b];
        n3[0] += f & 1; n3[1] += (f >> 1) & 1; n3[2] += (f >> 2) & 1;
    }
    return acc;
}

// NaN with a bad label; mean: sum / den (NaN when no row of the global batch is counted: 0 / 0, as torch), sum: the sum
MLA_CE_HD float finish_loss(double sum, int n_bad, int reduction, const float* den) {
    if (n_bad > 0) return NAN;
    return reduction == kMean ? float(sum / double(*den)) : float(sum);
}

// workspace of mla_cross_entropy_opts: double term[rows] | int32 flags[rows], rounded up to 8 bytes
inline int64_t workspace_bytes(int64_t rows) { return rows <= 0 ? 0 : (rows * 12 + 7) / 8 * 8; }

}  // namespace ce

#endif
