// bce.hip -- nn.BCELoss(weight, reduction) on the head's sigmoid outputs: the criterion of a multi-label training step
// (formulas, bad cells and lane layout: bce_core.h). Two launches, no atomics: one wavefront per row writes the row's term and
// two counters to the workspace, and one workgroup adds them in a fixed order, the terms in double. The scale of the mean is a
// launch argument (the batch shape is fixed per HIP graph), so nothing is read back from the device and a replay is a real step.
#include "bce_core.h"
#include "common.h"

namespace {

template <typename T>
__device__ __forceinline__ T wave_sum(T v) {
    _Pragma("unroll") for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
    return v;
}

template <typename T>
__device__ __forceinline__ T block_tree_256(T v, T* part) {
    part[threadIdx.x] = v;
    __syncthreads();
    for (int o = 128; o > 0; o >>= 1) {
        if (threadIdx.x < o) part[threadIdx.x] += part[threadIdx.x + o];
        __syncthreads();
    }
    const T r = part[0];
    __syncthreads();                                        // part is used again
    return r;
}

__global__ __launch_bounds__(256) void bce_rows_kernel(const float* __restrict__ p, int64_t ldp, const float* __restrict__ y, int64_t ldt,
                                                       int64_t rows, int K, const float* __restrict__ w, float s, float* __restrict__ dp,
                                                       int64_t ld_dp, double* __restrict__ term, int32_t* __restrict__ right,
                                                       int32_t* __restrict__ bad) {
    const int lane = threadIdx.x & 63;
    const int64_t b = int64_t(blockIdx.x) * bce::kRowsPerWg + (threadIdx.x >> 6);
    if (b >= rows) return;                                  // the whole wave; no barrier below
    const float* prow = p + b * ldp;
    const float* yrow = y + b * ldt;
    float pv[bce::kPerLane], yv[bce::kPerLane], wv[bce::kPerLane];
    _Pragma("unroll") for (int j = 0; j < bce::kPerLane; ++j) {      // every load of the row in flight before the first logarithm
        const int k = lane + bce::kLanes * j;
        pv[j] = k < K ? prow[k] : 0.f;
        yv[j] = k < K ? yrow[k] : 0.f;
        wv[j] = (w && k < K) ? w[k] : 1.f;
    }
    float t = 0.f;
    int n_right = 0, n_bad = 0;
    _Pragma("unroll") for (int j = 0; j < bce::kPerLane; ++j) {
        const int k = lane + bce::kLanes * j;
        if (k < K) {
            const bce::Cell c = bce::cell(pv[j], yv[j], wv[j], s, dp != nullptr);
            t += c.term;
            n_right += c.right;
            n_bad += c.bad;
            if (dp) dp[b * ld_dp + k] = c.grad;
        }
    }
    t = wave_sum(t);
    n_right = wave_sum(n_right);
    n_bad = wave_sum(n_bad);
    if (lane == 0) {
        term[b] = double(t);
        right[b] = n_right;
        bad[b] = n_bad;
    }
}

__global__ __launch_bounds__(bce::kThreads) void bce_finish_kernel(const double* __restrict__ term, const int32_t* __restrict__ right,
                                                                   const int32_t* __restrict__ bad, int64_t rows, int K, float s,
                                                                   float* __restrict__ loss, int* __restrict__ counts) {
    __shared__ double part[bce::kThreads];
    __shared__ int ipart[bce::kThreads];
    int n3[3];
    const double sum = block_tree_256(bce::finish_thread(term, right, bad, rows, K, threadIdx.x, n3), part);
    _Pragma("unroll") for (int i = 0; i < 3; ++i) n3[i] = block_tree_256(n3[i], ipart);
    if (threadIdx.x == 0) {
        *loss = bce::finish_loss(sum, n3[1], s);
        counts[0] = n3[0]; counts[1] = n3[1]; counts[2] = n3[2];
    }
}

}  // namespace

extern "C" int64_t mla_bce_workspace_bytes(int64_t rows) { return bce::workspace_bytes(rows); }

extern "C" int mla_bce(const float* p, int64_t ldp, const float* target, int64_t ldt, int64_t rows, int K, const float* weight, int reduction,
                       float scale, float* loss, float* dp, int64_t ld_dp, int* counts, void* workspace, mla_stream_t stream) {
    MLA_REQUIRE(p && target && loss && counts && workspace, MLA_E_ARG, "bce: null p, target, loss, counts or workspace");
    MLA_REQUIRE(rows > 0, MLA_E_ARG, "bce: rows = %lld", (long long)rows);
    MLA_REQUIRE(K >= 1 && K <= bce::kMaxK, MLA_E_SHAPE, "bce: K = %d, built for 1 to %d classes (16 per lane of a wavefront)", K, bce::kMaxK);
    MLA_REQUIRE(ldp >= K && ldt >= K && (!dp || ld_dp >= K), MLA_E_ARG, "bce: a row pitch below K = %d", K);
    MLA_REQUIRE(reduction == bce::kMean || reduction == bce::kSum, MLA_E_ARG, "bce: reduction code %d (0 = mean, 1 = sum)", reduction);
    MLA_REQUIRE(reduction != bce::kMean || (scale > 0.f && scale <= 3.4028234e38f), MLA_E_ARG,
                "bce: the mean needs a finite positive scale = 1 / (global rows * K), not %g", double(scale));
    MLA_REQUIRE(mla::aligned(workspace, 8), MLA_E_ARG, "bce: the workspace must be 8-byte aligned");
    double* term = static_cast<double*>(workspace);
    int32_t* right = reinterpret_cast<int32_t*>(term + rows);
    int32_t* bad = right + rows;
    const float s = bce::scale_of(reduction, scale);
    hipStream_t st = static_cast<hipStream_t>(stream);
    hipLaunchKernelGGL(bce_rows_kernel, dim3(unsigned((rows + bce::kRowsPerWg - 1) / bce::kRowsPerWg)), dim3(256), 0, st, p, ldp, target, ldt,
                       rows, K, weight, s, dp, ld_dp, term, right, bad);
    MLA_LAUNCH_OK("bce");
    hipLaunchKernelGGL(bce_finish_kernel, dim3(1), dim3(bce::kThreads), 0, st, term, right, bad, rows, K, s, loss, counts);
    MLA_LAUNCH_OK("bce finish");
    return MLA_OK;
}
