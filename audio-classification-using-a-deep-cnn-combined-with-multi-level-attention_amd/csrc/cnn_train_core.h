// cnn_train_core.h -- what the f32 (cnn_train.hip) and the bf16 (cnn_train_bf16.hip) finetune backward of the VGGish stack
// share: the rules that decide a gradient's bits, each written once. The 256-lane double-precision block tree, the 2x2
// pooling window (index decomposition, torch's first-maximum tie rule, ReLU mask), the reduction of the wgrad partials, the
// bias-slot reduction and the list of the compiled wgrad shapes. The device code is inline, templated or file-local: each
// translation unit compiles alone (-fno-gpu-rdc) and launches its own copy of the two kernels. The one host function that
// crosses the two files, conv1_bwd_vector, exists only in a -DMLA_CONV1_BWD_MFMA=0 build.
#ifndef MLA_CNN_TRAIN_CORE_H
#define MLA_CNN_TRAIN_CORE_H

#include "common.h"
#include "mma_core.h"

// the (Cin, Cout, H, W) of conv2 .. conv6: the shapes mla_conv_wgrad and mla_conv_wgrad_bf16 are compiled for
#define MLA_WGRAD_SHAPES(X) X(64, 128, 48, 32) X(128, 256, 24, 16) X(256, 256, 24, 16) X(256, 512, 12, 8) X(512, 512, 12, 8)

namespace ct {

using namespace mma;

// Sum of one double per lane over a 256-lane workgroup in a fixed tree (lane t += lane t + 128, then + 64, ...): the same
// bits whatever the schedule. Every lane of the workgroup calls it; the result is valid in lane 0.
__device__ __forceinline__ double block_sum256(double s) {
    __shared__ double part[256];
    part[threadIdx.x] = s;
    __syncthreads();
    for (int w = 128; w > 0; w >>= 1) {
        if (int(threadIdx.x) < w) part[threadIdx.x] += part[threadIdx.x + w];
        __syncthreads();
    }
    return part[0];
}

// one 16-byte chunk (Elem<T>::kPerChunk elements) as floats
template <typename T>
__device__ __forceinline__ void load_chunk(const T* p, float* v) {
    if constexpr (sizeof(T) == 2) {
        load8(p, v);
    } else {
        const f32x4 a = *reinterpret_cast<const f32x4*>(p);
        _Pragma("unroll") for (int k = 0; k < 4; ++k) v[k] = a[k];
    }
}
template <typename T>
__device__ __forceinline__ void store_chunk(T* p, const float* v) {
    if constexpr (sizeof(T) == 2) store8(p, v);
    else *reinterpret_cast<f32x4*>(p) = f32x4{v[0], v[1], v[2], v[3]};
}

// The 2x2 pooling window of work item i = (n, yo, xo, c / V) of an NHWC (n, H, W, C) tensor, for a lane that owns V
// consecutive channels: element offset of position (0,0) at the lane's first channel, and of the four positions from there
// in scan order (0,0), (0,1), (1,0), (1,1). The pooled element (n, yo, xo, c) itself is element i * V.
struct Window { int64_t base, off[4]; };
template <int V>
__device__ __forceinline__ Window window_of(int64_t i, int H, int W, int C) {
    const int cv = C / V, WO = W / 2, HO = H / 2;
    const int c = int(i % cv);
    int64_t r = i / cv;
    const int xo = int(r % WO); r /= WO;
    const int yo = int(r % HO);
    const int64_t n = r / HO;
    return Window{((n * H + 2 * yo) * W + 2 * xo) * C + c * V, {0, C, int64_t(W) * C, int64_t(W) * C + C}};
}

// torch's routing rule of max_pool2d: the FIRST maximum in scan order takes the window's gradient (a later value wins
// only if it is greater). Returns its position, `best` the maximum.
__device__ __forceinline__ int first_max(float v0, float v1, float v2, float v3, float& best) {
    best = v0;
    int arg = 0;
    if (v1 > best) { best = v1; arg = 1; }
    if (v2 > best) { best = v2; arg = 2; }
    if (v3 > best) { best = v3; arg = 3; }
    return arg;
}
// ... and relu'(0) = 0: the gradient d passes only if that maximum is positive
__device__ __forceinline__ int route(float v0, float v1, float v2, float v3, float d, float& g) {
    float best;
    const int arg = first_max(v0, v1, v2, v3, best);
    g = best > 0.f ? d : 0.f;
    return arg;
}

// 1: mla_conv1_bwd_bf16 runs conv1_bwd_mfma_kernel (cnn_train_bf16.hip). 0: the vector-pipe conv1_bwd_kernel<bf16_t> of
// cnn_train.hip through this launcher (workspace: 1024 * 8 * 80 floats); build both files with the flag (scripts/conv1_bwd_check.py).
#ifndef MLA_CONV1_BWD_MFMA
#define MLA_CONV1_BWD_MFMA 1
#endif
int conv1_bwd_vector(const float* x, const float* w, const float* bias, const bf16_t* d_pooled, int64_t n, float* workspace, float* dw,
                     float* db, hipStream_t s);

namespace {

// dW[co][ci][tap] (state_dict layout) = sum over splits of partial[split][co][tap][ci], splits in order
__global__ __launch_bounds__(256) void wgrad_reduce_kernel(const float* __restrict__ partial, int splits, int cout, int cin,
                                                           float* __restrict__ dw) {
    const int64_t total = int64_t(cout) * cin * 9;
    for (int64_t i = int64_t(blockIdx.x) * 256 + threadIdx.x; i < total; i += int64_t(gridDim.x) * 256) {
        const int tap = int(i % 9);
        const int ci = int((i / 9) % cin);
        const int co = int(i / (int64_t(9) * cin));
        const size_t src = (size_t(co) * 9 + tap) * cin + ci;
        float s = 0.f;
        for (int k = 0; k < splits; ++k) s += partial[size_t(k) * total + src];
        dw[i] = s;
    }
}

// db[c] of the pool / ReLU backward kernels, one workgroup per channel. Every lane of those kernels owns V consecutive
// channels that never change (the grid-stride step is a multiple of C / V) and leaves their dZ sums in slots
// [lane * V, lane * V + V): channel c is element c % V of lanes c / V, c / V + C / V, ... -- summed 256 at a time in
// lane order, then by the block tree.
template <int V>
__global__ __launch_bounds__(256) void bias_slots_finish_kernel(const double* __restrict__ slots, int64_t n_lanes, int C,
                                                                float* __restrict__ db) {
    const int c = blockIdx.x, cv = C / V;
    double s = 0.0;
    for (int64_t l = int64_t(c / V) + int64_t(threadIdx.x) * cv; l < n_lanes; l += int64_t(256) * cv) s += slots[l * V + c % V];
    s = block_sum256(s);
    if (threadIdx.x == 0) db[c] = float(s);
}

}  // namespace
}  // namespace ct
#endif
