// resnet.hip -- frozen torchvision ResNet-50 v1.5 trunk (model.py:128-149 of the reference, cnn_type="resnet").
//
// Activations are NHWC in the compute dtype (f32 or bf16), accumulation f32. Kernels:
//   rn_stem_kernel    Input normalisation (model.py:84-94) + conv1 7x7/2 pad 3 (3 -> 64), tap by tap: the zero padding
//                     applies to the NORMALISED channels, so a tap outside the image contributes nothing (not -mean/std)
//   rn_conv_kernel    generic implicit-GEMM conv on MFMA (1x1 / 3x3, stride 1 / 2, Cin and Cout multiples of 64);
//                     epilogue: raw store (train mode) or per-channel scale/shift [+ residual] [+ ReLU] (eval BN)
//   rn_bn_partial_kernel / rn_bn_finish_kernel
//                     BatchNorm2d batch statistics over NHWC rows (fixed reduction order: bit-identical runs), running-stat
//                     update and the scale/shift of the normalisation; rn_bn_sums_kernel / rn_bn_finish_sums_kernel split
//                     the finish around an all-reduce of [sum x, sum x^2, rows] (SyncBN across data-parallel ranks)
//   rn_bn_apply_kernel  y = x * scale + shift [+ residual] [ReLU] (train mode)
//   rn_maxpool_kernel   MaxPool2d(3, 2, 1);  rn_avgpool_kernel  AdaptiveAvgPool2d(1) -> f32 (N, C)
#include "rn_core.h"

namespace {

using namespace rn;
using mma::load8;
using mma::store8;

// ------------------------------------------------------------------------------------------------
// stem: x (N, 224, 224) f32 -> out NHWC (N, 112, 112, 64)
// ------------------------------------------------------------------------------------------------
template <typename T>
__global__ __launch_bounds__(256) void rn_stem_kernel(const float* __restrict__ x, int single, const float* __restrict__ w,
                                                      const float* __restrict__ scale, const float* __restrict__ shift,
                                                      int relu, T* __restrict__ out) {
    __shared__ float xs[7][kImg];
    const int oy = blockIdx.x % kStemOut;
    const int64_t n = blockIdx.x / kStemOut;
    const int t = threadIdx.x, o = t & 63, pg = t >> 6;
    for (int i = t; i < 7 * kImg; i += 256) {
        const int ky = i / kImg, ix = i - ky * kImg, iy = 2 * oy - 3 + ky;
        xs[ky][ix] = (iy >= 0 && iy < kImg) ? x[(n * kImg + iy) * kImg + ix] : 0.f;
    }
    // per-tap coefficients of the normalised channels: sum_c w_c (x_c - m_c) / s_c = a x + b for a tap inside the image
    float a[49], b[49];
#pragma unroll
    for (int k = 0; k < 49; ++k) {
        const float w0 = w[(o * 3 + 0) * 49 + k], w1 = w[(o * 3 + 1) * 49 + k], w2 = w[(o * 3 + 2) * 49 + k];
        a[k] = single ? w0 * kNormInv[0] : w0 * kNormInv[0] + w1 * kNormInv[1] + w2 * kNormInv[2];
        b[k] = -(w0 * kNormMean[0] * kNormInv[0] + w1 * kNormMean[1] * kNormInv[1] + w2 * kNormMean[2] * kNormInv[2]);
    }
    __syncthreads();
    // Taps outside the image are skipped, where nn.Conv2d multiplies its zero padding by the weight: a NaN or Inf weight makes the
    // whole channel NaN there. poison = +0 for finite weights, NaN otherwise, and starts every sum.
    float wsum = 0.f;
#pragma unroll
    for (int k = 0; k < 49; ++k) wsum += a[k] + b[k];
    const float poison = wsum - wsum;
    const float sc = scale ? scale[o] : 1.f, sh = scale ? shift[o] : 0.f;
    for (int ox = pg; ox < kStemOut; ox += 4) {
        float acc = poison;
#pragma unroll
        for (int ky = 0; ky < 7; ++ky) {
            const int iy = 2 * oy - 3 + ky;
            if (iy < 0 || iy >= kImg) continue;
#pragma unroll
            for (int kx = 0; kx < 7; ++kx) {
                const int ix = 2 * ox - 3 + kx;
                if (ix >= 0 && ix < kImg) acc += a[ky * 7 + kx] * xs[ky][ix] + b[ky * 7 + kx];
            }
        }
        float v = scale ? acc * sc + sh : acc;
        if (relu) v = mla::nan_relu(v);
        mma::store_elem<T>(out + ((n * kStemOut + oy) * kStemOut + ox) * kStemC + o, v);
    }
}

// ------------------------------------------------------------------------------------------------
// implicit-GEMM conv: rows = output pixels (N*Ho*Wo), cols = Cout, K = KS*KS*Cin, on the tile of rn_core.h (conv_tile).
// ------------------------------------------------------------------------------------------------
template <typename T, int BN>
__global__ __launch_bounds__(256) void rn_conv_kernel(const T* __restrict__ in, const T* __restrict__ w, T* __restrict__ out,
                                                      const float* __restrict__ scale, const float* __restrict__ shift,
                                                      const T* __restrict__ res, int relu, int64_t M, int H, int W, int Cin,
                                                      int Ho, int Wo, int Cout, int KS, int stride, int pad) {
    int64_t abase[kTileAL];
    int aiy[kTileAL], aix[kTileAL];
    bool aval[kTileAL];
#pragma unroll
    for (int i = 0; i < kTileAL; ++i) {
        const int64_t m = int64_t(blockIdx.x) * kTileM + (threadIdx.x >> 3) + 32 * i;
        aval[i] = m < M;
        const int64_t mm = aval[i] ? m : 0;
        const int ox = int(mm % Wo);
        const int64_t tmp = mm / Wo;
        const int oy = int(tmp % Ho);
        abase[i] = (tmp / Ho) * H;
        aiy[i] = oy * stride - pad;
        aix[i] = ox * stride - pad;
    }
    conv_tile<T, BN, false>(                     // never empty: KS * KS >= 1 taps, Cin >= 64 (mla_rn_conv checks both)
        w, KS * KS, Cin, KS * KS, M,
        [&](int i, int tap, int c0) {
            const int ky = tap / KS, kx = tap - ky * KS;
            const int iy = aiy[i] + ky, ix = aix[i] + kx;
            const bool ok = aval[i] && iy >= 0 && iy < H && ix >= 0 && ix < W;
            return ok ? *reinterpret_cast<const u32x4*>(in + ((abase[i] + iy) * W + ix) * Cin + c0) : mma::zero16();
        },
        [](int tap) { return tap; },
        [&](int co) {
            const float sc = scale ? scale[co] : 1.f, sh = scale ? shift[co] : 0.f;
            return [=](int64_t m, float v) {
                const int64_t off = m * Cout + co;
                if (scale) v = v * sc + sh;
                if (res) v += mma::load_elem<T>(res + off);
                if (relu) v = mla::nan_relu(v);
                mma::store_elem<T>(out + off, v);
            };
        });
}

// OIHW f32 -> [O][KH][KW][I] in T
template <typename T>
__global__ void rn_repack_kernel(const float* __restrict__ w, T* __restrict__ out, int64_t cout, int cin, int kk) {
    const int64_t total = cout * kk * cin;
    for (int64_t i = blockIdx.x * int64_t(blockDim.x) + threadIdx.x; i < total; i += int64_t(gridDim.x) * blockDim.x) {
        const int ci = int(i % cin);
        const int64_t tmp = i / cin;
        const int tap = int(tmp % kk);
        const int64_t co = tmp / kk;
        mma::store_elem<T>(out + i, w[(co * cin + ci) * kk + tap]);
    }
}

// ------------------------------------------------------------------------------------------------
// BatchNorm2d statistics: sum x and sum x^2 by (channel group, row slice) with bn_slice_sums (rn_core.h); the finish
// kernels add the slices in slice order.
// ------------------------------------------------------------------------------------------------
template <typename T>
__global__ __launch_bounds__(256) void rn_bn_partial_kernel(const T* __restrict__ x, int64_t rows, int C, double* __restrict__ part) {
    bn_slice_sums(rows, C, part, [&](int64_t off, int, float* a, float* b) {
        load8<T>(x + off, a);
#pragma unroll
        for (int k = 0; k < 8; ++k) b[k] = a[k];
    });
}

// One channel's statistics from its sums over n rows: one expression sequence for the single-process and the two-stage path.
__device__ __forceinline__ void bn_finish_channel(int c, double s, double s2, double n, const float* __restrict__ gamma,
                                                  const float* __restrict__ beta, float eps, float momentum,
                                                  float* __restrict__ running_mean, float* __restrict__ running_var,
                                                  float* __restrict__ mean_out, float* __restrict__ var_out,
                                                  float* __restrict__ scale, float* __restrict__ shift) {
    const double mean = s / n;
    double var = s2 / n - mean * mean;
    if (var < 0.0) var = 0.0;
    const double sc = double(gamma[c]) / sqrt(var + double(eps));
    scale[c] = float(sc);
    shift[c] = float(double(beta[c]) - mean * sc);
    if (mean_out) mean_out[c] = float(mean);
    if (var_out) var_out[c] = float(var);
    if (running_mean) {
        const double unbiased = n > 1.0 ? var * n / (n - 1.0) : var;
        running_mean[c] = float((1.0 - momentum) * running_mean[c] + momentum * mean);
        running_var[c] = float((1.0 - momentum) * running_var[c] + momentum * unbiased);
    }
}

__global__ void rn_bn_finish_kernel(const double* __restrict__ part, int P, int C, int64_t rows, const float* __restrict__ gamma,
                                    const float* __restrict__ beta, float eps, float momentum, float* __restrict__ running_mean,
                                    float* __restrict__ running_var, float* __restrict__ mean_out, float* __restrict__ var_out,
                                    float* __restrict__ scale, float* __restrict__ shift) {
    const int c = blockIdx.x * blockDim.x + threadIdx.x;
    if (c >= C) return;
    double s, s2;
    bn_sum_slices(part, P, C, c, s, s2);
    bn_finish_channel(c, s, s2, double(rows), gamma, beta, eps, momentum, running_mean, running_var, mean_out, var_out, scale, shift);
}

// Stage 1 of the data-parallel statistics: sums = [sum x (C), sum x^2 (C), rows], the message the ranks add up.
__global__ void rn_bn_sums_kernel(const double* __restrict__ part, int P, int C, int64_t rows, double* __restrict__ sums) {
    const int c = blockIdx.x * blockDim.x + threadIdx.x;
    if (c >= C) return;
    double s, s2;
    bn_sum_slices(part, P, C, c, s, s2);
    sums[c] = s;
    sums[C + c] = s2;
    if (c == 0) sums[2 * int64_t(C)] = double(rows);
}

// Stage 2: the statistics of the (all-reduced) sums; the row count is the message's last element.
__global__ void rn_bn_finish_sums_kernel(const double* __restrict__ sums, int C, const float* __restrict__ gamma,
                                         const float* __restrict__ beta, float eps, float momentum, float* __restrict__ running_mean,
                                         float* __restrict__ running_var, float* __restrict__ mean_out, float* __restrict__ var_out,
                                         float* __restrict__ scale, float* __restrict__ shift) {
    const int c = blockIdx.x * blockDim.x + threadIdx.x;
    if (c >= C) return;
    bn_finish_channel(c, sums[c], sums[C + c], sums[2 * int64_t(C)], gamma, beta, eps, momentum, running_mean, running_var, mean_out,
                      var_out, scale, shift);
}

__global__ void rn_bn_eval_kernel(const float* __restrict__ gamma, const float* __restrict__ beta, const float* __restrict__ rm,
                                  const float* __restrict__ rv, float eps, int C, float* __restrict__ scale, float* __restrict__ shift) {
    const int c = blockIdx.x * blockDim.x + threadIdx.x;
    if (c >= C) return;
    const float sc = gamma[c] / sqrtf(rv[c] + eps);
    scale[c] = sc;
    shift[c] = beta[c] - rm[c] * sc;
}

// x and out may be the same buffer (in-place apply): neither is __restrict__
template <typename T>
__global__ __launch_bounds__(256) void rn_bn_apply_kernel(const T* x, int64_t n8, int C, const float* __restrict__ scale,
                                                           const float* __restrict__ shift, const T* __restrict__ res, int relu, T* out) {
    for (int64_t i = blockIdx.x * int64_t(blockDim.x) + threadIdx.x; i < n8; i += int64_t(gridDim.x) * blockDim.x) {
        const int64_t off = i * 8;
        const int c = int(off % C);
        float v[8], r[8];
        load8<T>(x + off, v);
        if (res) load8<T>(res + off, r);
#pragma unroll
        for (int k = 0; k < 8; ++k) {
            v[k] = v[k] * scale[c + k] + shift[c + k];
            if (res) v[k] += r[k];
            if (relu) v[k] = mla::nan_relu(v[k]);
        }
        store8<T>(out + off, v);
    }
}

// MaxPool2d(kernel 3, stride 2, padding 1): one thread per 8 channels of an output pixel
template <typename T>
__global__ __launch_bounds__(256) void rn_maxpool_kernel(const T* __restrict__ in, int64_t n, int H, int W, int C, int Ho, int Wo,
                                                         T* __restrict__ out) {
    const int cg = C / 8;
    const int64_t total = n * Ho * Wo * cg;
    for (int64_t i = blockIdx.x * int64_t(blockDim.x) + threadIdx.x; i < total; i += int64_t(gridDim.x) * blockDim.x) {
        const int c = int(i % cg) * 8;
        int64_t pix = i / cg;
        const int ox = int(pix % Wo);
        const int64_t tmp = pix / Wo;
        const int oy = int(tmp % Ho);
        const int64_t img = tmp / Ho;
        float m[8];
#pragma unroll
        for (int k = 0; k < 8; ++k) m[k] = -INFINITY;
        for (int ky = 0; ky < 3; ++ky) {
            const int iy = 2 * oy - 1 + ky;
            if (iy < 0 || iy >= H) continue;
            for (int kx = 0; kx < 3; ++kx) {
                const int ix = 2 * ox - 1 + kx;
                if (ix < 0 || ix >= W) continue;
                float v[8];
                load8<T>(in + ((img * H + iy) * W + ix) * C + c, v);
#pragma unroll
                for (int k = 0; k < 8; ++k) m[k] = mla::nan_max(m[k], v[k]);
            }
        }
        store8<T>(out + pix * C + c, m);
    }
}

// AdaptiveAvgPool2d(1) + flatten: (n, HW, C) -> f32 (n, C); sum in pixel order
template <typename T>
__global__ __launch_bounds__(256) void rn_avgpool_kernel(const T* __restrict__ in, int64_t n, int HW, int C, float* __restrict__ out) {
    const int64_t total = n * C;
    for (int64_t i = blockIdx.x * int64_t(blockDim.x) + threadIdx.x; i < total; i += int64_t(gridDim.x) * blockDim.x) {
        const int c = int(i % C);
        const int64_t img = i / C;
        float s = 0.f;
        for (int p = 0; p < HW; ++p) s += mma::load_elem<T>(in + (img * HW + p) * C + c);
        out[i] = s / float(HW);
    }
}

}  // namespace

extern "C" int mla_rn_repack(const float* w_oihw, int64_t cout, int64_t cin, int64_t ks, void* out, int dtype, mla_stream_t stream) {
    MLA_REQUIRE(w_oihw && out && cout > 0 && cin > 0 && ks > 0, MLA_E_ARG, "bad rn_repack arguments");
    MLA_REQUIRE(dtype == MLA_F32 || dtype == MLA_BF16, MLA_E_DTYPE, "rn_repack dtype %d", dtype);
    hipStream_t s = static_cast<hipStream_t>(stream);
    const int64_t total = cout * ks * ks * cin;
    rn_dispatch(dtype, [&](auto tag) {
        using T = typename decltype(tag)::type;
        hipLaunchKernelGGL(rn_repack_kernel<T>, dim3(grid_for(total)), dim3(256), 0, s, w_oihw, static_cast<T*>(out), cout, int(cin), int(ks * ks));
    });
    MLA_LAUNCH_OK("rn_repack_kernel");
    return MLA_OK;
}

extern "C" int mla_rn_stem(const float* x, int64_t n, int64_t H, int64_t W, int single, const float* w, const float* scale, const float* shift, int relu,
                           void* out, int dtype, mla_stream_t stream) {
    MLA_REQUIRE(n >= 0 && (single == 0 || single == 1), MLA_E_ARG, "rn_stem n %lld single %d", (long long)n, single);
    MLA_REQUIRE(H == kImg && W == kImg, MLA_E_SHAPE, "rn_stem: images must be %d x %d (got %lld x %lld)", kImg, kImg, (long long)H, (long long)W);
    if (n == 0) return MLA_OK;
    MLA_REQUIRE(x && w && out && (!scale || shift), MLA_E_ARG, "null rn_stem buffers");
    MLA_REQUIRE(dtype == MLA_F32 || dtype == MLA_BF16, MLA_E_DTYPE, "rn_stem dtype %d", dtype);
    MLA_REQUIRE(n * kStemOut <= 0x7fffffffLL, MLA_E_SHAPE, "rn_stem: %lld images exceed the grid", (long long)n);
    hipStream_t s = static_cast<hipStream_t>(stream);
    const dim3 grid(unsigned(n * kStemOut));
    rn_dispatch(dtype, [&](auto tag) {
        using T = typename decltype(tag)::type;
        hipLaunchKernelGGL(rn_stem_kernel<T>, grid, dim3(256), 0, s, x, single, w, scale, shift, relu, static_cast<T*>(out));
    });
    MLA_LAUNCH_OK("rn_stem_kernel");
    return MLA_OK;
}

extern "C" int mla_rn_conv(const void* in, int64_t n, int64_t H, int64_t W, int64_t cin, const void* w_packed, int64_t cout, int64_t ks,
                           int64_t stride, const float* scale, const float* shift, const void* residual, int relu, void* out, int dtype,
                           mla_stream_t stream) {
    MLA_REQUIRE(n >= 0 && H > 0 && W > 0, MLA_E_ARG, "rn_conv n %lld H %lld W %lld", (long long)n, (long long)H, (long long)W);
    RN_CONV_REQUIRE("rn_conv", ks, stride, cin, cout, dtype);
    if (n == 0) return MLA_OK;
    MLA_REQUIRE(in && w_packed && out && (!scale || shift), MLA_E_ARG, "null rn_conv buffers");
    MLA_REQUIRE(mla::aligned(in, 16) && mla::aligned(w_packed, 16), MLA_E_ARG, "rn_conv buffers must be 16-byte aligned");
    const int64_t pad = ks / 2, Ho = (H + 2 * pad - ks) / stride + 1, Wo = (W + 2 * pad - ks) / stride + 1;
    const int64_t M = n * Ho * Wo;
    MLA_REQUIRE(H <= 4096 && W <= 4096 && (M + 127) / 128 <= 0x7fffffffLL, MLA_E_SHAPE, "rn_conv: %lld output pixels", (long long)M);
    hipStream_t s = static_cast<hipStream_t>(stream);
    const bool wide = cout % 128 == 0;
    const dim3 grid(unsigned((M + 127) / 128), unsigned(cout / (wide ? 128 : 64)));
    rn_dispatch(dtype, [&](auto tag) {
        using T = typename decltype(tag)::type;
        hipLaunchKernelGGL((wide ? rn_conv_kernel<T, 128> : rn_conv_kernel<T, 64>), grid, dim3(256), 0, s, static_cast<const T*>(in),
                           static_cast<const T*>(w_packed), static_cast<T*>(out), scale, shift, static_cast<const T*>(residual), relu, M,
                           int(H), int(W), int(cin), int(Ho), int(Wo), int(cout), int(ks), int(stride), int(pad));
    });
    MLA_LAUNCH_OK("rn_conv_kernel");
    return MLA_OK;
}

extern "C" int64_t mla_rn_bn_workspace_bytes(int64_t channels) { return 2 * int64_t(kMaxSlices) * channels * int64_t(sizeof(double)); }

// Checks the arguments of the statistics pass over x and launches rn_bn_partial_kernel into the workspace; returns the slice count P
// through *slices (0 on an error, which is then in mla_last_error).
static int rn_bn_partials(const void* x, int64_t rows, int64_t channels, int dtype, void* workspace, hipStream_t s, int* slices) {
    *slices = 0;
    MLA_REQUIRE(rows > 0 && channels > 0 && channels % 64 == 0 && channels <= 65536 * 64, MLA_E_SHAPE,
                "rn_bn_stats rows %lld channels %lld (channels: multiple of 64)", (long long)rows, (long long)channels);
    MLA_REQUIRE(x && workspace, MLA_E_ARG, "null rn_bn_stats buffers");
    MLA_REQUIRE(mla::aligned(x, 16) && mla::aligned(workspace, 8), MLA_E_ARG, "rn_bn_stats buffers must be 16-byte aligned");
    MLA_REQUIRE(dtype == MLA_F32 || dtype == MLA_BF16, MLA_E_DTYPE, "rn_bn_stats dtype %d", dtype);
    const int P = bn_slices(rows);
    double* part = static_cast<double*>(workspace);
    const dim3 grid(unsigned(channels / 64), unsigned(P));
    rn_dispatch(dtype, [&](auto tag) {
        using T = typename decltype(tag)::type;
        hipLaunchKernelGGL(rn_bn_partial_kernel<T>, grid, dim3(256), 0, s, static_cast<const T*>(x), rows, int(channels), part);
    });
    MLA_LAUNCH_OK("rn_bn_partial_kernel");
    *slices = P;
    return MLA_OK;
}

extern "C" int mla_rn_bn_stats(const void* x, int64_t rows, int64_t channels, int dtype, void* workspace, const float* gamma,
                               const float* beta, float eps, float momentum, float* running_mean, float* running_var, float* mean,
                               float* var_biased, float* scale, float* shift, mla_stream_t stream) {
    MLA_REQUIRE(rows > 0 && channels > 0 && channels % 64 == 0 && channels <= 65536 * 64, MLA_E_SHAPE,
                "rn_bn_stats rows %lld channels %lld (channels: multiple of 64)", (long long)rows, (long long)channels);
    MLA_REQUIRE(x && workspace && gamma && beta && scale && shift && (!running_mean == !running_var), MLA_E_ARG, "null rn_bn_stats buffers");
    hipStream_t s = static_cast<hipStream_t>(stream);
    int P = 0;
    const int rc = rn_bn_partials(x, rows, channels, dtype, workspace, s, &P);
    if (rc != MLA_OK) return rc;
    hipLaunchKernelGGL(rn_bn_finish_kernel, dim3(unsigned((channels + 255) / 256)), dim3(256), 0, s, static_cast<const double*>(workspace),
                       P, int(channels), rows, gamma, beta, eps, momentum, running_mean, running_var, mean, var_biased, scale, shift);
    MLA_LAUNCH_OK("rn_bn_finish_kernel");
    return MLA_OK;
}

extern "C" int mla_rn_bn_sums(const void* x, int64_t rows, int64_t channels, int dtype, void* workspace, double* sums,
                              mla_stream_t stream) {
    MLA_REQUIRE(sums && mla::aligned(sums, 8), MLA_E_ARG, "rn_bn_sums: sums must be a non-null, 8-byte aligned buffer");
    hipStream_t s = static_cast<hipStream_t>(stream);
    int P = 0;
    const int rc = rn_bn_partials(x, rows, channels, dtype, workspace, s, &P);
    if (rc != MLA_OK) return rc;
    hipLaunchKernelGGL(rn_bn_sums_kernel, dim3(unsigned((channels + 255) / 256)), dim3(256), 0, s, static_cast<const double*>(workspace), P,
                       int(channels), rows, sums);
    MLA_LAUNCH_OK("rn_bn_sums_kernel");
    return MLA_OK;
}

extern "C" int mla_rn_bn_finish(const double* sums, int64_t channels, const float* gamma, const float* beta, float eps, float momentum,
                                float* running_mean, float* running_var, float* mean, float* var_biased, float* scale, float* shift,
                                mla_stream_t stream) {
    MLA_REQUIRE(channels > 0 && channels <= 65536 * 64, MLA_E_SHAPE, "rn_bn_finish channels %lld", (long long)channels);
    MLA_REQUIRE(sums && gamma && beta && scale && shift && (!running_mean == !running_var), MLA_E_ARG, "null rn_bn_finish buffers");
    MLA_REQUIRE(mla::aligned(sums, 8), MLA_E_ARG, "rn_bn_finish: sums must be 8-byte aligned");
    hipLaunchKernelGGL(rn_bn_finish_sums_kernel, dim3(unsigned((channels + 255) / 256)), dim3(256), 0, static_cast<hipStream_t>(stream), sums,
                       int(channels), gamma, beta, eps, momentum, running_mean, running_var, mean, var_biased, scale, shift);
    MLA_LAUNCH_OK("rn_bn_finish_sums_kernel");
    return MLA_OK;
}

extern "C" int mla_rn_bn_eval_coeffs(const float* gamma, const float* beta, const float* running_mean, const float* running_var,
                                     float eps, int64_t channels, float* scale, float* shift, mla_stream_t stream) {
    MLA_REQUIRE(gamma && beta && running_mean && running_var && scale && shift && channels > 0, MLA_E_ARG, "bad rn_bn_eval_coeffs arguments");
    hipLaunchKernelGGL(rn_bn_eval_kernel, dim3(unsigned((channels + 255) / 256)), dim3(256), 0, static_cast<hipStream_t>(stream), gamma, beta,
                       running_mean, running_var, eps, int(channels), scale, shift);
    MLA_LAUNCH_OK("rn_bn_eval_kernel");
    return MLA_OK;
}

extern "C" int mla_rn_bn_apply(const void* x, int64_t rows, int64_t channels, const float* scale, const float* shift, const void* residual,
                               int relu, void* out, int dtype, mla_stream_t stream) {
    MLA_REQUIRE(rows >= 0 && channels > 0 && channels % 8 == 0, MLA_E_SHAPE, "rn_bn_apply channels %lld (multiple of 8)", (long long)channels);
    if (rows == 0) return MLA_OK;
    MLA_REQUIRE(x && scale && shift && out, MLA_E_ARG, "null rn_bn_apply buffers");
    MLA_REQUIRE(mla::aligned(x, 16) && mla::aligned(out, 16) && mla::aligned(residual, 16), MLA_E_ARG, "rn_bn_apply buffers must be 16-byte aligned");
    MLA_REQUIRE(dtype == MLA_F32 || dtype == MLA_BF16, MLA_E_DTYPE, "rn_bn_apply dtype %d", dtype);
    hipStream_t s = static_cast<hipStream_t>(stream);
    const int64_t n8 = rows * channels / 8;
    rn_dispatch(dtype, [&](auto tag) {
        using T = typename decltype(tag)::type;
        hipLaunchKernelGGL(rn_bn_apply_kernel<T>, dim3(grid_for(n8)), dim3(256), 0, s, static_cast<const T*>(x), n8, int(channels), scale, shift,
                           static_cast<const T*>(residual), relu, static_cast<T*>(out));
    });
    MLA_LAUNCH_OK("rn_bn_apply_kernel");
    return MLA_OK;
}

extern "C" int mla_rn_maxpool(const void* in, int64_t n, int64_t H, int64_t W, int64_t channels, void* out, int dtype, mla_stream_t stream) {
    MLA_REQUIRE(n >= 0 && H > 0 && W > 0 && channels > 0 && channels % 8 == 0 && H <= 65536 && W <= 65536, MLA_E_SHAPE,
                "rn_maxpool %lld x %lld x %lld", (long long)H, (long long)W, (long long)channels);
    if (n == 0) return MLA_OK;
    MLA_REQUIRE(in && out && mla::aligned(in, 16) && mla::aligned(out, 16), MLA_E_ARG, "rn_maxpool buffers: non-null, 16-byte aligned");
    MLA_REQUIRE(dtype == MLA_F32 || dtype == MLA_BF16, MLA_E_DTYPE, "rn_maxpool dtype %d", dtype);
    const int64_t Ho = (H - 1) / 2 + 1, Wo = (W - 1) / 2 + 1;
    hipStream_t s = static_cast<hipStream_t>(stream);
    const unsigned g = grid_for(n * Ho * Wo * channels / 8);
    rn_dispatch(dtype, [&](auto tag) {
        using T = typename decltype(tag)::type;
        hipLaunchKernelGGL(rn_maxpool_kernel<T>, dim3(g), dim3(256), 0, s, static_cast<const T*>(in), n, int(H), int(W), int(channels), int(Ho),
                           int(Wo), static_cast<T*>(out));
    });
    MLA_LAUNCH_OK("rn_maxpool_kernel");
    return MLA_OK;
}

extern "C" int mla_rn_avgpool(const void* in, int64_t n, int64_t hw, int64_t channels, float* out, int dtype, mla_stream_t stream) {
    MLA_REQUIRE(n >= 0 && hw > 0 && hw <= 65536 && channels > 0 && channels <= 65536, MLA_E_SHAPE, "rn_avgpool hw %lld channels %lld",
                (long long)hw, (long long)channels);
    if (n == 0) return MLA_OK;
    MLA_REQUIRE(in && out, MLA_E_ARG, "null rn_avgpool buffers");
    MLA_REQUIRE(dtype == MLA_F32 || dtype == MLA_BF16, MLA_E_DTYPE, "rn_avgpool dtype %d", dtype);
    hipStream_t s = static_cast<hipStream_t>(stream);
    const unsigned g = grid_for(n * channels);
    rn_dispatch(dtype, [&](auto tag) {
        using T = typename decltype(tag)::type;
        hipLaunchKernelGGL(rn_avgpool_kernel<T>, dim3(g), dim3(256), 0, s, static_cast<const T*>(in), n, int(hw), int(channels), out);
    });
    MLA_LAUNCH_OK("rn_avgpool_kernel");
    return MLA_OK;
}
