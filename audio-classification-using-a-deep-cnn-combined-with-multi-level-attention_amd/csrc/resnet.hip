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
#include "common.h"
#include "mma_core.h"

namespace {

using mma::bf16_t;
using mma::f32x4;
using mma::u32x4;

// ------------------------------------------------------------------------------------------------
// stem: x (N, 224, 224) f32 -> out NHWC (N, 112, 112, 64)
// ------------------------------------------------------------------------------------------------
constexpr int kImg = 224, kStemOut = 112, kStemC = 64;

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
    const float mean[3] = {0.485f, 0.456f, 0.406f}, inv[3] = {1.f / 0.229f, 1.f / 0.224f, 1.f / 0.225f};
    float a[49], b[49];
#pragma unroll
    for (int k = 0; k < 49; ++k) {
        const float w0 = w[(o * 3 + 0) * 49 + k], w1 = w[(o * 3 + 1) * 49 + k], w2 = w[(o * 3 + 2) * 49 + k];
        a[k] = single ? w0 * inv[0] : w0 * inv[0] + w1 * inv[1] + w2 * inv[2];
        b[k] = -(w0 * mean[0] * inv[0] + w1 * mean[1] * inv[1] + w2 * mean[2] * inv[2]);
    }
    __syncthreads();
    const float sc = scale ? scale[o] : 1.f, sh = scale ? shift[o] : 0.f;
    for (int ox = pg; ox < kStemOut; ox += 4) {
        float acc = 0.f;
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
        if (relu) v = fmaxf(v, 0.f);
        mma::store_elem<T>(out + ((n * kStemOut + oy) * kStemOut + ox) * kStemC + o, v);
    }
}

// ------------------------------------------------------------------------------------------------
// implicit-GEMM conv: rows = output pixels (N*Ho*Wo), cols = Cout, K = KS*KS*Cin (tap-major, channel-minor).
// Workgroup tile 128 pixels x BN channels, 4 waves as 2 x 2, one 128-byte LDS row per pixel / weight row per k-block
// (64 bf16 or 32 f32 channels of one tap). The next k-block is loaded into registers while the current one computes.
// ------------------------------------------------------------------------------------------------
template <typename T, int BN>
__global__ __launch_bounds__(256) void rn_conv_kernel(const T* __restrict__ in, const T* __restrict__ w, T* __restrict__ out,
                                                      const float* __restrict__ scale, const float* __restrict__ shift,
                                                      const T* __restrict__ res, int relu, int64_t M, int H, int W, int Cin,
                                                      int Ho, int Wo, int Cout, int KS, int stride, int pad) {
    constexpr int EPC = mma::Elem<T>::kPerChunk, EPR = mma::Elem<T>::kPerRow;
    constexpr int BM = 128, AL = BM * 8 / 256, BL = BN * 8 / 256, TN = BN / 32;
    __shared__ __attribute__((aligned(16))) char lds[(BM + BN) * mma::kRowBytes];
    char* As = lds;
    char* Bs = lds + BM * mma::kRowBytes;
    const int t = threadIdx.x, lane = t & 63, wid = t >> 6, q = t & 7, r0 = t >> 3;
    const int64_t m0 = int64_t(blockIdx.x) * BM;
    const int n0 = blockIdx.y * BN;

    int64_t abase[AL];
    int aiy[AL], aix[AL];
    bool aval[AL];
#pragma unroll
    for (int i = 0; i < AL; ++i) {
        const int64_t m = m0 + r0 + 32 * i;
        aval[i] = m < M;
        const int64_t mm = aval[i] ? m : 0;
        const int ox = int(mm % Wo);
        const int64_t tmp = mm / Wo;
        const int oy = int(tmp % Ho);
        abase[i] = (tmp / Ho) * H;
        aiy[i] = oy * stride - pad;
        aix[i] = ox * stride - pad;
    }
    const int KK = KS * KS, csteps = Cin / EPR, nk = KK * csteps;
    u32x4 ra[AL], rb[BL];
    auto load = [&](int k) {
        const int tap = k / csteps, cs = k - tap * csteps, ky = tap / KS, kx = tap - ky * KS;
        const int c0 = cs * EPR + q * EPC;
#pragma unroll
        for (int i = 0; i < AL; ++i) {
            const int iy = aiy[i] + ky, ix = aix[i] + kx;
            const bool ok = aval[i] && iy >= 0 && iy < H && ix >= 0 && ix < W;
            ra[i] = ok ? *reinterpret_cast<const u32x4*>(in + ((abase[i] + iy) * W + ix) * Cin + c0) : mma::zero16();
        }
#pragma unroll
        for (int j = 0; j < BL; ++j) {
            const int64_t co = n0 + r0 + 32 * j;
            rb[j] = *reinterpret_cast<const u32x4*>(w + (co * KK + tap) * Cin + c0);
        }
    };

    f32x4 acc[4][TN];
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int j = 0; j < TN; ++j) acc[i][j] = f32x4{0.f, 0.f, 0.f, 0.f};

    const int wm = wid & 1, wn = wid >> 1;
    load(0);
    for (int k = 0; k < nk; ++k) {
#pragma unroll
        for (int i = 0; i < AL; ++i) mma::lds_write16(As, mma::tile_off(r0 + 32 * i, q), ra[i]);
#pragma unroll
        for (int j = 0; j < BL; ++j) mma::lds_write16(Bs, mma::tile_off(r0 + 32 * j, q), rb[j]);
        __syncthreads();
        if (k + 1 < nk) load(k + 1);
#pragma unroll
        for (int ks = 0; ks < 2; ++ks) {
            const int ch = ks * 4 + (lane >> 4);
            u32x4 a[4], b[TN];
#pragma unroll
            for (int i = 0; i < 4; ++i) a[i] = mma::lds_read16(As, mma::tile_off(wm * 64 + i * 16 + (lane & 15), ch));
#pragma unroll
            for (int j = 0; j < TN; ++j) b[j] = mma::lds_read16(Bs, mma::tile_off(wn * (BN / 2) + j * 16 + (lane & 15), ch));
#pragma unroll
            for (int i = 0; i < 4; ++i)
#pragma unroll
                for (int j = 0; j < TN; ++j) mma::mma_step<T>(a[i], b[j], acc[i][j]);
        }
        __syncthreads();
    }

#pragma unroll
    for (int j = 0; j < TN; ++j) {
        const int co = n0 + wn * (BN / 2) + j * 16 + (lane & 15);
        const float sc = scale ? scale[co] : 1.f, sh = scale ? shift[co] : 0.f;
#pragma unroll
        for (int i = 0; i < 4; ++i) {
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                const int64_t m = m0 + wm * 64 + i * 16 + 4 * (lane >> 4) + e;
                if (m >= M) continue;
                const int64_t off = m * Cout + co;
                float v = acc[i][j][e];
                if (scale) v = v * sc + sh;
                if (res) v += mma::load_elem<T>(res + off);
                if (relu) v = fmaxf(v, 0.f);
                mma::store_elem<T>(out + off, v);
            }
        }
    }
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
// BatchNorm2d statistics: block (channel group of 64, row slice p). Thread: 8 channels (chunk q) of rows r0, r0+32, ...
// of its slice; sums in double; the 32 row lanes are added in LDS in a fixed order, the P slices by the finish kernel
// in a fixed order -> the same bits on every run for a given shape.
// ------------------------------------------------------------------------------------------------
constexpr int kMaxSlices = 512;

int bn_slices(int64_t rows) {
    const int64_t p = (rows + 2047) / 2048;
    return int(p < 1 ? 1 : (p > kMaxSlices ? kMaxSlices : p));
}

template <typename T>
__device__ __forceinline__ void load8(const T* p, float* v) {
    if constexpr (sizeof(T) == 2) {
        const u32x4 u = *reinterpret_cast<const u32x4*>(p);
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            v[2 * k] = __builtin_bit_cast(float, u[k] << 16);
            v[2 * k + 1] = __builtin_bit_cast(float, u[k] & 0xFFFF0000u);
        }
    } else {
        const f32x4 a = *reinterpret_cast<const f32x4*>(p), b = *reinterpret_cast<const f32x4*>(p + 4);
#pragma unroll
        for (int k = 0; k < 4; ++k) { v[k] = a[k]; v[4 + k] = b[k]; }
    }
}

template <typename T>
__device__ __forceinline__ void store8(T* p, const float* v) {
    if constexpr (sizeof(T) == 2) {
        u32x4 u;
#pragma unroll
        for (int k = 0; k < 4; ++k) u[k] = mma::pack_bf16x2(v[2 * k], v[2 * k + 1]);
        *reinterpret_cast<u32x4*>(p) = u;
    } else {
        *reinterpret_cast<f32x4*>(p) = f32x4{v[0], v[1], v[2], v[3]};
        *reinterpret_cast<f32x4*>(p + 4) = f32x4{v[4], v[5], v[6], v[7]};
    }
}

template <typename T>
__global__ __launch_bounds__(256) void rn_bn_partial_kernel(const T* __restrict__ x, int64_t rows, int C, double* __restrict__ part) {
    __shared__ double red[2][32][64];
    const int t = threadIdx.x, q = t & 7, r0 = t >> 3;
    const int c0 = blockIdx.x * 64 + q * 8, P = gridDim.y, p = blockIdx.y;
    double s[8], s2[8];
#pragma unroll
    for (int k = 0; k < 8; ++k) s[k] = s2[k] = 0.0;
    for (int64_t r = int64_t(p) * 32 + r0; r < rows; r += int64_t(P) * 32) {
        float v[8];
        load8<T>(x + r * C + c0, v);
#pragma unroll
        for (int k = 0; k < 8; ++k) { s[k] += v[k]; s2[k] += double(v[k]) * v[k]; }
    }
#pragma unroll
    for (int k = 0; k < 8; ++k) { red[0][r0][q * 8 + k] = s[k]; red[1][r0][q * 8 + k] = s2[k]; }
    __syncthreads();
    if (t < 128) {
        const int which = t >> 6, c = t & 63;
        double acc = 0.0;
        for (int i = 0; i < 32; ++i) acc += red[which][i][c];
        part[(int64_t(which) * P + p) * C + blockIdx.x * 64 + c] = acc;
    }
}

// The P slices of one channel, added in slice order: the fixed order that rn_bn_finish_kernel and rn_bn_sums_kernel share.
__device__ __forceinline__ void bn_sum_slices(const double* __restrict__ part, int P, int C, int c, double& s, double& s2) {
    s = 0.0;
    s2 = 0.0;
    for (int p = 0; p < P; ++p) { s += part[int64_t(p) * C + c]; s2 += part[int64_t(P + p) * C + c]; }
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
            if (relu) v[k] = fmaxf(v[k], 0.f);
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
                for (int k = 0; k < 8; ++k) m[k] = fmaxf(m[k], v[k]);
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

unsigned grid_for(int64_t work, int64_t cap = 16384) {
    const int64_t g = (work + 255) / 256;
    return unsigned(g < 1 ? 1 : (g > cap ? cap : g));
}

}  // namespace

extern "C" int mla_rn_repack(const float* w_oihw, int64_t cout, int64_t cin, int64_t ks, void* out, int dtype, mla_stream_t stream) {
    MLA_REQUIRE(w_oihw && out && cout > 0 && cin > 0 && ks > 0, MLA_E_ARG, "bad rn_repack arguments");
    MLA_REQUIRE(dtype == MLA_F32 || dtype == MLA_BF16, MLA_E_DTYPE, "rn_repack dtype %d", dtype);
    hipStream_t s = static_cast<hipStream_t>(stream);
    const int64_t total = cout * ks * ks * cin;
    if (dtype == MLA_F32)
        hipLaunchKernelGGL(rn_repack_kernel<float>, dim3(grid_for(total)), dim3(256), 0, s, w_oihw, static_cast<float*>(out), cout, int(cin), int(ks * ks));
    else
        hipLaunchKernelGGL(rn_repack_kernel<bf16_t>, dim3(grid_for(total)), dim3(256), 0, s, w_oihw, static_cast<bf16_t*>(out), cout, int(cin), int(ks * ks));
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
    if (dtype == MLA_F32)
        hipLaunchKernelGGL(rn_stem_kernel<float>, grid, dim3(256), 0, s, x, single, w, scale, shift, relu, static_cast<float*>(out));
    else
        hipLaunchKernelGGL(rn_stem_kernel<bf16_t>, grid, dim3(256), 0, s, x, single, w, scale, shift, relu, static_cast<bf16_t*>(out));
    MLA_LAUNCH_OK("rn_stem_kernel");
    return MLA_OK;
}

extern "C" int mla_rn_conv(const void* in, int64_t n, int64_t H, int64_t W, int64_t cin, const void* w_packed, int64_t cout, int64_t ks,
                           int64_t stride, const float* scale, const float* shift, const void* residual, int relu, void* out, int dtype,
                           mla_stream_t stream) {
    MLA_REQUIRE(n >= 0 && H > 0 && W > 0, MLA_E_ARG, "rn_conv n %lld H %lld W %lld", (long long)n, (long long)H, (long long)W);
    MLA_REQUIRE((ks == 1 || ks == 3) && (stride == 1 || stride == 2), MLA_E_SHAPE, "rn_conv: kernel %lld stride %lld not compiled",
                (long long)ks, (long long)stride);
    MLA_REQUIRE(cin > 0 && cout > 0 && cin % 64 == 0 && cout % 64 == 0 && cin <= 4096 && cout <= 4096, MLA_E_SHAPE,
                "rn_conv: Cin %lld / Cout %lld must be multiples of 64 (<= 4096)", (long long)cin, (long long)cout);
    MLA_REQUIRE(dtype == MLA_F32 || dtype == MLA_BF16, MLA_E_DTYPE, "rn_conv dtype %d", dtype);
    if (n == 0) return MLA_OK;
    MLA_REQUIRE(in && w_packed && out && (!scale || shift), MLA_E_ARG, "null rn_conv buffers");
    MLA_REQUIRE(mla::aligned(in, 16) && mla::aligned(w_packed, 16), MLA_E_ARG, "rn_conv buffers must be 16-byte aligned");
    const int64_t pad = ks / 2, Ho = (H + 2 * pad - ks) / stride + 1, Wo = (W + 2 * pad - ks) / stride + 1;
    const int64_t M = n * Ho * Wo;
    MLA_REQUIRE(H <= 4096 && W <= 4096 && (M + 127) / 128 <= 0x7fffffffLL, MLA_E_SHAPE, "rn_conv: %lld output pixels", (long long)M);
    hipStream_t s = static_cast<hipStream_t>(stream);
    const bool wide = cout % 128 == 0;
    const dim3 grid(unsigned((M + 127) / 128), unsigned(cout / (wide ? 128 : 64)));
#define RN_CONV(T, BN)                                                                                                          \
    hipLaunchKernelGGL((rn_conv_kernel<T, BN>), grid, dim3(256), 0, s, static_cast<const T*>(in), static_cast<const T*>(w_packed), \
                       static_cast<T*>(out), scale, shift, static_cast<const T*>(residual), relu, M, int(H), int(W), int(cin),  \
                       int(Ho), int(Wo), int(cout), int(ks), int(stride), int(pad))
    if (dtype == MLA_F32) {
        if (wide) RN_CONV(float, 128); else RN_CONV(float, 64);
    } else {
        if (wide) RN_CONV(bf16_t, 128); else RN_CONV(bf16_t, 64);
    }
#undef RN_CONV
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
    if (dtype == MLA_F32)
        hipLaunchKernelGGL(rn_bn_partial_kernel<float>, grid, dim3(256), 0, s, static_cast<const float*>(x), rows, int(channels), part);
    else
        hipLaunchKernelGGL(rn_bn_partial_kernel<bf16_t>, grid, dim3(256), 0, s, static_cast<const bf16_t*>(x), rows, int(channels), part);
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
    if (dtype == MLA_F32)
        hipLaunchKernelGGL(rn_bn_apply_kernel<float>, dim3(grid_for(n8)), dim3(256), 0, s, static_cast<const float*>(x), n8, int(channels),
                           scale, shift, static_cast<const float*>(residual), relu, static_cast<float*>(out));
    else
        hipLaunchKernelGGL(rn_bn_apply_kernel<bf16_t>, dim3(grid_for(n8)), dim3(256), 0, s, static_cast<const bf16_t*>(x), n8, int(channels),
                           scale, shift, static_cast<const bf16_t*>(residual), relu, static_cast<bf16_t*>(out));
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
    if (dtype == MLA_F32)
        hipLaunchKernelGGL(rn_maxpool_kernel<float>, dim3(g), dim3(256), 0, s, static_cast<const float*>(in), n, int(H), int(W), int(channels),
                           int(Ho), int(Wo), static_cast<float*>(out));
    else
        hipLaunchKernelGGL(rn_maxpool_kernel<bf16_t>, dim3(g), dim3(256), 0, s, static_cast<const bf16_t*>(in), n, int(H), int(W),
                           int(channels), int(Ho), int(Wo), static_cast<bf16_t*>(out));
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
    if (dtype == MLA_F32)
        hipLaunchKernelGGL(rn_avgpool_kernel<float>, dim3(g), dim3(256), 0, s, static_cast<const float*>(in), n, int(hw), int(channels), out);
    else
        hipLaunchKernelGGL(rn_avgpool_kernel<bf16_t>, dim3(g), dim3(256), 0, s, static_cast<const bf16_t*>(in), n, int(hw), int(channels), out);
    MLA_LAUNCH_OK("rn_avgpool_kernel");
    return MLA_OK;
}
