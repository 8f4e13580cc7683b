// resnet_bwd.hip -- backward of the ResNet-50 v1.5 trunk (cnn_trainable / first_cnn_layer_trainable finetuning,
// model.py:131-136 of the reference). Activations and gradients are NHWC in the compute dtype (f32 or bf16), accumulation
// f32, weight gradients f32 in OIHW. No float atomics, no host synchronisation, caller-owned workspaces, and every
// reduction runs in a fixed order: bit-identical results run to run (and under graph replay). Kernels:
//   rn_repack_dgrad_kernel   OIHW f32 -> [Cin][k][k][Cout] with the taps flipped: the weights of the data gradient
//   rn_dgrad_s2_kernel       data gradient of a stride-2 conv as four parity classes of input pixel; each class gathers
//                            its fixed subset of taps with stride 1 (stride 1 is mla_rn_conv on the repacked weights)
//   rn_wgrad_kernel          weight gradient, a GEMM over the output pixels, split-K with f32 partials reduced in split
//                            order by rn_wgrad_reduce_kernel; both operands go through an LDS transpose
//   rn_stem_wgrad_*          stem weight gradient with the Input normalisation folded in (two sums per output / tap)
//   rn_bn_bwd_*              BatchNorm2d train-mode backward (+ fused ReLU mask, + residual-path gradient); rn_bn_bwd_sums_kernel
//                            / rn_bn_bwd_coef_kernel split it around an all-reduce of [sum g, sum g xhat, rows] (SyncBN
//                            across data-parallel ranks: the batch means of the global batch)
//   rn_act_bwd_kernel        backward of the eval-mode epilogue (BatchNorm folded to scale / shift [+ residual] [ReLU]): mask and scale
//   rn_stem_dgrad_kernel     stem data gradient down to the raw planes, the Input normalisation folded in (rn_stem_dgrad_core.h)
//   rn_maxpool_bwd_kernel    MaxPool2d(3, 2, 1) backward as a gather (first maximum in torch's scan order)
//   rn_avgpool_bwd_kernel    AdaptiveAvgPool2d(1) backward: dY / HW broadcast
#include "rn_core.h"
#include "rn_stem_dgrad_core.h"

namespace {

using namespace rn;
using mma::load8;
using mma::store8;

// ------------------------------------------------------------------------------------------------
// dgrad weights: w (Cout, Cin, k, k) f32 -> out[ci][t][co] = w[co][ci][k*k-1-t] in T
// ------------------------------------------------------------------------------------------------
template <typename T>
__global__ void rn_repack_dgrad_kernel(const float* __restrict__ w, T* __restrict__ out, int cout, int64_t cin, int kk) {
    const int64_t total = cin * kk * cout;
    for (int64_t i = blockIdx.x * int64_t(blockDim.x) + threadIdx.x; i < total; i += int64_t(gridDim.x) * blockDim.x) {
        const int co = int(i % cout);
        const int64_t tmp = i / cout;
        const int t = int(tmp % kk);
        const int64_t ci = tmp / kk;
        mma::store_elem<T>(out + i, w[(co * cin + ci) * kk + (kk - 1 - t)]);
    }
}

// ------------------------------------------------------------------------------------------------
// stride-2 data gradient. Forward: y[oy] = sum_ky x[2 oy - pad + ky] w[ky]. An input row iy = 2a + py receives the taps
// ky = ky0 + 2j (ky0 = (py + pad) & 1) from the output row oy = a + (py + pad - ky) / 2; so each of the four parity classes
// (py, px) is a stride-1 gather over the output grid with its own tap subset (no zero taps reach the matrix cores).
// Rows = the class's input pixels, cols = Cin, K = class taps x Cout, on the tile of rn_conv_kernel (rn_core.h conv_tile).
// A class without taps (odd positions of a 1x1/2 downsample) writes the residual alone.
// ------------------------------------------------------------------------------------------------
template <typename T, int BN>
__global__ __launch_bounds__(256) void rn_dgrad_s2_kernel(const T* __restrict__ dy, const T* __restrict__ wd, const T* __restrict__ res,
                                                          T* __restrict__ out, int64_t Mc, int Ho, int Wo, int Cout, int H, int W,
                                                          int Cin, int KS, int pad) {
    const int py = blockIdx.z >> 1, px = blockIdx.z & 1;
    const int Hc = H / 2, Wc = W / 2;
    const int ky0 = (py + pad) & 1, kx0 = (px + pad) & 1;
    const int nty = (KS - ky0 + 1) / 2, ntx = (KS - kx0 + 1) / 2;

    int64_t abase[kTileAL];
    int aa[kTileAL], ab[kTileAL];
    bool aval[kTileAL];
#pragma unroll
    for (int i = 0; i < kTileAL; ++i) {
        const int64_t m = int64_t(blockIdx.x) * kTileM + (threadIdx.x >> 3) + 32 * i;
        aval[i] = m < Mc;
        const int64_t mm = aval[i] ? m : 0;
        ab[i] = int(mm % Wc);
        const int64_t tmp = mm / Wc;
        aa[i] = int(tmp % Hc);
        abase[i] = (tmp / Hc) * Ho;
    }
    auto taps = [&](int tap, int& ky, int& kx) {
        const int jy = tap / ntx, jx = tap - jy * ntx;
        ky = ky0 + 2 * jy;
        kx = kx0 + 2 * jx;
    };
    conv_tile<T, BN, true>(
        wd, KS * KS, Cout, nty * ntx, Mc,
        [&](int i, int tap, int c0) {
            int ky, kx;
            taps(tap, ky, kx);
            const int oy = aa[i] + (py + pad - ky) / 2, ox = ab[i] + (px + pad - kx) / 2;
            const bool ok = aval[i] && oy >= 0 && oy < Ho && ox >= 0 && ox < Wo;
            return ok ? *reinterpret_cast<const u32x4*>(dy + ((abase[i] + oy) * Wo + ox) * Cout + c0) : mma::zero16();
        },
        [&](int tap) {
            int ky, kx;
            taps(tap, ky, kx);
            return (KS - 1 - ky) * KS + (KS - 1 - kx);       // the flipped tap of the dgrad repack
        },
        [&](int ci) {
            return [=](int64_t m, float v) {
                const int b = int(m % Wc);
                const int64_t tmp = m / Wc;
                const int a = int(tmp % Hc);
                const int64_t img = tmp / Hc;
                const int64_t off = ((img * H + 2 * a + py) * W + 2 * b + px) * Cin + ci;
                if (res) v += mma::load_elem<T>(res + off);
                mma::store_elem<T>(out + off, v);
            };
        });
}

// ------------------------------------------------------------------------------------------------
// weight gradient: dW[co][tap][ci] = sum_p dy[p][co] * x_tap[p][ci], p over the output pixels of this split.
// Workgroup tile 64 co x 64 ci of one tap, 4 waves as 2 x 2 (32 x 32 each). Per k-block of EPR pixels both operands are
// loaded pixel-major (16 B = EPC channels of one pixel) and written TRANSPOSED into the 128-byte LDS rows the MFMA
// fragments read (one row per channel, the pixels along it).
// ------------------------------------------------------------------------------------------------
template <typename T>
__global__ __launch_bounds__(256) void rn_wgrad_kernel(const T* __restrict__ x, const T* __restrict__ dy, float* __restrict__ ws,
                                                       int64_t P, int64_t kb_per, int H, int W, int Cin, int Ho, int Wo, int Cout,
                                                       int KS, int stride, int pad) {
    constexpr int EPC = mma::Elem<T>::kPerChunk, EPR = mma::Elem<T>::kPerRow;
    constexpr int CPP = 64 / EPC;                       // 16-byte chunks per pixel of a 64-channel slab
    constexpr int LPT = EPR * CPP / 256;                // chunks per thread and operand per k-block (2)
    __shared__ __attribute__((aligned(16))) char lds[2 * 64 * mma::kRowBytes];
    char* As = lds;
    char* Bs = lds + 64 * mma::kRowBytes;
    const int t = threadIdx.x, lane = t & 63, wid = t >> 6;
    const int KK = KS * KS;
    const int co0 = blockIdx.x * 64;
    const int tap = int(blockIdx.y % KK), ci0 = int(blockIdx.y / KK) * 64;
    const int ky = tap / KS, kx = tap - ky * KS;
    const int64_t s = blockIdx.z;
    const int64_t p_begin = s * kb_per * EPR;
    int64_t p_end = p_begin + kb_per * EPR;
    if (p_end > P) p_end = P;
    const int64_t nkb = (p_end - p_begin + EPR - 1) / EPR;

    u32x4 ra[LPT], rb[LPT];
    auto load = [&](int64_t kb) {
#pragma unroll
        for (int l = 0; l < LPT; ++l) {
            const int idx = t + 256 * l, px = idx / CPP, cc = idx - px * CPP;
            const int64_t p = p_begin + kb * EPR + px;
            ra[l] = mma::zero16();
            rb[l] = mma::zero16();
            if (p < p_end) {
                ra[l] = *reinterpret_cast<const u32x4*>(dy + p * Cout + co0 + cc * EPC);
                const int ox = int(p % Wo);
                const int64_t tmp = p / Wo;
                const int oy = int(tmp % Ho);
                const int64_t img = tmp / Ho;
                const int iy = oy * stride - pad + ky, ix = ox * stride - pad + kx;
                if (iy >= 0 && iy < H && ix >= 0 && ix < W)
                    rb[l] = *reinterpret_cast<const u32x4*>(x + ((img * H + iy) * W + ix) * Cin + ci0 + cc * EPC);
            }
        }
    };
    auto put = [&](char* base, int px, int cc, const u32x4& v) {
        // element e of the chunk is channel cc*EPC + e = the LDS row; the pixel px is the K position along that row
        const int chunk = px / EPC, within = (px - chunk * EPC) * int(sizeof(T));
        if constexpr (sizeof(T) == 2) {
#pragma unroll
            for (int e = 0; e < EPC; ++e) {
                const uint16_t h = uint16_t((e & 1) ? (v[e >> 1] >> 16) : (v[e >> 1] & 0xFFFFu));
                *reinterpret_cast<uint16_t*>(base + mma::tile_off(cc * EPC + e, chunk) + within) = h;
            }
        } else {
#pragma unroll
            for (int e = 0; e < EPC; ++e) *reinterpret_cast<uint32_t*>(base + mma::tile_off(cc * EPC + e, chunk) + within) = v[e];
        }
    };

    f32x4 acc[2][2];
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int j = 0; j < 2; ++j) acc[i][j] = f32x4{0.f, 0.f, 0.f, 0.f};
    const int wm = wid & 1, wn = wid >> 1;
    if (nkb > 0) load(0);
    for (int64_t kb = 0; kb < nkb; ++kb) {
#pragma unroll
        for (int l = 0; l < LPT; ++l) {
            const int idx = t + 256 * l, px = idx / CPP, cc = idx - px * CPP;
            put(As, px, cc, ra[l]);
            put(Bs, px, cc, rb[l]);
        }
        __syncthreads();
        if (kb + 1 < nkb) load(kb + 1);
#pragma unroll
        for (int ks = 0; ks < 2; ++ks) {
            const int ch = ks * 4 + (lane >> 4);
            u32x4 a[2], b[2];
#pragma unroll
            for (int i = 0; i < 2; ++i) a[i] = mma::lds_read16(As, mma::tile_off(wm * 32 + i * 16 + (lane & 15), ch));
#pragma unroll
            for (int j = 0; j < 2; ++j) b[j] = mma::lds_read16(Bs, mma::tile_off(wn * 32 + j * 16 + (lane & 15), ch));
#pragma unroll
            for (int i = 0; i < 2; ++i)
#pragma unroll
                for (int j = 0; j < 2; ++j) mma::mma_step<T>(a[i], b[j], acc[i][j]);
        }
        __syncthreads();
    }
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int j = 0; j < 2; ++j)
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                const int co = co0 + wm * 32 + i * 16 + 4 * (lane >> 4) + e;
                const int ci = ci0 + wn * 32 + j * 16 + (lane & 15);
                ws[((s * Cout + co) * KK + tap) * Cin + ci] = acc[i][j][e];
            }
}

// dw (Cout, Cin, k, k) = sum over the splits, in split order, of ws[s][co][tap][ci]
__global__ void rn_wgrad_reduce_kernel(const float* __restrict__ ws, int S, int Cout, int Cin, int KK, float* __restrict__ dw) {
    const int64_t plane = int64_t(Cout) * Cin * KK;
    for (int64_t i = blockIdx.x * int64_t(blockDim.x) + threadIdx.x; i < plane; i += int64_t(gridDim.x) * blockDim.x) {
        const int ci = int(i % Cin);
        const int64_t tmp = i / Cin;
        const int tap = int(tmp % KK);
        const int64_t co = tmp / KK;
        float acc = 0.f;
        for (int s = 0; s < S; ++s) acc += ws[s * plane + i];
        dw[(co * Cin + ci) * KK + tap] = acc;
    }
}

// ------------------------------------------------------------------------------------------------
// stem weight gradient. The forward folds the Input normalisation into the taps (resnet.hip rn_stem_kernel): inside the
// image the normalised channel c is inv_c (x [c carries x] - mean_c), outside it is 0. So per (o, tap) two sums over the
// output pixels whose tap falls inside the image -- S1 = sum dY x, S0 = sum dY -- give
// dW[o][c][tap] = inv_c ([c carries x] S1 - mean_c S0). Block: `rpb` consecutive output rows (image, oy); thread: output
// channel o = t & 63 at every 4th column; the four column groups are added in LDS in a fixed order, the blocks' partials
// by the finish kernel in block order (double).
// ------------------------------------------------------------------------------------------------
template <typename T>
__global__ __launch_bounds__(256) void rn_stem_wgrad_partial_kernel(const float* __restrict__ x, const T* __restrict__ dy,
                                                                    int64_t rows, int rpb, float* __restrict__ part) {
    __shared__ float xs[7][kImg];
    __shared__ float red[4][kStemC][49];
    const int t = threadIdx.x, o = t & 63, pg = t >> 6;
    float s1[49], s0[49];
#pragma unroll
    for (int k = 0; k < 49; ++k) s1[k] = s0[k] = 0.f;
    const int64_t r_begin = int64_t(blockIdx.x) * rpb;
    const int64_t r_end = r_begin + rpb < rows ? r_begin + rpb : rows;
    for (int64_t r = r_begin; r < r_end; ++r) {
        const int oy = int(r % kStemOut);
        const int64_t n = r / kStemOut;
        __syncthreads();
        for (int i = t; i < 7 * kImg; i += 256) {
            const int ky = i / kImg, ix = i - ky * kImg, iy = 2 * oy - 3 + ky;
            xs[ky][ix] = (iy >= 0 && iy < kImg) ? x[(n * kImg + iy) * kImg + ix] : 0.f;
        }
        __syncthreads();
        for (int ox = pg; ox < kStemOut; ox += 4) {
            const float d = mma::load_elem<T>(dy + (r * kStemOut + ox) * kStemC + o);
#pragma unroll
            for (int ky = 0; ky < 7; ++ky) {
                const int iy = 2 * oy - 3 + ky;
                if (iy < 0 || iy >= kImg) continue;
#pragma unroll
                for (int kx = 0; kx < 7; ++kx) {
                    const int ix = 2 * ox - 3 + kx;
                    if (ix >= 0 && ix < kImg) {
                        s1[ky * 7 + kx] += d * xs[ky][ix];
                        s0[ky * 7 + kx] += d;
                    }
                }
            }
        }
    }
#pragma unroll
    for (int which = 0; which < 2; ++which) {
        __syncthreads();
#pragma unroll
        for (int k = 0; k < 49; ++k) red[pg][o][k] = which ? s0[k] : s1[k];
        __syncthreads();
        for (int i = t; i < kStemC * 49; i += 256) {
            const int oo = i / 49, k = i - oo * 49;
            const float v = ((red[0][oo][k] + red[1][oo][k]) + red[2][oo][k]) + red[3][oo][k];
            part[((int64_t(blockIdx.x) * kStemC + oo) * 49 + k) * 2 + which] = v;
        }
    }
}

__global__ void rn_stem_wgrad_finish_kernel(const float* __restrict__ part, int S, int single, float* __restrict__ dw) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;       // (o, tap)
    if (i >= kStemC * 49) return;
    const int o = i / 49, k = i - o * 49;
    double s1 = 0.0, s0 = 0.0;
    for (int s = 0; s < S; ++s) {
        s1 += part[(int64_t(s) * kStemC * 49 + i) * 2];
        s0 += part[(int64_t(s) * kStemC * 49 + i) * 2 + 1];
    }
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        const double carry = (c == 0 || !single) ? 1.0 : 0.0;
        dw[(o * 3 + c) * 49 + k] = float(double(kNormInv[c]) * (carry * s1 - double(kNormMean[c]) * s0));
    }
}

// ------------------------------------------------------------------------------------------------
// BatchNorm2d backward (train mode). g = dy [* (y > 0)]; xhat = (x - mean) * invstd;
// dx = gamma invstd (g - mean(g) - xhat mean(g xhat)); dgamma = sum g xhat, dbeta = sum g.
// Sums in double by (channel group, row slice) with bn_slice_sums, the slices added by bn_sum_slices (rn_core.h).
// ------------------------------------------------------------------------------------------------
template <typename T>
__device__ __forceinline__ void bn_bwd_elems(const T* x, const T* dy, const T* y, const float* mean, const float* invstd, int c,
                                             float* g, float* xh) {
    float xv[8], m[8];
    load8<T>(x, xv);
    load8<T>(dy, g);
    if (y) {
        load8<T>(y, m);
#pragma unroll
        for (int k = 0; k < 8; ++k) g[k] = m[k] > 0.f ? g[k] : 0.f;
    }
#pragma unroll
    for (int k = 0; k < 8; ++k) xh[k] = (xv[k] - mean[c + k]) * invstd[c + k];
}

// one definition of 1 / sqrt(var + eps): rn_bn_bwd_invstd_kernel and stage 2's rn_bn_bwd_coef_kernel give the same bits
__device__ __forceinline__ float bn_bwd_invstd(float var, float eps) { return float(1.0 / sqrt(double(var) + double(eps))); }

__global__ void rn_bn_bwd_invstd_kernel(const float* __restrict__ var, float eps, int C, float* __restrict__ invstd) {
    const int c = blockIdx.x * blockDim.x + threadIdx.x;
    if (c < C) invstd[c] = bn_bwd_invstd(var[c], eps);
}

template <typename T>
__global__ __launch_bounds__(256) void rn_bn_bwd_partial_kernel(const T* __restrict__ x, const T* __restrict__ dy, const T* __restrict__ y,
                                                                const float* __restrict__ mean, const float* __restrict__ invstd,
                                                                int64_t rows, int C, double* __restrict__ part) {
    bn_slice_sums(rows, C, part, [&](int64_t off, int c0, float* g, float* xh) {
        bn_bwd_elems<T>(x + off, dy + off, y ? y + off : nullptr, mean, invstd, c0, g, xh);
    });
}

// What the fused and the split (SyncBN) backward share per channel. bn_bwd_local: the local sums in slice order, dgamma / dbeta
// from them if requested. bn_bwd_coefs: coef[c] = mean(g), coef[C + c] = mean(g xhat), coef[2C + c] = gamma invstd, the means
// over `count` rows (the local rows, or the global batch's after an all-reduce of the sums).
__device__ __forceinline__ void bn_bwd_local(const double* __restrict__ part, int P, int C, int c, float* __restrict__ dgamma,
                                             float* __restrict__ dbeta, double& s, double& s2) {
    bn_sum_slices(part, P, C, c, s, s2);
    if (dgamma) dgamma[c] = float(s2);
    if (dbeta) dbeta[c] = float(s);
}

__device__ __forceinline__ void bn_bwd_coefs(int C, int c, double s, double s2, double count, float gamma, float invstd,
                                             float* __restrict__ coef) {
    coef[c] = float(s / count);
    coef[C + c] = float(s2 / count);
    coef[2 * C + c] = gamma * invstd;
}

__global__ void rn_bn_bwd_finish_kernel(const double* __restrict__ part, int P, int C, int64_t rows, const float* __restrict__ gamma,
                                        const float* __restrict__ invstd, float* __restrict__ coef, float* __restrict__ dgamma,
                                        float* __restrict__ dbeta) {
    const int c = blockIdx.x * blockDim.x + threadIdx.x;
    if (c >= C) return;
    double s, s2;
    bn_bwd_local(part, P, C, c, dgamma, dbeta, s, s2);
    bn_bwd_coefs(C, c, s, s2, double(rows), gamma[c], invstd[c], coef);
}

// Stage 1 of the split: sums = [sum g (C), sum g xhat (C), rows], the message of the all-reduce. dgamma / dbeta are this
// rank's part (the gradient all-reduce adds the ranks' parts), so they are written here, from the LOCAL sums.
__global__ void rn_bn_bwd_sums_kernel(const double* __restrict__ part, int P, int C, int64_t rows, double* __restrict__ sums,
                                      float* __restrict__ dgamma, float* __restrict__ dbeta) {
    const int c = blockIdx.x * blockDim.x + threadIdx.x;
    if (c >= C) return;
    double s, s2;
    bn_bwd_local(part, P, C, c, dgamma, dbeta, s, s2);
    sums[c] = s;
    sums[C + c] = s2;
    if (c == 0) sums[2 * int64_t(C)] = double(rows);
}

// Stage 2: invstd (recomputed: nothing has to survive in the workspace from stage 1) and the coefficients from the
// (all-reduced) sums; the row count is the message's last element. A count that is not > 0 (a message that did not come from
// stage 1 on every rank) cannot be refused on the host without a device-to-host copy: the coefficients become NaN, so that
// every dx element is NaN instead of a plausible wrong number.
__global__ void rn_bn_bwd_coef_kernel(const double* __restrict__ sums, int C, const float* __restrict__ var, float eps,
                                      const float* __restrict__ gamma, float* __restrict__ invstd, float* __restrict__ coef) {
    const int c = blockIdx.x * blockDim.x + threadIdx.x;
    if (c >= C) return;
    const float is = bn_bwd_invstd(var[c], eps);
    invstd[c] = is;
    const double count = sums[2 * int64_t(C)];
    if (count > 0.0) {
        bn_bwd_coefs(C, c, sums[c], sums[C + c], count, gamma[c], is, coef);
    } else {
        coef[c] = coef[C + c] = coef[2 * C + c] = __builtin_nanf("");
    }
}

template <typename T>
__global__ __launch_bounds__(256) void rn_bn_bwd_apply_kernel(const T* __restrict__ x, const T* __restrict__ dy, const T* __restrict__ y,
                                                              const float* __restrict__ mean, const float* __restrict__ invstd,
                                                              const float* __restrict__ coef, int64_t n8, int C, T* __restrict__ dx,
                                                              T* __restrict__ dres) {
    for (int64_t i = blockIdx.x * int64_t(blockDim.x) + threadIdx.x; i < n8; i += int64_t(gridDim.x) * blockDim.x) {
        const int64_t off = i * 8;
        const int c = int(off % C);
        float g[8], xh[8], v[8];
        bn_bwd_elems<T>(x + off, dy + off, y ? y + off : nullptr, mean, invstd, c, g, xh);
#pragma unroll
        for (int k = 0; k < 8; ++k) v[k] = coef[2 * C + c + k] * (g[k] - coef[c + k] - xh[k] * coef[C + c + k]);
        store8<T>(dx + off, v);
        if (dres) store8<T>(dres + off, g);
    }
}

// ------------------------------------------------------------------------------------------------
// MaxPool2d(3, 2, 1) backward as a gather: input pixel (iy, ix) lies in the windows oy in [iy/2, (iy+1)/2], ox likewise
// (at most 4). For each, the window's argmax is recomputed in torch's scan order (ky-major, strict >, padding never
// chosen) and the pixel takes dY where it is that argmax. Windows are visited in (oy, ox) order.
// ------------------------------------------------------------------------------------------------
template <typename T>
__global__ __launch_bounds__(256) void rn_maxpool_bwd_kernel(const T* __restrict__ in, const T* __restrict__ dy, int64_t n, int H, int W,
                                                             int C, int Ho, int Wo, T* __restrict__ dx) {
    const int cg = C / 8;
    const int64_t total = n * H * W * cg;
    for (int64_t i = blockIdx.x * int64_t(blockDim.x) + threadIdx.x; i < total; i += int64_t(gridDim.x) * blockDim.x) {
        const int c = int(i % cg) * 8;
        const int64_t pix = i / cg;
        const int ix = int(pix % W);
        const int64_t tmp = pix / W;
        const int iy = int(tmp % H);
        const int64_t img = tmp / H;
        float acc[8];
#pragma unroll
        for (int k = 0; k < 8; ++k) acc[k] = 0.f;
        const int oy_hi = (iy + 1) / 2 < Ho - 1 ? (iy + 1) / 2 : Ho - 1, ox_hi = (ix + 1) / 2 < Wo - 1 ? (ix + 1) / 2 : Wo - 1;
        for (int oy = iy / 2; oy <= oy_hi; ++oy) {
            for (int ox = ix / 2; ox <= ox_hi; ++ox) {
                float best[8];
                int arg[8];
#pragma unroll
                for (int k = 0; k < 8; ++k) { best[k] = -INFINITY; arg[k] = -1; }
                for (int ky = 0; ky < 3; ++ky) {
                    const int yy = 2 * oy - 1 + ky;
                    if (yy < 0 || yy >= H) continue;
                    for (int kx = 0; kx < 3; ++kx) {
                        const int xx = 2 * ox - 1 + kx;
                        if (xx < 0 || xx >= W) continue;
                        float v[8];
                        load8<T>(in + ((img * H + yy) * W + xx) * C + c, v);
#pragma unroll
                        for (int k = 0; k < 8; ++k)
                            if (v[k] > best[k] || arg[k] < 0) { best[k] = v[k]; arg[k] = yy * W + xx; }
                    }
                }
                float d[8];
                load8<T>(dy + ((img * Ho + oy) * Wo + ox) * C + c, d);
#pragma unroll
                for (int k = 0; k < 8; ++k)
                    if (arg[k] == iy * W + ix) acc[k] += d[k];
            }
        }
        store8<T>(dx + pix * C + c, acc);
    }
}

// AdaptiveAvgPool2d(1) backward: dx (n, hw, C) = d (n, C) f32 / hw
template <typename T>
__global__ __launch_bounds__(256) void rn_avgpool_bwd_kernel(const float* __restrict__ d, int64_t n, int hw, int C, T* __restrict__ dx) {
    const int64_t total = n * hw * C / 8;
    for (int64_t i = blockIdx.x * int64_t(blockDim.x) + threadIdx.x; i < total; i += int64_t(gridDim.x) * blockDim.x) {
        const int64_t off = i * 8;
        const int c = int(off % C);
        const int64_t img = off / (int64_t(hw) * C);
        float v[8];
#pragma unroll
        for (int k = 0; k < 8; ++k) v[k] = d[img * C + c + k] / float(hw);
        store8<T>(dx + off, v);
    }
}

// ------------------------------------------------------------------------------------------------
// backward of the eval-mode epilogue y = [relu](conv * scale + shift [+ residual]) over NHWC rows: the BatchNorm is a
// per-channel constant there, so its backward is a mask and a scale. g = dy [* (y > 0)] (NaN in y gives 0, as torch's
// threshold_backward); dpre = g * scale[c], the gradient of the conv output; dres (or null) = g, the residual's gradient.
// ------------------------------------------------------------------------------------------------
template <typename T>
__global__ __launch_bounds__(256) void rn_act_bwd_kernel(const T* __restrict__ dy, const T* __restrict__ y, const float* __restrict__ scale,
                                                         int64_t n8, int C, T* __restrict__ dpre, T* __restrict__ dres) {
    for (int64_t i = blockIdx.x * int64_t(blockDim.x) + threadIdx.x; i < n8; i += int64_t(gridDim.x) * blockDim.x) {
        const int64_t off = i * 8;
        const int c = int(off % C);
        float g[8], v[8];
        load8<T>(dy + off, g);
        if (y) {
            float m[8];
            load8<T>(y + off, m);
#pragma unroll
            for (int k = 0; k < 8; ++k) g[k] = m[k] > 0.f ? g[k] : 0.f;
        }
#pragma unroll
        for (int k = 0; k < 8; ++k) v[k] = g[k] * scale[c + k];
        store8<T>(dpre + off, v);
        if (dres) store8<T>(dres + off, g);
    }
}

// ------------------------------------------------------------------------------------------------
// stem data gradient: dy (n, 112, 112, 64) [behind the eval epilogue: y, scale] -> dx (n, 224, 224) f32 of the RAW planes, the
// Input normalisation and channel configuration folded into the taps as the forward folds them. Persistent workgroups, item =
// (image, 8 input rows); tiling, tap map and the gather are rn_stem_dgrad_core.h, which csrc/rn_stem_dgrad_hostsim.cpp runs on
// the host. Every dx element is summed by one lane in a fixed order and stored once: no atomics, no workspace.
// ------------------------------------------------------------------------------------------------
namespace sd = rn_stem_dgrad;
static_assert(sd::kImg == kImg && sd::kOut == kStemOut && sd::kC == kStemC && sd::kInv[0] == kNormInv[0] && sd::kInv[1] == kNormInv[1] &&
                  sd::kInv[2] == kNormInv[2],
              "rn_stem_dgrad_core.h restates the stem geometry of rn_core.h");

template <typename T>
__global__ __launch_bounds__(sd::kThreads) void rn_stem_dgrad_kernel(const T* __restrict__ dy, const T* __restrict__ y,
                                                                     const float* __restrict__ scale, const float* __restrict__ w,
                                                                     int single, int64_t n_items, float* __restrict__ dx) {
    __shared__ __attribute__((aligned(16))) float sA[sd::kTaps * sd::kC];
    __shared__ __attribute__((aligned(16))) float sG[sd::kSlots * sd::kOut * sd::kGroup];
    const int t = threadIdx.x;
    for (int i = t; i < sd::kC * sd::kTaps; i += sd::kThreads) {
        const int o = i / sd::kTaps, tap = i - o * sd::kTaps;
        sA[sd::a_index(o, tap)] = sd::fold_a(w[sd::w_index(o, 0, tap)], w[sd::w_index(o, 1, tap)], w[sd::w_index(o, 2, tap)], single);
    }                                                            // made visible by the first pass's barrier

    for (int64_t item = blockIdx.x; item < n_items; item += gridDim.x) {
        const int64_t n = item / sd::kTiles;
        const int tile = int(item % sd::kTiles);
        float acc[sd::kPixPerLane];
#pragma unroll
        for (int j = 0; j < sd::kPixPerLane; ++j) acc[j] = 0.f;

        for (int grp = 0; grp < sd::kGroups; ++grp) {
            // ---- stage g of the tile's 7 output rows, 16 channels
            for (int i = t; i < sd::kStageLoads; i += sd::kThreads) {
                int r, ox, c8;
                sd::stage_of(i, &r, &ox, &c8);
                const int oy = sd::slot_row(tile, r);
                float g[8];
#pragma unroll
                for (int k = 0; k < 8; ++k) g[k] = 0.f;
                if (sd::row_live(oy)) {
                    const int c = grp * sd::kGroup + c8;
                    const int64_t off = sd::g_index(n, oy, ox) + c;
                    load8<T>(dy + off, g);
                    if (y) {
                        float m[8];
                        load8<T>(y + off, m);
#pragma unroll
                        for (int k = 0; k < 8; ++k) g[k] = sd::route(g[k], m[k], scale[c + k], true);
                    }
                }
                float* dst = sG + sd::s_index(r, ox) + c8;
                *reinterpret_cast<f32x4*>(dst) = f32x4{g[0], g[1], g[2], g[3]};
                *reinterpret_cast<f32x4*>(dst + 4) = f32x4{g[4], g[5], g[6], g[7]};
            }
            __syncthreads();
            // ---- gather: each pixel from its 3 or 4 x 3 or 4 output positions
#pragma unroll
            for (int j = 0; j < sd::kPixPerLane; ++j) {
                int row, ix, ky0, nty, fy, kx0, ntx, fx;
                sd::pixel_of(t + sd::kThreads * j, &row, &ix);
                sd::axis_taps(row, &ky0, &nty, &fy);
                sd::axis_taps(ix, &kx0, &ntx, &fx);
                for (int jy = 0; jy < nty; ++jy) {
                    const int r = fy - jy + 1;                   // slot of output row 4 tile + fy - jy
                    if (!sd::row_live(sd::slot_row(tile, r))) continue;
                    for (int jx = 0; jx < ntx; ++jx) {
                        const int ox = fx - jx;
                        if (ox < 0 || ox >= sd::kOut) continue;
                        const int tap = (ky0 + 2 * jy) * 7 + kx0 + 2 * jx;
                        float gv[sd::kGroup], av[sd::kGroup];
#pragma unroll
                        for (int k = 0; k < sd::kGroup / 4; ++k) {
                            const f32x4 q = *reinterpret_cast<const f32x4*>(sG + sd::s_index(r, ox) + 4 * k);
                            const f32x4 a = *reinterpret_cast<const f32x4*>(sA + sd::a_index(grp * sd::kGroup, tap) + 4 * k);
#pragma unroll
                            for (int e = 0; e < 4; ++e) {
                                gv[4 * k + e] = q[e];
                                av[4 * k + e] = a[e];
                            }
                        }
                        acc[j] = sd::gather(acc[j], gv, av);
                    }
                }
            }
            __syncthreads();                                     // the next pass (or item) overwrites sG
        }
#pragma unroll
        for (int j = 0; j < sd::kPixPerLane; ++j) {
            int row, ix;
            sd::pixel_of(t + sd::kThreads * j, &row, &ix);
            dx[(n * sd::kImg + tile * sd::kTileRows + row) * sd::kImg + ix] = acc[j];
        }
    }
}

// wgrad split count: enough workgroups to fill the GPU, a function of the shape only (never of the data or the launch)
struct WgradPlan {
    int64_t kb_per;
    int S;
};

WgradPlan wgrad_plan(int64_t P, int64_t cin, int64_t cout, int64_t ks, int dtype) {
    const int64_t epr = dtype == MLA_BF16 ? 64 : 32;
    const int64_t tiles = (cout / 64) * (cin / 64) * ks * ks;
    const int64_t kblocks = (P + epr - 1) / epr;
    int64_t S = (2048 + tiles - 1) / tiles;
    if (S > kblocks) S = kblocks;
    if (S < 1) S = 1;
    const int64_t kb_per = (kblocks + S - 1) / S;
    return {kb_per, int((kblocks + kb_per - 1) / kb_per)};
}

int64_t stem_rows_per_block(int64_t rows) { return (rows + 1023) / 1024; }

}  // namespace

extern "C" int mla_rn_repack_dgrad(const float* w_oihw, int64_t cout, int64_t cin, int64_t ks, void* out, int dtype, mla_stream_t stream) {
    MLA_REQUIRE(w_oihw && out && cout > 0 && cin > 0 && ks > 0 && cout <= 65536, MLA_E_ARG, "bad rn_repack_dgrad arguments");
    MLA_REQUIRE(dtype == MLA_F32 || dtype == MLA_BF16, MLA_E_DTYPE, "rn_repack_dgrad dtype %d", dtype);
    hipStream_t s = static_cast<hipStream_t>(stream);
    const int64_t total = cout * ks * ks * cin;
    rn_dispatch(dtype, [&](auto tag) {
        using T = typename decltype(tag)::type;
        hipLaunchKernelGGL(rn_repack_dgrad_kernel<T>, dim3(grid_for(total)), dim3(256), 0, s, w_oihw, static_cast<T*>(out), int(cout), cin,
                           int(ks * ks));
    });
    MLA_LAUNCH_OK("rn_repack_dgrad_kernel");
    return MLA_OK;
}

extern "C" int mla_rn_conv_dgrad(const void* dy, int64_t n, int64_t Ho, int64_t Wo, int64_t cout, const void* w_dgrad, int64_t cin, int64_t ks,
                                 int64_t stride, int64_t H, int64_t W, const void* residual, void* dx, int dtype, mla_stream_t stream) {
    RN_CONV_REQUIRE("rn_conv_dgrad", ks, stride, cin, cout, dtype);
    if (stride == 1) {
        MLA_REQUIRE(H == Ho && W == Wo, MLA_E_SHAPE, "rn_conv_dgrad: stride 1 keeps the size (%lld x %lld vs %lld x %lld)", (long long)H,
                    (long long)W, (long long)Ho, (long long)Wo);
        return mla_rn_conv(dy, n, Ho, Wo, cout, w_dgrad, cin, ks, 1, nullptr, nullptr, residual, 0, dx, dtype, stream);
    }
    MLA_REQUIRE(n >= 0 && Ho > 0 && Wo > 0 && H == 2 * Ho && W == 2 * Wo && H <= 4096 && W <= 4096, MLA_E_SHAPE,
                "rn_conv_dgrad stride 2: input %lld x %lld must be twice the output %lld x %lld", (long long)H, (long long)W, (long long)Ho,
                (long long)Wo);
    if (n == 0) return MLA_OK;
    MLA_REQUIRE(dy && w_dgrad && dx, MLA_E_ARG, "null rn_conv_dgrad buffers");
    MLA_REQUIRE(mla::aligned(dy, 16) && mla::aligned(w_dgrad, 16), MLA_E_ARG, "rn_conv_dgrad buffers must be 16-byte aligned");
    const int64_t Mc = n * Ho * Wo;                   // pixels of one parity class
    MLA_REQUIRE((Mc + 127) / 128 <= 0x7fffffffLL, MLA_E_SHAPE, "rn_conv_dgrad: %lld pixels", (long long)Mc);
    hipStream_t s = static_cast<hipStream_t>(stream);
    const bool wide = cin % 128 == 0;
    const dim3 grid(unsigned((Mc + 127) / 128), unsigned(cin / (wide ? 128 : 64)), 4);
    rn_dispatch(dtype, [&](auto tag) {
        using T = typename decltype(tag)::type;
        hipLaunchKernelGGL((wide ? rn_dgrad_s2_kernel<T, 128> : rn_dgrad_s2_kernel<T, 64>), grid, dim3(256), 0, s, static_cast<const T*>(dy),
                           static_cast<const T*>(w_dgrad), static_cast<const T*>(residual), static_cast<T*>(dx), Mc, int(Ho), int(Wo), int(cout),
                           int(H), int(W), int(cin), int(ks), int(ks / 2));
    });
    MLA_LAUNCH_OK("rn_dgrad_s2_kernel");
    return MLA_OK;
}

extern "C" int64_t mla_rn_conv_wgrad_workspace_floats(int64_t n, int64_t Ho, int64_t Wo, int64_t cin, int64_t cout, int64_t ks, int dtype) {
    if (n <= 0 || Ho <= 0 || Wo <= 0 || cin <= 0 || cout <= 0 || ks <= 0) return 0;
    const WgradPlan pl = wgrad_plan(n * Ho * Wo, cin, cout, ks, dtype);
    return int64_t(pl.S) * cout * cin * ks * ks;
}

extern "C" int mla_rn_conv_wgrad(const void* x, const void* dy, int64_t n, int64_t H, int64_t W, int64_t cin, int64_t cout, int64_t ks,
                                 int64_t stride, float* workspace, int64_t workspace_floats, float* dw_oihw, int dtype, mla_stream_t stream) {
    MLA_REQUIRE(n > 0 && H > 0 && W > 0 && H <= 4096 && W <= 4096, MLA_E_SHAPE, "rn_conv_wgrad n %lld H %lld W %lld", (long long)n,
                (long long)H, (long long)W);
    RN_CONV_REQUIRE("rn_conv_wgrad", ks, stride, cin, cout, dtype);
    MLA_REQUIRE(x && dy && workspace && dw_oihw, MLA_E_ARG, "null rn_conv_wgrad buffers");
    MLA_REQUIRE(mla::aligned(x, 16) && mla::aligned(dy, 16), MLA_E_ARG, "rn_conv_wgrad buffers must be 16-byte aligned");
    const int64_t pad = ks / 2, Ho = (H + 2 * pad - ks) / stride + 1, Wo = (W + 2 * pad - ks) / stride + 1;
    const int64_t need = mla_rn_conv_wgrad_workspace_floats(n, Ho, Wo, cin, cout, ks, dtype);
    MLA_REQUIRE(workspace_floats >= need, MLA_E_ARG, "rn_conv_wgrad workspace: %lld floats, need %lld", (long long)workspace_floats,
                (long long)need);
    const WgradPlan pl = wgrad_plan(n * Ho * Wo, cin, cout, ks, dtype);
    hipStream_t s = static_cast<hipStream_t>(stream);
    const dim3 grid(unsigned(cout / 64), unsigned((cin / 64) * ks * ks), unsigned(pl.S));
    rn_dispatch(dtype, [&](auto tag) {
        using T = typename decltype(tag)::type;
        hipLaunchKernelGGL(rn_wgrad_kernel<T>, grid, dim3(256), 0, s, static_cast<const T*>(x), static_cast<const T*>(dy), workspace, n * Ho * Wo,
                           pl.kb_per, int(H), int(W), int(cin), int(Ho), int(Wo), int(cout), int(ks), int(stride), int(pad));
    });
    MLA_LAUNCH_OK("rn_wgrad_kernel");
    hipLaunchKernelGGL(rn_wgrad_reduce_kernel, dim3(grid_for(cout * cin * ks * ks)), dim3(256), 0, s, workspace, pl.S, int(cout), int(cin),
                       int(ks * ks), dw_oihw);
    MLA_LAUNCH_OK("rn_wgrad_reduce_kernel");
    return MLA_OK;
}

extern "C" int64_t mla_rn_stem_wgrad_workspace_floats(int64_t n) {
    if (n <= 0) return 0;
    const int64_t rows = n * kStemOut, rpb = stem_rows_per_block(rows);
    return (rows + rpb - 1) / rpb * kStemC * 49 * 2;
}

extern "C" int mla_rn_stem_wgrad(const float* x, int64_t n, int single, const void* dy, float* workspace, int64_t workspace_floats, float* dw,
                                 int dtype, mla_stream_t stream) {
    MLA_REQUIRE(n > 0 && n * kStemOut <= 0x7fffffffLL && (single == 0 || single == 1), MLA_E_ARG, "rn_stem_wgrad n %lld single %d",
                (long long)n, single);
    MLA_REQUIRE(x && dy && workspace && dw, MLA_E_ARG, "null rn_stem_wgrad buffers");
    MLA_REQUIRE(dtype == MLA_F32 || dtype == MLA_BF16, MLA_E_DTYPE, "rn_stem_wgrad dtype %d", dtype);
    MLA_REQUIRE(workspace_floats >= mla_rn_stem_wgrad_workspace_floats(n), MLA_E_ARG, "rn_stem_wgrad workspace: %lld floats, need %lld",
                (long long)workspace_floats, (long long)mla_rn_stem_wgrad_workspace_floats(n));
    const int64_t rows = n * kStemOut, rpb = stem_rows_per_block(rows);
    const int S = int((rows + rpb - 1) / rpb);
    hipStream_t s = static_cast<hipStream_t>(stream);
    rn_dispatch(dtype, [&](auto tag) {
        using T = typename decltype(tag)::type;
        hipLaunchKernelGGL(rn_stem_wgrad_partial_kernel<T>, dim3(S), dim3(256), 0, s, x, static_cast<const T*>(dy), rows, int(rpb), workspace);
    });
    MLA_LAUNCH_OK("rn_stem_wgrad_partial_kernel");
    hipLaunchKernelGGL(rn_stem_wgrad_finish_kernel, dim3((kStemC * 49 + 255) / 256), dim3(256), 0, s, workspace, S, single, dw);
    MLA_LAUNCH_OK("rn_stem_wgrad_finish_kernel");
    return MLA_OK;
}

extern "C" int64_t mla_rn_bn_bwd_workspace_bytes(int64_t channels) {
    return 2 * int64_t(kMaxSlices) * channels * int64_t(sizeof(double)) + 4 * channels * int64_t(sizeof(float));
}

namespace {

// The workspace of mla_rn_bn_bwd_workspace_bytes: [slice partials: 2 kMaxSlices C doubles][invstd: C floats][coef: 3 C floats].
struct BnBwdWs {
    double* part;
    float* invstd;
    float* coef;
    BnBwdWs(void* workspace, int64_t channels)
        : part(static_cast<double*>(workspace)), invstd(reinterpret_cast<float*>(part + 2 * int64_t(kMaxSlices) * channels)),
          coef(invstd + channels) {}
};

// The argument checks of the three entry points; `others` / `others_aligned`: what the caller found for its own buffers
// (gamma, sums, dx, dres), folded in so that the order of the checks is shape, NULL, alignment, dtype for each of them.
int bn_bwd_check(const char* who, const void* x, const void* dy, const void* y, int64_t rows, int64_t channels, const float* mean,
                 const float* var, const void* workspace, bool others, bool others_aligned, int dtype) {
    MLA_REQUIRE(rows > 0 && channels > 0 && channels % 64 == 0 && channels <= 65536 * 64, MLA_E_SHAPE,
                "%s rows %lld channels %lld (channels: multiple of 64)", who, (long long)rows, (long long)channels);
    MLA_REQUIRE(x && dy && mean && var && workspace && others, MLA_E_ARG, "null %s buffers", who);
    MLA_REQUIRE(mla::aligned(x, 16) && mla::aligned(dy, 16) && mla::aligned(y, 16) && mla::aligned(workspace, 8) && others_aligned, MLA_E_ARG,
                "%s buffers must be 16-byte aligned (sums: 8-byte)", who);
    MLA_REQUIRE(dtype == MLA_F32 || dtype == MLA_BF16, MLA_E_DTYPE, "%s dtype %d", who, dtype);
    return MLA_OK;
}

// invstd and the slice partials of (g, g xhat): the first half of the fused call and of stage 1
int bn_bwd_partials(const void* x, const void* dy, const void* y, int64_t rows, int64_t channels, const float* mean, const float* var,
                    float eps, const BnBwdWs& ws, int dtype, hipStream_t s, int* slices) {
    const int P = bn_slices(rows);
    const int C = int(channels);
    hipLaunchKernelGGL(rn_bn_bwd_invstd_kernel, dim3(unsigned((channels + 255) / 256)), dim3(256), 0, s, var, eps, C, ws.invstd);
    MLA_LAUNCH_OK("rn_bn_bwd_invstd_kernel");
    const dim3 grid(unsigned(channels / 64), unsigned(P));
    rn_dispatch(dtype, [&](auto tag) {
        using T = typename decltype(tag)::type;
        hipLaunchKernelGGL(rn_bn_bwd_partial_kernel<T>, grid, dim3(256), 0, s, static_cast<const T*>(x), static_cast<const T*>(dy),
                           static_cast<const T*>(y), mean, ws.invstd, rows, C, ws.part);
    });
    MLA_LAUNCH_OK("rn_bn_bwd_partial_kernel");
    *slices = P;
    return MLA_OK;
}

// dx (and dres) from ws.invstd / ws.coef: the second half of the fused call and of stage 2
int bn_bwd_elementwise(const void* x, const void* dy, const void* y, int64_t rows, int64_t channels, const float* mean, const BnBwdWs& ws,
                       void* dx, void* dres, int dtype, hipStream_t s) {
    const int64_t n8 = rows * channels / 8;
    rn_dispatch(dtype, [&](auto tag) {
        using T = typename decltype(tag)::type;
        hipLaunchKernelGGL(rn_bn_bwd_apply_kernel<T>, dim3(grid_for(n8)), dim3(256), 0, s, static_cast<const T*>(x), static_cast<const T*>(dy),
                           static_cast<const T*>(y), mean, ws.invstd, ws.coef, n8, int(channels), static_cast<T*>(dx), static_cast<T*>(dres));
    });
    MLA_LAUNCH_OK("rn_bn_bwd_apply_kernel");
    return MLA_OK;
}

}  // namespace

extern "C" int mla_rn_bn_bwd(const void* x, const void* dy, const void* y, int64_t rows, int64_t channels, const float* mean, const float* var,
                             const float* gamma, float eps, void* workspace, float* dgamma, float* dbeta, void* dx, void* dres, int dtype,
                             mla_stream_t stream) {
    int rc = bn_bwd_check("rn_bn_bwd", x, dy, y, rows, channels, mean, var, workspace, gamma && dx,
                          mla::aligned(dx, 16) && mla::aligned(dres, 16), dtype);
    if (rc != MLA_OK) return rc;
    hipStream_t s = static_cast<hipStream_t>(stream);
    const BnBwdWs ws(workspace, channels);
    int P = 0;
    if ((rc = bn_bwd_partials(x, dy, y, rows, channels, mean, var, eps, ws, dtype, s, &P)) != MLA_OK) return rc;
    hipLaunchKernelGGL(rn_bn_bwd_finish_kernel, dim3(unsigned((channels + 255) / 256)), dim3(256), 0, s, ws.part, P, int(channels), rows,
                       gamma, ws.invstd, ws.coef, dgamma, dbeta);
    MLA_LAUNCH_OK("rn_bn_bwd_finish_kernel");
    return bn_bwd_elementwise(x, dy, y, rows, channels, mean, ws, dx, dres, dtype, s);
}

extern "C" int mla_rn_bn_bwd_sums(const void* x, const void* dy, const void* y, int64_t rows, int64_t channels, const float* mean,
                                  const float* var, float eps, void* workspace, double* sums, float* dgamma, float* dbeta, int dtype,
                                  mla_stream_t stream) {
    int rc = bn_bwd_check("rn_bn_bwd_sums", x, dy, y, rows, channels, mean, var, workspace, sums != nullptr, mla::aligned(sums, 8), dtype);
    if (rc != MLA_OK) return rc;
    hipStream_t s = static_cast<hipStream_t>(stream);
    const BnBwdWs ws(workspace, channels);
    int P = 0;
    if ((rc = bn_bwd_partials(x, dy, y, rows, channels, mean, var, eps, ws, dtype, s, &P)) != MLA_OK) return rc;
    hipLaunchKernelGGL(rn_bn_bwd_sums_kernel, dim3(unsigned((channels + 255) / 256)), dim3(256), 0, s, ws.part, P, int(channels), rows, sums,
                       dgamma, dbeta);
    MLA_LAUNCH_OK("rn_bn_bwd_sums_kernel");
    return MLA_OK;
}

extern "C" int mla_rn_bn_bwd_apply(const void* x, const void* dy, const void* y, int64_t rows, int64_t channels, const float* mean,
                                   const float* var, const float* gamma, float eps, const double* sums, void* workspace, void* dx, void* dres,
                                   int dtype, mla_stream_t stream) {
    const int rc = bn_bwd_check("rn_bn_bwd_apply", x, dy, y, rows, channels, mean, var, workspace, gamma && sums && dx,
                                mla::aligned(sums, 8) && mla::aligned(dx, 16) && mla::aligned(dres, 16), dtype);
    if (rc != MLA_OK) return rc;
    hipStream_t s = static_cast<hipStream_t>(stream);
    const BnBwdWs ws(workspace, channels);
    const int C = int(channels);
    const dim3 per_channel(unsigned((channels + 255) / 256));
    hipLaunchKernelGGL(rn_bn_bwd_coef_kernel, per_channel, dim3(256), 0, s, sums, C, var, eps, gamma, ws.invstd, ws.coef);
    MLA_LAUNCH_OK("rn_bn_bwd_coef_kernel");
    return bn_bwd_elementwise(x, dy, y, rows, channels, mean, ws, dx, dres, dtype, s);
}

extern "C" int mla_rn_maxpool_bwd(const void* in, const void* dy, int64_t n, int64_t H, int64_t W, int64_t channels, void* dx, int dtype,
                                  mla_stream_t stream) {
    MLA_REQUIRE(n >= 0 && H > 0 && W > 0 && channels > 0 && channels % 8 == 0 && H <= 65536 && W <= 65536, MLA_E_SHAPE,
                "rn_maxpool_bwd %lld x %lld x %lld", (long long)H, (long long)W, (long long)channels);
    if (n == 0) return MLA_OK;
    MLA_REQUIRE(in && dy && dx && mla::aligned(in, 16) && mla::aligned(dy, 16) && mla::aligned(dx, 16), MLA_E_ARG,
                "rn_maxpool_bwd buffers: non-null, 16-byte aligned");
    MLA_REQUIRE(dtype == MLA_F32 || dtype == MLA_BF16, MLA_E_DTYPE, "rn_maxpool_bwd dtype %d", dtype);
    const int64_t Ho = (H - 1) / 2 + 1, Wo = (W - 1) / 2 + 1;
    hipStream_t s = static_cast<hipStream_t>(stream);
    const unsigned g = grid_for(n * H * W * channels / 8);
    rn_dispatch(dtype, [&](auto tag) {
        using T = typename decltype(tag)::type;
        hipLaunchKernelGGL(rn_maxpool_bwd_kernel<T>, dim3(g), dim3(256), 0, s, static_cast<const T*>(in), static_cast<const T*>(dy), n, int(H),
                           int(W), int(channels), int(Ho), int(Wo), static_cast<T*>(dx));
    });
    MLA_LAUNCH_OK("rn_maxpool_bwd_kernel");
    return MLA_OK;
}

extern "C" int mla_rn_avgpool_bwd(const float* d, int64_t n, int64_t hw, int64_t channels, void* dx, int dtype, mla_stream_t stream) {
    MLA_REQUIRE(n >= 0 && hw > 0 && hw <= 65536 && channels > 0 && channels % 8 == 0, MLA_E_SHAPE, "rn_avgpool_bwd hw %lld channels %lld",
                (long long)hw, (long long)channels);
    if (n == 0) return MLA_OK;
    MLA_REQUIRE(d && dx && mla::aligned(dx, 16), MLA_E_ARG, "rn_avgpool_bwd buffers: non-null, 16-byte aligned output");
    MLA_REQUIRE(dtype == MLA_F32 || dtype == MLA_BF16, MLA_E_DTYPE, "rn_avgpool_bwd dtype %d", dtype);
    hipStream_t s = static_cast<hipStream_t>(stream);
    const unsigned g = grid_for(n * hw * channels / 8);
    rn_dispatch(dtype, [&](auto tag) {
        using T = typename decltype(tag)::type;
        hipLaunchKernelGGL(rn_avgpool_bwd_kernel<T>, dim3(g), dim3(256), 0, s, d, n, int(hw), int(channels), static_cast<T*>(dx));
    });
    MLA_LAUNCH_OK("rn_avgpool_bwd_kernel");
    return MLA_OK;
}

extern "C" int mla_rn_act_bwd(const void* dy, const void* y, const float* scale, int64_t rows, int64_t channels, void* dpre, void* dres, int dtype,
                              mla_stream_t stream) {
    MLA_REQUIRE(rows >= 0 && channels > 0 && channels % 8 == 0 && channels <= 65536, MLA_E_SHAPE,
                "rn_act_bwd rows %lld channels %lld (channels: multiple of 8)", (long long)rows, (long long)channels);
    MLA_REQUIRE(dtype == MLA_F32 || dtype == MLA_BF16, MLA_E_DTYPE, "rn_act_bwd dtype %d", dtype);
    if (rows == 0) return MLA_OK;
    MLA_REQUIRE(dy && scale && dpre, MLA_E_ARG, "null rn_act_bwd buffers");
    MLA_REQUIRE(mla::aligned(dy, 16) && mla::aligned(y, 16) && mla::aligned(dpre, 16) && mla::aligned(dres, 16), MLA_E_ARG,
                "rn_act_bwd buffers must be 16-byte aligned");
    MLA_REQUIRE(rows <= (int64_t(1) << 40) / channels, MLA_E_SHAPE, "rn_act_bwd: %lld rows are too many for one launch", (long long)rows);
    hipStream_t s = static_cast<hipStream_t>(stream);
    const int64_t n8 = rows * channels / 8;
    rn_dispatch(dtype, [&](auto tag) {
        using T = typename decltype(tag)::type;
        hipLaunchKernelGGL(rn_act_bwd_kernel<T>, dim3(grid_for(n8)), dim3(256), 0, s, static_cast<const T*>(dy), static_cast<const T*>(y), scale,
                           n8, int(channels), static_cast<T*>(dpre), static_cast<T*>(dres));
    });
    MLA_LAUNCH_OK("rn_act_bwd_kernel");
    return MLA_OK;
}

extern "C" int mla_rn_stem_dgrad(const void* dy, int64_t n, const void* y, const float* scale, const float* w, int single, float* dx, int dtype,
                                 mla_stream_t stream) {
    MLA_REQUIRE(n >= 0 && (single == 0 || single == 1), MLA_E_ARG, "bad rn_stem_dgrad arguments: n = %lld, single = %d", (long long)n, single);
    MLA_REQUIRE(dtype == MLA_F32 || dtype == MLA_BF16, MLA_E_DTYPE, "rn_stem_dgrad dtype %d (f32 or bf16)", dtype);
    MLA_REQUIRE((y == nullptr) == (scale == nullptr), MLA_E_ARG, "rn_stem_dgrad: y and scale come together (both, or neither)");
    if (n == 0) return MLA_OK;
    MLA_REQUIRE(dy && w && dx, MLA_E_ARG, "bad rn_stem_dgrad arguments: null pointer");
    MLA_REQUIRE(n <= (int64_t(1) << 32), MLA_E_SHAPE, "rn_stem_dgrad: %lld images are too many for one launch", (long long)n);
    MLA_REQUIRE(mla::aligned(dy, 16) && mla::aligned(y, 16), MLA_E_ARG, "rn_stem_dgrad: dy and y must be 16-byte aligned");
    hipStream_t s = static_cast<hipStream_t>(stream);
    rn_dispatch(dtype, [&](auto tag) {
        using T = typename decltype(tag)::type;
        hipLaunchKernelGGL(rn_stem_dgrad_kernel<T>, dim3(sd::grid_of(n)), dim3(sd::kThreads), 0, s, static_cast<const T*>(dy),
                           static_cast<const T*>(y), scale, w, single, sd::items_of(n), dx);
    });
    MLA_LAUNCH_OK("rn_stem_dgrad_kernel");
    return MLA_OK;
}
