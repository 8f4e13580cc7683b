// conv1_dgrad.hip -- gradient of the fused conv1 + ReLU + 2x2 max-pool layer (vggish.py:108-110, Cin = 1) with respect to its INPUT:
// the last link of the chain that carries a class score's gradient down to the log-mel examples (Ensemble.saliency). The conv2 ..
// conv6 data gradients are mla_conv3x3 with flipped weights; this layer recomputes itself, as its weight gradient (conv1_bwd, cnn_train.hip)
// does, because the forward keeps nothing of it.
//
//   conv1_dgrad<TD>       x (n, 96, 64) f32, w (64, 1, 3, 3), bias (64), d_pooled (n, 48, 32, 64) f32 or bf16 -> dx (n, 96, 64) f32.
//                         Persistent workgroups, item = (clip, 12 input rows): phase 1 recomputes the 8 x 32 pooled windows that touch
//                         the tile (lane = window) and leaves per (window, channel) the routed gradient and a one-byte position code
//                         in LDS, phase 2 gathers them per input pixel (lane = 3 pixels); 64 channels in four passes of 16.
//                         Tiling, codes and the gather are conv1_dgrad_core.h, which csrc/conv1_dgrad_hostsim.cpp runs on the host.
//                         bf16 d_pooled: x and w are rounded to bf16 for the recompute, as the bf16 forward rounds them.
//
// Deterministic without atomics or a workspace: each dx element is summed by one lane in a fixed order and stored once.
// Per clip: reads 24 KB of x (1.33x with the halo rows) and 384 KB (f32) / 192 KB (bf16) of d_pooled (1.33x), writes 24 KB;
// 1.33 * 48 * 32 * 64 * 36 recompute FMAs and 96 * 64 * 4 * 64 code tests, of which 9 in 16 are FMAs.
#include "cnn_train_core.h"
#include "conv1_dgrad_core.h"

namespace {

using namespace ct;
namespace cd = conv1_dgrad;

constexpr int kGPitch = cd::kGroup + 4;                          // floats per window row of sG: 80 B, 16-byte reads of 8 windows hit 8 bank quads

template <typename TD>
__global__ __launch_bounds__(cd::kThreads) void conv1_dgrad_kernel(const float* __restrict__ x, const float* __restrict__ w,
                                                                   const float* __restrict__ bias, const TD* __restrict__ d_pooled,
                                                                   int64_t n_items, float* __restrict__ dx) {
    constexpr bool LP = sizeof(TD) == 2;
    __shared__ float sW[cd::kC * cd::kWPitch];
    __shared__ __attribute__((aligned(16))) float sG[cd::kWins * kGPitch];
    __shared__ __attribute__((aligned(16))) uint32_t sC[cd::kWins * (cd::kGroup / 4)];
    const int t = threadIdx.x;
    for (int i = t; i < cd::kC * cd::kWPitch; i += cd::kThreads) {
        const int ch = i / cd::kWPitch, k = i % cd::kWPitch;
        const float v = k < 9 ? w[ch * 9 + k] : 0.f;
        sW[i] = LP ? cd::round_bf16(v) : v;
    }
    __syncthreads();

    const int r = t / cd::kPW, wx = t % cd::kPW;                 // phase 1: this lane's window slot
    int prow[cd::kPixPerLane], pix[cd::kPixPerLane], pr0[cd::kPixPerLane], pwx0[cd::kPixPerLane];       // phase 2: its pixels
    uint32_t taps[cd::kPixPerLane][4];
    _Pragma("unroll") for (int j = 0; j < cd::kPixPerLane; ++j) {
        cd::pixel_windows(t + cd::kThreads * j, &prow[j], &pix[j], &pr0[j], &pwx0[j]);
        _Pragma("unroll") for (int s = 0; s < 4; ++s) taps[j][s] = cd::tap_word(prow[j], pr0[j] + (s >> 1), pix[j], pwx0[j] + (s & 1));
    }

    for (int64_t item = blockIdx.x; item < n_items; item += gridDim.x) {
        const int64_t n = item / cd::kTiles;
        const int tile = int(item % cd::kTiles);
        const int wy = cd::window_row(tile, r);
        const bool live = cd::window_live(wy);
        float patch[4][4];
        _Pragma("unroll") for (int a = 0; a < 4; ++a)
            _Pragma("unroll") for (int b = 0; b < 4; ++b) {
                const int64_t at = live ? cd::patch_index(n, wy, wx, a, b) : -1;
                const float v = at >= 0 ? x[at] : 0.f;
                patch[a][b] = LP ? cd::round_bf16(v) : v;
            }
        float acc[cd::kPixPerLane];
        _Pragma("unroll") for (int j = 0; j < cd::kPixPerLane; ++j) acc[j] = 0.f;

        for (int grp = 0; grp < cd::kGroups; ++grp) {
            // ---- phase 1: routed gradient and code of this lane's window, 16 channels
            float g[cd::kGroup];
            uint32_t cw[cd::kGroup / 4] = {0u, 0u, 0u, 0u};
            if (live) {
                const TD* dp = d_pooled + cd::d_index(n, wy, wx) + grp * cd::kGroup;
                load8(dp, g);
                load8(dp + 8, g + 8);
            }
            _Pragma("unroll") for (int c = 0; c < cd::kGroup; ++c) {
                const int ch = grp * cd::kGroup + c;
                const int code = live ? cd::window_code(patch, sW + ch * cd::kWPitch, bias[ch]) : cd::kOff;
                if (code == cd::kOff) g[c] = 0.f;
                cw[c >> 2] |= uint32_t(code) << (8 * (c & 3));
            }
            _Pragma("unroll") for (int k = 0; k < cd::kGroup / 4; ++k)
                *reinterpret_cast<f32x4*>(sG + t * kGPitch + 4 * k) = f32x4{g[4 * k], g[4 * k + 1], g[4 * k + 2], g[4 * k + 3]};
            *reinterpret_cast<u32x4*>(sC + t * (cd::kGroup / 4)) = u32x4{cw[0], cw[1], cw[2], cw[3]};
            __syncthreads();
            // ---- phase 2: each pixel gathers from its 2 x 2 windows
            _Pragma("unroll") for (int j = 0; j < cd::kPixPerLane; ++j) {
                _Pragma("unroll") for (int s = 0; s < 4; ++s) {
                    const int rs = pr0[j] + (s >> 1), ws = pwx0[j] + (s & 1);
                    if (ws < 0 || ws >= cd::kPW) continue;       // left of column 0 / right of column 63: no such window
                    const int slot = rs * cd::kPW + ws;
                    const u32x4 cq = *reinterpret_cast<const u32x4*>(sC + slot * (cd::kGroup / 4));
                    uint8_t codes[cd::kGroup];
                    float gv[cd::kGroup];
                    _Pragma("unroll") for (int k = 0; k < cd::kGroup / 4; ++k) {
                        const f32x4 q = *reinterpret_cast<const f32x4*>(sG + slot * kGPitch + 4 * k);
                        _Pragma("unroll") for (int e = 0; e < 4; ++e) {
                            gv[4 * k + e] = q[e];
                            codes[4 * k + e] = uint8_t((cq[k] >> (8 * e)) & 0xffu);
                        }
                    }
                    acc[j] = cd::gather(acc[j], codes, gv, sW + grp * cd::kGroup * cd::kWPitch, taps[j][s]);
                }
            }
            __syncthreads();                                     // the next pass (or item) overwrites sG / sC
        }
        _Pragma("unroll") for (int j = 0; j < cd::kPixPerLane; ++j)
            dx[(n * cd::kH + tile * cd::kTileRows + prow[j]) * cd::kW + pix[j]] = acc[j];
    }
}

template <typename TD>
int launch_conv1_dgrad(const float* x, const float* w, const float* bias, const TD* d_pooled, int64_t n, float* dx, hipStream_t s) {
    hipLaunchKernelGGL(conv1_dgrad_kernel<TD>, dim3(cd::grid_of(n)), dim3(cd::kThreads), 0, s, x, w, bias, d_pooled, cd::items_of(n), dx);
    MLA_LAUNCH_OK("conv1_dgrad");
    return MLA_OK;
}

}  // namespace

extern "C" int mla_conv1_dgrad(const float* x, const float* w, const float* bias, const void* d_pooled, int d_dtype, int64_t n, float* dx,
                               mla_stream_t stream) {
    MLA_REQUIRE(n >= 0, MLA_E_ARG, "bad conv1_dgrad arguments: n = %lld", (long long)n);
    MLA_REQUIRE(d_dtype == MLA_F32 || d_dtype == MLA_BF16, MLA_E_DTYPE, "conv1_dgrad: d_pooled dtype %d (f32 or bf16)", d_dtype);
    if (n == 0) return MLA_OK;
    MLA_REQUIRE(x && w && bias && d_pooled && dx, MLA_E_ARG, "bad conv1_dgrad arguments: null pointer");
    MLA_REQUIRE(n <= (int64_t(1) << 40), MLA_E_SHAPE, "conv1_dgrad: %lld clips are too many for one launch", (long long)n);
    MLA_REQUIRE(mla::aligned(d_pooled, 16), MLA_E_ARG, "conv1_dgrad: d_pooled must be 16-byte aligned");
    hipStream_t s = static_cast<hipStream_t>(stream);
    if (d_dtype == MLA_BF16) return launch_conv1_dgrad(x, w, bias, static_cast<const bf16_t*>(d_pooled), n, dx, s);
    return launch_conv1_dgrad(x, w, bias, static_cast<const float*>(d_pooled), n, dx, s);
}
