// rn_core.h -- what the forward (resnet.hip) and the backward (resnet_bwd.hip) of the ResNet-50 trunk share: the stem
// geometry and normalisation constants, the argument checks of the conv entry points, the dtype dispatch, the
// implicit-GEMM tile of rn_conv_kernel / rn_dgrad_s2_kernel and the BatchNorm slice reduction with its workspace layout.
// Everything is inline / constexpr: each translation unit compiles alone (-fno-gpu-rdc).
#ifndef MLA_RN_CORE_H
#define MLA_RN_CORE_H

#include "common.h"
#include "mma_core.h"

namespace rn {

using mma::bf16_t;
using mma::f32x4;
using mma::u32x4;

// stem: x (N, 224, 224) f32 -> NHWC (N, 112, 112, 64); Input normalisation (model.py:84-94): (x - mean_c) * inv_c
constexpr int kImg = 224, kStemOut = 112, kStemC = 64;
constexpr float kNormMean[3] = {0.485f, 0.456f, 0.406f}, kNormInv[3] = {1.f / 0.229f, 1.f / 0.224f, 1.f / 0.225f};

inline unsigned grid_for(int64_t work, int64_t cap = 16384) {
    const int64_t g = (work + 255) / 256;
    return unsigned(g < 1 ? 1 : (g > cap ? cap : g));
}

// The convs the trunk kernels are compiled for: mla_rn_conv, mla_rn_conv_dgrad and mla_rn_conv_wgrad accept the same ones.
#define RN_CONV_REQUIRE(who, ks, stride, cin, cout, dtype)                                                                        \
    do {                                                                                                                          \
        MLA_REQUIRE(((ks) == 1 || (ks) == 3) && ((stride) == 1 || (stride) == 2), MLA_E_SHAPE,                                    \
                    who ": kernel %lld stride %lld not compiled", (long long)(ks), (long long)(stride));                          \
        MLA_REQUIRE((cin) > 0 && (cout) > 0 && (cin) % 64 == 0 && (cout) % 64 == 0 && (cin) <= 4096 && (cout) <= 4096, MLA_E_SHAPE, \
                    who ": Cin %lld / Cout %lld must be multiples of 64 (<= 4096)", (long long)(cin), (long long)(cout));         \
        MLA_REQUIRE((dtype) == MLA_F32 || (dtype) == MLA_BF16, MLA_E_DTYPE, who " dtype %d", (dtype));                            \
    } while (0)

// f(Tag<T>{}) for the element type of a (checked) dtype:  rn_dispatch(dtype, [&](auto tag) { using T = typename decltype(tag)::type; ... });
template <typename T>
struct Tag {
    using type = T;
};

template <typename F>
inline void rn_dispatch(int dtype, F&& f) {
    if (dtype == MLA_F32)
        f(Tag<float>{});
    else
        f(Tag<bf16_t>{});
}

// ------------------------------------------------------------------------------------------------
// implicit-GEMM tile: rows = pixels, cols = the channels n of the weight rows w[n][tap][c], K = taps x KC channels
// (tap-major, channel-minor). Workgroup tile 128 pixels x BN channels (grid x, y), 4 waves as 2 x 2, one 128-byte LDS row
// per pixel / weight row per k-block (64 bf16 or 32 f32 channels of one tap). The next k-block is loaded into registers
// while the current one computes. The caller supplies
//   a_chunk(i, tap, c0)  the 16 bytes at channel c0 of tap `tap` for tile row (threadIdx.x >> 3) + 32 i (zero16 outside)
//   w_tap(tap)           the index of that tap in the KK taps of a weight row
//   column(n)            the epilogue of channel n: a functor (m, v) that stores accumulator v of pixel m < M (what it
//                        reads per channel, it reads once)
// MayBeEmpty: ntaps may be 0 (the accumulators stay 0); false spares the forward conv the guard around its first prefetch.
// ------------------------------------------------------------------------------------------------
constexpr int kTileM = 128, kTileAL = kTileM * 8 / 256;

template <typename T, int BN, bool MayBeEmpty, typename AChunk, typename WTap, typename Column>
__device__ __forceinline__ void conv_tile(const T* __restrict__ w, int KK, int KC, int ntaps, int64_t M, AChunk a_chunk, WTap w_tap,
                                          Column column) {
    constexpr int EPC = mma::Elem<T>::kPerChunk, EPR = mma::Elem<T>::kPerRow;
    constexpr int BM = kTileM, AL = kTileAL, BL = BN * 8 / 256, TN = BN / 32;
    __shared__ __attribute__((aligned(16))) char lds[(BM + BN) * mma::kRowBytes];
    char* As = lds;
    char* Bs = lds + BM * mma::kRowBytes;
    const int t = threadIdx.x, lane = t & 63, wid = t >> 6, q = t & 7, r0 = t >> 3;
    const int64_t m0 = int64_t(blockIdx.x) * BM;
    const int n0 = blockIdx.y * BN;
    const int csteps = KC / EPR, nk = ntaps * csteps;
    u32x4 ra[AL], rb[BL];
    auto load = [&](int k) {
        const int tap = k / csteps, cs = k - tap * csteps;
        const int c0 = cs * EPR + q * EPC;
#pragma unroll
        for (int i = 0; i < AL; ++i) ra[i] = a_chunk(i, tap, c0);
        const int wt = w_tap(tap);
#pragma unroll
        for (int j = 0; j < BL; ++j) {
            const int64_t n = n0 + r0 + 32 * j;
            rb[j] = *reinterpret_cast<const u32x4*>(w + (n * KK + wt) * KC + c0);
        }
    };

    f32x4 acc[4][TN];
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int j = 0; j < TN; ++j) acc[i][j] = f32x4{0.f, 0.f, 0.f, 0.f};

    const int wm = wid & 1, wn = wid >> 1;
    if (!MayBeEmpty || nk > 0) load(0);
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
        const auto store = column(n0 + wn * (BN / 2) + j * 16 + (lane & 15));
#pragma unroll
        for (int i = 0; i < 4; ++i) {
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                const int64_t m = m0 + wm * 64 + i * 16 + 4 * (lane >> 4) + e;
                if (m < M) store(m, acc[i][j][e]);
            }
        }
    }
}

// ------------------------------------------------------------------------------------------------
// BatchNorm2d sums over NHWC rows: block (channel group of 64, row slice p of P = gridDim.y). Thread: 8 channels (chunk q)
// of rows r0, r0+32, ... of its slice; two(off, c0, a, b) yields the two 8-wide factors of the row chunk at element offset
// off (channels c0 .. c0+7), and the block sums a and a * b (the product formed in double) in double. The 32 row lanes are
// added in LDS in a fixed order into part[(which * P + p) * C + c], the P slices by bn_sum_slices in slice order -> the
// same bits on every run for a given shape. kMaxSlices sizes the caller-owned workspaces of the forward and the backward.
// ------------------------------------------------------------------------------------------------
constexpr int kMaxSlices = 512;

inline int bn_slices(int64_t rows) {
    const int64_t p = (rows + 2047) / 2048;
    return int(p < 1 ? 1 : (p > kMaxSlices ? kMaxSlices : p));
}

template <typename Two>
__device__ __forceinline__ void bn_slice_sums(int64_t rows, int C, double* __restrict__ part, Two two) {
    __shared__ double red[2][32][64];
    const int t = threadIdx.x, q = t & 7, r0 = t >> 3;
    const int c0 = blockIdx.x * 64 + q * 8, P = gridDim.y, p = blockIdx.y;
    double s[8], s2[8];
#pragma unroll
    for (int k = 0; k < 8; ++k) s[k] = s2[k] = 0.0;
    for (int64_t r = int64_t(p) * 32 + r0; r < rows; r += int64_t(P) * 32) {
        float a[8], b[8];
        two(r * C + c0, c0, a, b);
#pragma unroll
        for (int k = 0; k < 8; ++k) { s[k] += a[k]; s2[k] += double(a[k]) * b[k]; }
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

// The P slices of one channel, added in slice order: the fixed order every consumer of `part` shares.
__device__ __forceinline__ void bn_sum_slices(const double* __restrict__ part, int P, int C, int c, double& s, double& s2) {
    s = 0.0;
    s2 = 0.0;
    for (int p = 0; p < P; ++p) { s += part[int64_t(p) * C + c]; s2 += part[int64_t(P + p) * C + c]; }
}

}  // namespace rn
#endif
