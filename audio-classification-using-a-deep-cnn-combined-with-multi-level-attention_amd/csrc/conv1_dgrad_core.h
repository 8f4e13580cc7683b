// conv1_dgrad_core.h -- tile, halo, window-code and gather arithmetic of conv1_dgrad_kernel (conv1_dgrad.hip), written so that the
// SAME source runs inside the kernel on gfx950 and on the host in csrc/conv1_dgrad_hostsim.cpp (built with g++ by the CPU tests).
//
// dx = d/dx of max_pool2d(relu(conv2d(x, w, bias, padding=1)), 2) contracted with d_pooled, x (n, 96, 64), Cin = 1, 64 channels.
// The layer is recomputed under the rules of conv1_bwd_kernel (cnn_train.hip, first_max in cnn_train_core.h): the f32 fma chain in
// (ky, kx) order, the bias added after the pool, the FIRST maximum in scan order takes the gradient, nothing flows where
// best + bias <= 0.
//
// Work item = (clip, tile of 12 input rows x 64 columns); one 256-lane workgroup per item at a time. Pre-pool output (oy, ox) reads
// input (oy - 1 + ky, ox - 1 + kx), so input pixel (iy, ix) collects from the pre-pool outputs (iy + 1 - ky, ix + 1 - kx): rows
// iy0 - 1 .. iy0 + 12 of a tile that starts at iy0, i.e. the 8 pooled rows 6 tile - 1 .. 6 tile + 6 (one window of halo on either
// side) by 32 pooled columns = 256 windows, one per lane. Channels go in four groups of 16:
//   phase 1  lane = window: recompute the four pre-pool outputs per channel and leave in LDS the routed gradient g (d_pooled where
//            the ReLU is on, else 0) and a one-byte code: 4 x the window position 0..3 of the first maximum, or 16 = off. Windows
//            outside the image (pooled row -1 or 48) are off and read nothing.
//   phase 2  lane = 3 input pixels: each pixel meets 2 x 2 windows; in the fixed order (window, channel) it adds g * w[ch][tap] where
//            the code's position is the pre-pool output that tap (ky, kx) of this pixel addresses. Which tap reaches which of a
//            window's four positions depends on the (pixel, window) pair alone: a tap word of five nibbles, made once per lane, that
//            the code shifts into place (9 of the 16 pairings exist; the others and "off" read kNoTap).
// Every dx element is owned by one lane of one item and stored once; its sum runs over channel groups, windows and channels in an
// order that depends on nothing but the pixel: the bits do not depend on n or on the grid.
#ifndef MLA_CONV1_DGRAD_CORE_H
#define MLA_CONV1_DGRAD_CORE_H

#include <cmath>
#include <cstdint>

#ifndef MLA_HD
#if defined(__HIPCC__)
#define MLA_HD __host__ __device__ __forceinline__
#else
#define MLA_HD inline
#endif
#endif

namespace conv1_dgrad {

constexpr int kH = 96, kW = 64, kPH = 48, kPW = 32, kC = 64;     // input, pooled output, channels
constexpr int kThreads = 256;
constexpr int kTileRows = 12;                                    // input rows per item
constexpr int kTiles = kH / kTileRows;                           // items per clip
constexpr int kWinRows = kTileRows / 2 + 2;                      // pooled rows an item recomputes: its own 6 and one of halo each side
constexpr int kWins = kWinRows * kPW;                            // = kThreads: one window per lane
constexpr int kGroup = 16, kGroups = kC / kGroup;                // channels per pass through LDS
constexpr int kPixPerLane = kTileRows * kW / kThreads;           // 3
constexpr int kOff = 16;                                         // code: the ReLU is off (or the window is outside the image); else 4 x position
constexpr int kNoTap = 15;                                       // tap-word nibble: no tap of this pixel reaches that position
constexpr int kWPitch = 16;                                      // floats per channel of the staged filters: taps 0..8, then zeros
constexpr int kMaxWg = 768;                                      // persistent workgroups (3 per CU at 29 KB of LDS each)
static_assert(kWins == kThreads && kTileRows % 2 == 0 && kH % kTileRows == 0 && kTileRows * kW % kThreads == 0, "conv1_dgrad tiling");

MLA_HD int64_t items_of(int64_t n) { return n * kTiles; }
MLA_HD int grid_of(int64_t n) { return int(items_of(n) < kMaxWg ? items_of(n) : kMaxWg); }

// round-to-nearest-even to bf16, as the bf16 forward rounds x and w (NaN stays NaN)
MLA_HD float round_bf16(float f) {
    uint32_t u;
    __builtin_memcpy(&u, &f, 4);
    if ((u & 0x7fffffffu) > 0x7f800000u) return f;
    u = (u + 0x7fffu + ((u >> 16) & 1u)) & 0xffff0000u;
    __builtin_memcpy(&f, &u, 4);
    return f;
}

// pooled row of window-slot row r (0 .. kWinRows - 1) of a tile: -1 and 48 are outside the image
MLA_HD int window_row(int tile, int r) { return (kTileRows / 2) * tile - 1 + r; }
MLA_HD bool window_live(int wy) { return wy >= 0 && wy < kPH; }

// element of x under patch position (a, b) of window (wy, wx) of clip n: input (2 wy - 1 + a, 2 wx - 1 + b), or -1 for the zero padding
MLA_HD int64_t patch_index(int64_t n, int wy, int wx, int a, int b) {
    const int iy = 2 * wy - 1 + a, ix = 2 * wx - 1 + b;
    if (iy < 0 || iy >= kH || ix < 0 || ix >= kW) return -1;
    return (n * kH + iy) * kW + ix;
}
// first channel of window (wy, wx) of clip n in d_pooled (n, 48, 32, 64)
MLA_HD int64_t d_index(int64_t n, int wy, int wx) { return ((n * kPH + wy) * kPW + wx) * kC; }

// The window's code for one channel: the four pre-pool outputs in scan order (0,0) (0,1) (1,0) (1,1) as conv1_bwd_kernel forms them,
// torch's routing rule (a later value wins only if it is greater), the bias after the pool, relu'(0) = 0.
MLA_HD int window_code(const float (&patch)[4][4], const float* w9, float bias) {
    float o[4] = {0.f, 0.f, 0.f, 0.f};
    _Pragma("unroll") for (int ky = 0; ky < 3; ++ky)
        _Pragma("unroll") for (int kx = 0; kx < 3; ++kx) {
            const float wv = w9[ky * 3 + kx];
            o[0] = fmaf(patch[ky][kx], wv, o[0]);
            o[1] = fmaf(patch[ky][kx + 1], wv, o[1]);
            o[2] = fmaf(patch[ky + 1][kx], wv, o[2]);
            o[3] = fmaf(patch[ky + 1][kx + 1], wv, o[3]);
        }
    float best = o[0];
    int arg = 0;
    if (o[1] > best) { best = o[1]; arg = 1; }
    if (o[2] > best) { best = o[2]; arg = 2; }
    if (o[3] > best) { best = o[3]; arg = 3; }
    return best + bias > 0.f ? 4 * arg : kOff;
}

// Input pixel p (0 .. 767) of a tile: its row in the tile and column, and the first of its 2 x 2 windows as (slot row, pooled
// column): pre-pool rows iy - 1 .. iy + 1 span slot rows r0, r0 + 1, pre-pool columns ix - 1 .. ix + 1 the pooled columns wx0 (-1 at
// ix = 0), wx0 + 1 (32 at ix = 63).
MLA_HD void pixel_windows(int p, int* row, int* ix, int* r0, int* wx0) {
    *row = p / kW;
    *ix = p % kW;
    *r0 = (*row + 1) >> 1;
    *wx0 = ((*ix + 1) >> 1) - 1;
}
// Tap word of the pixel at tile row `row`, column ix for the window at slot row r, pooled column wx: position (py, px) of the window
// is pre-pool output (2 wy + py, 2 wx + px), reached from the pixel by tap ky = dy - py, kx = dx - px with dy = iy + 1 - 2 wy,
// dx = ix + 1 - 2 wx. Nibble at bit 4 * position = ky * 3 + kx, or kNoTap outside the 3 x 3 filter; the nibble at bit kOff = kNoTap.
MLA_HD uint32_t tap_word(int row, int r, int ix, int wx) {
    const int dy = row + 3 - 2 * r, dx = ix + 1 - 2 * wx;
    uint32_t word = uint32_t(kNoTap) << kOff;
    for (int pos = 0; pos < 4; ++pos) {
        const int ky = dy - (pos >> 1), kx = dx - (pos & 1);
        const bool in = ky >= 0 && ky < 3 && kx >= 0 && kx < 3;
        word |= uint32_t(in ? ky * 3 + kx : kNoTap) << (4 * pos);
    }
    return word;
}

// One window's share of one pixel, the kGroup channels of a group in order. w: the group's [kGroup][kWPitch] filters.
MLA_HD float gather(float acc, const uint8_t* codes, const float* g, const float* w, uint32_t taps) {
    _Pragma("unroll") for (int c = 0; c < kGroup; ++c) {
        const uint32_t tap = (taps >> codes[c]) & 15u;
        // no tap: 0 * (the zero padding of the filter row) is added, whatever g holds. Branch-free on purpose: a branch around the
        // filter read makes every one of the 192 reads of a pass wait for its own LDS round trip
        const float gm = tap != uint32_t(kNoTap) ? g[c] : 0.f;
        acc = fmaf(gm, w[c * kWPitch + tap], acc);
    }
    return acc;
}

}  // namespace conv1_dgrad
#endif
