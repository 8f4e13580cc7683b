// rn_stem_dgrad_core.h -- tile, halo, tap-map and gather arithmetic of rn_stem_dgrad_kernel (resnet_bwd.hip), written so that the
// SAME source runs inside the kernel on gfx950 and on the host in csrc/rn_stem_dgrad_hostsim.cpp (built with g++ by the CPU tests).
//
// dx (n, 224, 224) f32 = the gradient of the ResNet stem with respect to the RAW planes Input receives. The forward
// (rn_stem_kernel, resnet.hip) folds Input's channel repeat / single configuration and normalisation into one coefficient per
// (output channel, tap): a[o][ky][kx] = sum over the channels that carry x of w[o][c][ky][kx] / std_c; the constant part b of the
// fold has no gradient. Output (oy, ox) reads input (2 oy - 3 + ky, 2 ox - 3 + kx), so
//   dx[iy][ix] = sum_o sum_{ky,kx} a[o][ky][kx] g[(iy + 3 - ky) / 2][(ix + 3 - kx) / 2][o]
// over the taps whose two quotients are integers in [0, 112): ky = ky0 + 2 jy with ky0 = (iy + 1) & 1, 4 taps for odd iy and 3 for
// even iy, likewise kx. g is the gradient of the conv sum: dy, or dy (y > 0) scale[o] behind the eval-mode epilogue
// y = relu(conv scale + shift) (y NaN gives 0, as torch's threshold_backward).
//
// Work item = (image, tile of 8 input rows x 224 columns); one 256-lane workgroup per item at a time, 7 pixels per lane. The tile's
// rows collect from the 7 output rows 4 tile - 1 .. 4 tile + 5 (slots 0 .. 6; rows outside the image are zero-filled and never
// gathered). The 64 channels go in four passes of 16: a pass stages g of the 7 x 112 positions in LDS (a 16-byte load of 8
// channels per lane and step), then every pixel gathers its 3 or 4 x 3 or 4 positions x 16 channels in the fixed order (jy, jx,
// channel). Every dx element is owned by one lane of one item and stored once; its sum runs in an order that depends on nothing
// but the pixel: the bits do not depend on n or on the grid. No atomics, no workspace, nothing for the caller to zero.
#ifndef MLA_RN_STEM_DGRAD_CORE_H
#define MLA_RN_STEM_DGRAD_CORE_H

#include <cmath>
#include <cstdint>

#ifndef MLA_HD
#if defined(__HIPCC__)
#define MLA_HD __host__ __device__ __forceinline__
#else
#define MLA_HD inline
#endif
#endif

namespace rn_stem_dgrad {

constexpr int kImg = 224, kOut = 112, kC = 64, kTaps = 49;       // input plane, output plane, output channels, 7 x 7 taps
constexpr float kInv[3] = {1.f / 0.229f, 1.f / 0.224f, 1.f / 0.225f};      // Input's 1 / std_c (rn_core.h kNormInv)
constexpr int kThreads = 256;
constexpr int kTileRows = 8;                                     // input rows per item
constexpr int kTiles = kImg / kTileRows;                         // items per image
constexpr int kSlots = kTileRows / 2 + 3;                        // output rows a tile gathers from
constexpr int kGroup = 16, kGroups = kC / kGroup;                // channels per pass through LDS
constexpr int kPixPerLane = kTileRows * kImg / kThreads;         // 7
constexpr int kStageLoads = kSlots * kOut * (kGroup / 8);        // 8-channel loads per pass
constexpr int kMaxWg = 512;                                      // persistent workgroups (2 per CU at 61 KB of LDS each)
static_assert(kTileRows % 2 == 0 && kImg % kTileRows == 0 && kTileRows * kImg % kThreads == 0 && kGroup % 8 == 0, "rn_stem_dgrad tiling");

MLA_HD int64_t items_of(int64_t n) { return n * kTiles; }
MLA_HD int grid_of(int64_t n) { return int(items_of(n) < kMaxWg ? items_of(n) : kMaxWg); }

// the forward's folded tap coefficient (rn_stem_kernel): what d(conv sum) / dx of a tap inside the image is
MLA_HD float fold_a(float w0, float w1, float w2, int single) {
    return single ? w0 * kInv[0] : w0 * kInv[0] + w1 * kInv[1] + w2 * kInv[2];
}
// staged coefficients: sA[tap * kC + o], so that the 16 channels of a pass are contiguous
MLA_HD int a_index(int o, int tap) { return tap * kC + o; }
// element of w (64, 3, 7, 7) that channel c of (o, tap) reads
MLA_HD int w_index(int o, int c, int tap) { return (o * 3 + c) * kTaps + tap; }

// output row of slot r (0 .. kSlots - 1) of a tile: -1, 112 and 113 are outside the image
MLA_HD int slot_row(int tile, int r) { return (kTileRows / 2) * tile - 1 + r; }
MLA_HD bool row_live(int oy) { return oy >= 0 && oy < kOut; }

// Stage load i (0 .. kStageLoads - 1) of a pass: slot r, output column ox, first channel c8 (0 or 8) within the group
MLA_HD void stage_of(int i, int* r, int* ox, int* c8) {
    const int pos = i / (kGroup / 8);
    *c8 = (i - pos * (kGroup / 8)) * 8;
    *r = pos / kOut;
    *ox = pos - *r * kOut;
}
// first channel of output (oy, ox) of image n in dy / y (n, 112, 112, 64)
MLA_HD int64_t g_index(int64_t n, int oy, int ox) { return ((n * kOut + oy) * kOut + ox) * kC; }
// LDS float offset of (slot, ox) within a pass
MLA_HD int s_index(int r, int ox) { return (r * kOut + ox) * kGroup; }

// g of one element: the eval epilogue's mask-and-scale, or dy itself (has_y false)
MLA_HD float route(float dy, float y, float scale, bool has_y) { return has_y ? (y > 0.f ? dy : 0.f) * scale : dy; }

// Pixel p (0 .. 1791) of a tile: its row in the tile and column.
MLA_HD void pixel_of(int p, int* row, int* ix) {
    *row = p / kImg;
    *ix = p - *row * kImg;
}
// Tap subset along one axis of the pixel at coordinate i (the tile starts at an even row, so the in-tile row has iy's parity):
// taps k = k0 + 2 j, j < count, the j-th reaching output coordinate first - j (which may lie outside [0, 112)).
MLA_HD void axis_taps(int i, int* k0, int* count, int* first) {
    *k0 = (i + 1) & 1;
    *count = (7 - *k0 + 1) / 2;
    *first = (i + 3 - *k0) / 2;
}

// One output position's share of one pixel, the kGroup channels of a pass in order. g: the position's staged gradients,
// a: the tap's staged coefficients of the pass.
MLA_HD float gather(float acc, const float* g, const float* a) {
    _Pragma("unroll") for (int c = 0; c < kGroup; ++c) acc = fmaf(a[c], g[c], acc);
    return acc;
}

}  // namespace rn_stem_dgrad
#endif
