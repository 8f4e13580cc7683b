// conv1_dgrad_hostsim.cpp -- TEST HARNESS (never part of libmla_hip.so): runs conv1_dgrad_kernel's work items on the host in the
// kernel's order -- workgroup -> its items by grid stride, per item the four channel groups, per group phase 1 (lane = window: patch,
// codes and routed gradients into the workgroup's LDS images) then phase 2 (lane = 3 pixels: the gather over 2 x 2 windows) -- through
// the functions of conv1_dgrad_core.h the kernel uses. Built with g++ -ffp-contract=off by tests/test_conv1_dgrad_cpu.py. Every
// store to dx also counts in `writes`, and the highest element read of x, w, bias and d_pooled is kept, so the test can show that
// each element of dx is written exactly once and that no input is read past its end.
#include <cstdint>
#include <vector>

#include "conv1_dgrad_core.h"

using namespace conv1_dgrad;

extern "C" int hostsim_conv1_dgrad_max_wg(void) { return kMaxWg; }
extern "C" int hostsim_conv1_dgrad_grid(int64_t n) { return grid_of(n); }

// x (n, 96, 64), w (64, 9), bias (64), d (n, 48, 32, 64) as float32 (bf16 != 0: values a bf16 tensor holds; x and w are rounded to
// bf16 for the recompute); grid: workgroups, 0 = the launcher's choice; dx and writes (zeroed by the caller): n * 96 * 64 elements;
// max_read[4]: highest element index read of x, w, bias, d (-1: none). Returns 0, -1 for bad sizes.
extern "C" int hostsim_conv1_dgrad(const float* x, const float* w, const float* bias, const float* d, int bf16, int64_t n, int grid,
                                   float* dx, int32_t* writes, int64_t* max_read) {
    if (n < 0 || grid < 0) return -1;
    for (int k = 0; k < 4; ++k) max_read[k] = -1;
    if (n == 0) return 0;
    if (grid == 0) grid = grid_of(n);
    auto seen = [&](int which, int64_t at) { if (at > max_read[which]) max_read[which] = at; };
    std::vector<float> sW(kC * kWPitch, 0.f), sG(kWins * kGroup);
    std::vector<uint8_t> sC(kWins * kGroup);
    for (int i = 0; i < kC * 9; ++i) {
        sW[i / 9 * kWPitch + i % 9] = bf16 ? round_bf16(w[i]) : w[i];
        seen(1, i);
    }
    const int64_t n_items = items_of(n);
    for (int wg = 0; wg < grid; ++wg) {
        for (int64_t item = wg; item < n_items; item += grid) {
            const int64_t img = item / kTiles;
            const int tile = int(item % kTiles);
            std::vector<float> acc(kTileRows * kW, 0.f);
            for (int grp = 0; grp < kGroups; ++grp) {
                for (int t = 0; t < kThreads; ++t) {                                    // phase 1
                    const int r = t / kPW, wx = t % kPW, wy = window_row(tile, r);
                    const bool live = window_live(wy);
                    float patch[4][4];
                    for (int a = 0; a < 4; ++a)
                        for (int b = 0; b < 4; ++b) {
                            const int64_t at = live ? patch_index(img, wy, wx, a, b) : -1;
                            if (at >= 0) seen(0, at);
                            const float v = at >= 0 ? x[at] : 0.f;
                            patch[a][b] = bf16 ? round_bf16(v) : v;
                        }
                    for (int c = 0; c < kGroup; ++c) {
                        const int ch = grp * kGroup + c;
                        int code = kOff;
                        float g = 0.f;
                        if (live) {
                            const int64_t at = d_index(img, wy, wx) + ch;
                            seen(3, at);
                            seen(2, ch);
                            code = window_code(patch, sW.data() + ch * kWPitch, bias[ch]);
                            g = code == kOff ? 0.f : d[at];
                        }
                        sG[t * kGroup + c] = g;
                        sC[t * kGroup + c] = uint8_t(code);
                    }
                }
                for (int t = 0; t < kThreads; ++t)                                      // phase 2
                    for (int j = 0; j < kPixPerLane; ++j) {
                        const int p = t + kThreads * j;
                        int row, ix, r0, wx0;
                        pixel_windows(p, &row, &ix, &r0, &wx0);
                        for (int s = 0; s < 4; ++s) {
                            const int rs = r0 + (s >> 1), ws = wx0 + (s & 1);
                            if (ws < 0 || ws >= kPW) continue;
                            const int slot = rs * kPW + ws;
                            if (slot < 0 || slot >= kWins) return -2;
                            acc[p] = gather(acc[p], sC.data() + slot * kGroup, sG.data() + slot * kGroup, sW.data() + grp * kGroup * kWPitch,
                                            tap_word(row, rs, ix, ws));
                        }
                    }
            }
            for (int p = 0; p < kTileRows * kW; ++p) {
                const int64_t o = (img * kH + tile * kTileRows + p / kW) * kW + p % kW;
                if (o < 0 || o >= n * kH * kW) return -3;
                dx[o] = acc[p];
                ++writes[o];
            }
        }
    }
    return 0;
}
