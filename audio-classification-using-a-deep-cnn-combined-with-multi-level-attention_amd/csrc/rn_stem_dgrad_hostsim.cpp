// rn_stem_dgrad_hostsim.cpp -- TEST HARNESS (never part of libmla_hip.so): runs rn_stem_dgrad_kernel's work items on the host in the
// kernel's order -- workgroup -> its items by grid stride, per item the four channel passes, per pass the stage loop (g of the
// tile's 7 output rows into the workgroup's LDS image) then the gather (lane = 7 pixels) -- through the functions of
// rn_stem_dgrad_core.h the kernel uses. Built with g++ -ffp-contract=off by tests/test_rn_stem_dgrad_cpu.py. Every store to dx also
// counts in `writes`, and the highest element read of dy, y, scale and w is kept, so the test can show that each element of dx is
// written exactly once and that no input is read past its end.
#include <cstdint>
#include <vector>

#include "rn_stem_dgrad_core.h"

using namespace rn_stem_dgrad;

extern "C" int hostsim_rn_stem_dgrad_max_wg(void) { return kMaxWg; }
extern "C" int hostsim_rn_stem_dgrad_grid(int64_t n) { return grid_of(n); }
extern "C" int hostsim_rn_stem_dgrad_tiles(void) { return kTiles; }

// dy (n, 112, 112, 64) as float32 (the values a bf16 tensor holds, for bf16), y likewise or null, scale (64) or null, w (64, 3, 7, 7);
// grid: workgroups, 0 = the launcher's choice; dx and writes (zeroed by the caller): n * 224 * 224 elements; max_read[4]: highest
// element index read of dy, y, scale, w (-1: none). Returns 0, -1 for bad arguments, -2 / -3 for an index outside LDS / dx.
extern "C" int hostsim_rn_stem_dgrad(const float* dy, const float* y, const float* scale, const float* w, int single, int64_t n, int grid,
                                     float* dx, int32_t* writes, int64_t* max_read) {
    if (n < 0 || grid < 0 || (y == nullptr) != (scale == nullptr)) return -1;
    for (int k = 0; k < 4; ++k) max_read[k] = -1;
    if (n == 0) return 0;
    if (grid == 0) grid = grid_of(n);
    auto seen = [&](int which, int64_t at) { if (at > max_read[which]) max_read[which] = at; };
    std::vector<float> sA(kTaps * kC), sG(kSlots * kOut * kGroup);
    for (int i = 0; i < kC * kTaps; ++i) {
        const int o = i / kTaps, tap = i - o * kTaps;
        for (int c = 0; c < 3; ++c) seen(3, w_index(o, c, tap));
        sA[a_index(o, tap)] = fold_a(w[w_index(o, 0, tap)], w[w_index(o, 1, tap)], w[w_index(o, 2, tap)], single);
    }
    const int64_t n_items = items_of(n);
    std::vector<float> acc(kTileRows * kImg);
    for (int wg = 0; wg < grid; ++wg) {
        for (int64_t item = wg; item < n_items; item += grid) {
            const int64_t img = item / kTiles;
            const int tile = int(item % kTiles);
            for (auto& a : acc) a = 0.f;
            for (int grp = 0; grp < kGroups; ++grp) {
                for (int i = 0; i < kStageLoads; ++i) {                                 // stage: lane i % kThreads, step i / kThreads
                    int r, ox, c8;
                    stage_of(i, &r, &ox, &c8);
                    const int oy = slot_row(tile, r);
                    const int at = s_index(r, ox) + c8;
                    if (at < 0 || at + 8 > int(sG.size())) return -2;
                    for (int k = 0; k < 8; ++k) {
                        float g = 0.f;
                        if (row_live(oy)) {
                            const int c = grp * kGroup + c8 + k;
                            const int64_t off = g_index(img, oy, ox) + c;
                            seen(0, off);
                            g = dy[off];
                            if (y) {
                                seen(1, off);
                                seen(2, c);
                                g = route(g, y[off], scale[c], true);
                            }
                        }
                        sG[at + k] = g;
                    }
                }
                for (int t = 0; t < kThreads; ++t)                                      // gather
                    for (int j = 0; j < kPixPerLane; ++j) {
                        const int p = t + kThreads * j;
                        int row, ix, ky0, nty, fy, kx0, ntx, fx;
                        pixel_of(p, &row, &ix);
                        axis_taps(row, &ky0, &nty, &fy);
                        axis_taps(ix, &kx0, &ntx, &fx);
                        for (int jy = 0; jy < nty; ++jy) {
                            const int r = fy - jy + 1;
                            if (r < 0 || r >= kSlots) return -2;
                            if (!row_live(slot_row(tile, r))) continue;
                            for (int jx = 0; jx < ntx; ++jx) {
                                const int ox = fx - jx;
                                if (ox < 0 || ox >= kOut) continue;
                                const int tap = (ky0 + 2 * jy) * 7 + kx0 + 2 * jx;
                                if (tap < 0 || tap >= kTaps) return -2;
                                acc[p] = gather(acc[p], sG.data() + s_index(r, ox), sA.data() + a_index(grp * kGroup, tap));
                            }
                        }
                    }
            }
            for (int p = 0; p < kTileRows * kImg; ++p) {
                int row, ix;
                pixel_of(p, &row, &ix);
                const int64_t o = (img * kImg + tile * kTileRows + row) * kImg + ix;
                if (o < 0 || o >= n * kImg * kImg) return -3;
                dx[o] = acc[p];
                ++writes[o];
            }
        }
    }
    return 0;
}
