// logmel_bwd_hostsim.cpp -- TEST HARNESS (never part of libmla_hip.so): runs logmel_bwd_kernel's work items on the host in the
// kernel's order -- workgroup -> its items by grid stride, per item the 16 groups of 16 lanes stage by stage (every hand-off of the
// kernel is the end of a loop over all lanes here), then the gather -- through the functions of logmel_bwd_core.h the kernel uses,
// with plain arrays standing in for LDS. Built with g++ -ffp-contract=off by tests/test_logmel_bwd_cpu.py. Every store to d_wave
// also counts in `writes`, and the highest element read of pcm and of d_examples is kept, so the test can show that each element
// is written exactly once and that no input is read past its last used element.
#include <cstdint>
#include <vector>

#include "logmel_bwd_core.h"

using namespace logmel_bwd;

extern "C" int hostsim_logmel_bwd_max_wg(void) { return kMaxWg; }
extern "C" int hostsim_logmel_bwd_grid(int64_t n_items) { return grid_of(n_items); }
extern "C" int64_t hostsim_logmel_bwd_items(int64_t n_wave, int64_t n_samples) { return n_wave * items_per_row(n_samples); }
extern "C" int hostsim_logmel_bwd_table_floats(void) { return kBwdTabFloats; }
extern "C" int hostsim_logmel_bwd_build_tables(float* tab) { return build_bwd_tables(tab); }

// pcm: n_wave rows of n_samples (float32, or int16 when is_i16) at `stride` elements; g: (n_wave * N, 96, 64) float32; grid:
// workgroups, 0 = the launcher's choice; d_wave / writes: n_wave rows at `d_stride` (writes zeroed by the caller); max_read[2]:
// highest element index read of pcm and g (-1: none). Returns 0, negative for bad sizes or an index outside an array.
extern "C" int hostsim_logmel_bwd(const void* pcm, int is_i16, int64_t n_wave, int64_t n_samples, int64_t stride, const float* g, int grid,
                                  float* d_wave, int64_t d_stride, int32_t* writes, int64_t* max_read) {
    if (n_wave < 0 || n_samples < 0 || stride < n_samples || d_stride < n_samples || grid < 0) return -1;
    max_read[0] = max_read[1] = -1;
    std::vector<float> tab(kTabFloats), btab(kBwdTabFloats);
    if (build_tables(tab.data()) != 0 || build_bwd_tables(btab.data()) != 0) return -2;
    const int64_t ipr = items_per_row(n_samples), n_items = n_wave * ipr, used = used_frames(n_samples);
    if (n_items == 0) return 0;
    if (grid == 0) grid = grid_of(n_items);
    const float* win = tab.data() + kTabWindow;
    LaneConsts c[16];
    for (int j = 0; j < 16; ++j) load_consts(c[j], tab.data(), j);
    auto sample = [&](int64_t at) {
        if (at > max_read[0]) max_read[0] = at;
        return is_i16 ? float(static_cast<const int16_t*>(pcm)[at]) * (1.0f / 32768.0f) : static_cast<const float*>(pcm)[at];
    };
    std::vector<float> lds(kItemFrames * kGroupFloats);
    struct Lane { float re[16], im[16], pr[16], pi[16], ur[16], ui[16]; };
    std::vector<Lane> lanes(kThreads);
    for (int wg = 0; wg < grid; ++wg) {
        for (int64_t item = wg; item < n_items; item += grid) {
            int64_t row, c0;
            item_locate(item, ipr, &row, &c0);
            bool live[kItemFrames];
            for (int grp = 0; grp < kItemFrames; ++grp) live[grp] = frame_live(group_frame(c0, grp), used);
            auto each = [&](auto&& fn) {                   // one stage: every lane of every live group, then the hand-off
                for (int grp = 0; grp < kItemFrames; ++grp) {
                    if (!live[grp]) continue;
                    float* a = lds.data() + grp * kGroupFloats;
                    for (int j = 0; j < 16; ++j) fn(grp, j, lanes[grp * 16 + j], a, a + kBufA);
                }
            };
            each([&](int grp, int j, Lane& l, float* a, float*) {
                const int64_t f = group_frame(c0, grp);
                float x[2 * kN1];
                for (int n = 0; n < kN1; ++n)
                    for (int e = 0; e < 2; ++e) {
                        const int m = lane_sample(j, n, e);
                        x[2 * n + e] = m < kWin ? sample(pcm_index(row, stride, f, m)) : 0.f;
                    }
                window_lane(j, x, win, l.re, l.im);
                phase1_fft(c[j], j, l.re, l.im, a);
            });
            each([&](int, int j, Lane& l, float* a, float*) { phase2_read(j, a, l.re, l.im); });
            each([&](int, int j, Lane& l, float* a, float*) { phase2_fft(l.re, l.im); store_z(j, l.re, l.im, a); });
            each([&](int, int j, Lane& l, float* a, float* b) { split_lane(j, btab.data(), a, b, l.pr, l.pi); });
            each([&](int grp, int j, Lane&, float*, float* b) {
                const int64_t f = group_frame(c0, grp);
                float gv[4];
                for (int s = 0; s < 4; ++s) {
                    const int64_t at = g_index(row, used, f, band_of(j, s));
                    if (at > max_read[1]) max_read[1] = at;
                    gv[s] = g[at];
                }
                ratio_lane(c[j], j, b, tab.data() + kTabMelW + kMelRow * j, gv, b + 256);
            });
            each([&](int, int j, Lane& l, float* a, float* b) { spectrum_grad_lane(j, btab.data(), b + 256, l.pr, l.pi, l.ur, l.ui, a); });
            each([&](int, int j, Lane& l, float* a, float*) { join_lane(j, btab.data(), l.ur, l.ui, a, l.re, l.im); });
            each([&](int, int j, Lane& l, float* a, float*) { phase1_fft_full(c[j], j, l.re, l.im, a); });
            each([&](int, int j, Lane& l, float* a, float*) { phase2_read(j, a, l.re, l.im); });
            each([&](int, int j, Lane& l, float* a, float*) { phase2_fft(l.re, l.im); window_out_lane(j, l.re, l.im, win, a); });
            for (int t = 0; t < kThreads; ++t)                                          // the gather
                for (int i = t; i < kItemChunks * kHop; i += kThreads) {
                    int cl, o;
                    out_locate(i, &cl, &o);
                    const int64_t s = (c0 + cl) * kHop + o;
                    if (s >= n_samples) continue;
                    float acc = 0.f;
                    for (int d = 0; d < 3; ++d) {
                        const int m = term_pos(o, d), grp = cl + d;
                        if (grp < 0 || grp >= kItemFrames) return -3;
                        if (m < kWin && live[grp]) acc += lds[grp * kGroupFloats + m];
                    }
                    const int64_t at = row * d_stride + s;
                    d_wave[at] = acc;
                    ++writes[at];
                }
        }
    }
    return 0;
}
