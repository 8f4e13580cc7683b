// logmel_bags_hostsim.cpp -- TEST HARNESS (never part of libmla_hip.so): runs logmel_bags_kernel's work items on the host in the
// kernel's order -- item -> (clip, slot, frame), logmel_core.h's phases for the 8 frames of an item the clip has (as
// logmel_hostsim.cpp runs them), zeros for any other, then the item's 8 columns into every window that holds them -- through
// the index functions of logmel_bags_core.h the kernel uses. Built with g++ -ffp-contract=off by tests/test_logmel_bags_cpu.py.
// Every store also counts in `writes`, so the test can show that each element of `out` is written exactly once.
#include <cstdint>
#include <vector>

#include "logmel_bags_core.h"
#include "logmel_hostsim_frame.h"

using namespace logmel;
using namespace logmel_bags;

// pcm[clips][row_stride] float32 at 16 kHz; counts[clips] in 0..4; out and writes: clips * n_frames * 64 * 96 elements (writes must
// come in zeroed). Returns 0, -1 for a configuration the kernel refuses, -2 for a count outside 0..4 or beyond n_samples.
extern "C" int hostsim_logmel_bags(const float* pcm, int64_t clips, int64_t n_samples, int64_t row_stride, const int32_t* counts,
                                   int n_frames, int stride, float* out, int32_t* writes) {
    if (!config_ok(n_frames, stride)) return -1;
    for (int64_t c = 0; c < clips; ++c)
        if (counts[c] < 0 || counts[c] > kSlots || samples_read(counts[c]) > n_samples) return -2;
    std::vector<float> tab(kTabFloats);
    if (build_tables(tab.data()) != 0) return -3;
    LaneConsts c[16];
    for (int j = 0; j < 16; ++j) load_consts(c[j], tab.data(), j);
    const int64_t n_items = clips * kClipItems;
    for (int64_t item = 0; item < n_items; ++item) {
        int clip, slot, frame;
        item_locate(int(item), &clip, &slot, &frame);
        float stage[kItemCols][kBands];                        // the wave's stage: column-major, as the kernel's sink leaves it
        for (int x = 0; x < kItemCols; ++x) {
            if (slot < counts[clip]) {
                frame_row(c, tab.data(), pcm + clip * row_stride + frame_sample(slot, frame + x), stage[x]);
            } else {
                for (int b = 0; b < kBands; ++b) stage[x][b] = 0.f;
            }
        }
        const int col = item_column(slot, frame);
        int t_lo, t_hi;
        column_windows(col, n_frames, stride, &t_lo, &t_hi);
        for (int band = 0; band < kBands; ++band) {            // lane = band
            for (int t = t_lo; t <= t_hi; ++t) {
                const int64_t o = out_offset(clip, n_frames, stride, t, band, col);
                for (int x = 0; x < kItemCols; ++x) {
                    out[o + x] = stage[x][band];
                    ++writes[o + x];
                }
            }
        }
    }
    return 0;
}
