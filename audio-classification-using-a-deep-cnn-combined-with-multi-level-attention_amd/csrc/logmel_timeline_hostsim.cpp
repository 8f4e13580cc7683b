// logmel_timeline_hostsim.cpp -- TEST HARNESS (never part of libmla_hip.so): runs logmel_timeline_kernel's work items on the host
// in the kernel's order -- item -> recording through the descriptors' first_item prefix, item -> first column, logmel_core.h's
// phases for the 8 columns of an item that has a spectrum (as logmel_bags_hostsim.cpp runs them), zeros for any other, then the
// item's 8 columns into every kept slot that holds them -- through the index functions of logmel_timeline_core.h the kernel uses.
// Built with g++ -ffp-contract=off by tests/test_logmel_timeline_cpu.py. Every store also counts in `writes`, every column whose
// spectrum is computed counts in `computed`, and the highest sample read of each row is kept, so the test can show that each
// element of `out` is written exactly once, that no column outside the kept slots is computed and how far a row is read.
#include <cstdint>
#include <vector>

#include "logmel_hostsim_frame.h"
#include "logmel_timeline_core.h"

using namespace logmel;
using namespace logmel_timeline;

// The host-only arithmetic behind mla_timeline_counts, and the descriptor fields that follow from it.
extern "C" int hostsim_timeline_counts(int64_t n, int64_t q, int64_t* windows, int64_t* slots, int64_t* cols, int64_t* spec_cols,
                                       int64_t* items, int64_t* read) {
    if (!counts(n, q, windows, slots, cols, spec_cols)) return -1;
    *items = items_of(*cols, q);
    *read = samples_read(*spec_cols);
    return 0;
}

// pcm[recordings][row_stride] float32 at 16 kHz; desc[recordings][5] as mla_logmel_timeline takes it; out and writes:
// total_slots * 64 * 96 elements (writes must come in zeroed); computed[recordings][cols_pitch] (zeroed) counts the spectra of
// every column; max_read[recordings] receives the highest sample index read, -1 for none. Returns 0, or -(10 r + k) where check k
// of logmel_timeline::check_rec fails for recording r, -1 for total_slots that is not the sum, -3 for tables that do not build.
extern "C" int hostsim_logmel_timeline(const float* pcm, int64_t recordings, int64_t n_samples, int64_t row_stride, const int64_t* desc,
                                       int64_t total_slots, float* out, int32_t* writes, int32_t* computed, int64_t cols_pitch,
                                       int64_t* max_read) {
    const Rec* recs = reinterpret_cast<const Rec*>(desc);
    int64_t slot_prefix = 0, n_items = 0;
    for (int64_t r = 0; r < recordings; ++r) {
        const int bad = check_rec(recs[r], n_samples, slot_prefix, n_items);
        if (bad) return -int(10 * (r + 1) + bad);
        slot_prefix += slots_of(recs[r].cols, recs[r].q);
        n_items += items_of(recs[r].cols, recs[r].q);
        max_read[r] = -1;
    }
    if (slot_prefix != total_slots) return -1;
    std::vector<float> tab(kTabFloats);
    if (build_tables(tab.data()) != 0) return -3;
    LaneConsts c[16];
    for (int j = 0; j < 16; ++j) load_consts(c[j], tab.data(), j);
    for (int64_t item = 0; item < n_items; ++item) {
        const int r = find_rec(recs, int(recordings), item);
        const Rec& k = recs[r];
        const int col = item_column(int(item - k.first_item), int(k.cols), int(k.q));
        float stage[kItemCols][kBands];                        // the wave's stage: column-major, as the kernel's sink leaves it
        for (int x = 0; x < kItemCols; ++x) {
            if (col < k.spec_cols) {
                const int64_t s0 = column_sample(col + x);
                frame_row(c, tab.data(), pcm + r * row_stride + s0, stage[x]);
                ++computed[r * cols_pitch + col + x];
                if (s0 + kWin - 1 > max_read[r]) max_read[r] = s0 + kWin - 1;
            } else {
                for (int b = 0; b < kBands; ++b) stage[x][b] = 0.f;
            }
        }
        for (int band = 0; band < kBands; ++band) {            // lane = band
            for (int s = 0; s < kColumnSlots; ++s) {
                int row, x0;
                if (!column_slot(col, int(k.cols), int(k.q), s, &row, &x0)) continue;
                const int64_t o = out_offset(k.first_slot, row, band, x0);
                for (int x = 0; x < kItemCols; ++x) {
                    out[o + x] = stage[x][band];
                    ++writes[o + x];
                }
            }
        }
    }
    return 0;
}
