// logmel_timeline_core.h -- index arithmetic of the timeline kernel (logmel_timeline_kernel in logmel.hip), written so that the SAME
// source runs inside the kernel on gfx950 and on the host in csrc/logmel_timeline_hostsim.cpp (built with g++ by the CPU tests).
//
// A recording at 16 kHz with n samples has the log-mel columns c = 0 .. (n - 400) / 160. With hop_slots = q >= 1 (a hop of 32 q
// columns = 0.32 q s) a LONG recording (n >= 61 680, four whole examples) is scored in
//   W = 1 + (n - 61 680) / (5 120 q)
// windows; window j is the reference's native bag (dataset.py:318-324 create_spec + :355-359 overlapping_split) of the crop
// wave[5 120 q j : 5 120 q j + 61 680], whose slot t < 10 is columns [32 (q j + t), 32 (q j + t) + 96) of the recording. A SHORT
// recording (240 <= n < 61 680) has the one window logmel_bags_core.h gives it: columns of the examples it lacks are 0.0.
//
//   slot u = columns [32 u, 32 u + 96), kept iff u mod q < 10 and u <= q (W - 1) + 9; kept slots are stored in order of u:
//   q <= 10: q (W - 1) + 10 rows, window j = rows q j .. q j + 9;      q > 10: 10 W rows, window j = rows 10 j .. 10 j + 9
//
// The track of a recording is its columns 0 .. cols - 1, cols = 32 q (W - 1) + 384. Work item = 8 consecutive columns (one
// wave-iteration of pair_step). Only items of columns that lie in a kept slot exist: all of the track for q <= 11 (at q = 11 the
// windows still overlap by 32 columns), 48 per window for q >= 12. An item whose columns have a spectrum (col < spec_cols) computes
// them, any other (a short recording's missing examples) stores 0.0; either way the item writes its 8 columns into every kept slot
// that holds them, so each element of the output is written exactly once.
#ifndef MLA_LOGMEL_TIMELINE_CORE_H
#define MLA_LOGMEL_TIMELINE_CORE_H

#include <cstdint>

#include "logmel_bags_core.h"

namespace logmel_timeline {

constexpr int kWindowSlots = 10;                                            // T: slots per window (overlapping_split)
constexpr int kSlotStride = 32;                                             // columns between slots: (384 - 96) // 9
constexpr int kSlotCols = logmel_bags::kFrameLen;                           // 96
constexpr int kWindowCols = logmel_bags::kSpecCols;                         // 384
constexpr int kItemCols = logmel_bags::kItemCols;                           // 8
constexpr int kWindowItems = kWindowCols / kItemCols;                       // 48
constexpr int kMinSamples = 240;                                            // below: mel_features.py:42-45 raises
constexpr int64_t kWindowSamples = 15600 + 3 * 15360;                       // 61 680: all that four 0.96 s examples read
constexpr int64_t kSlotSamples = int64_t(kSlotStride) * logmel::kHop;       // 5 120 samples per slot of hop
constexpr int64_t kMaxCols = 0x7fffff00;                                    // columns, slots of one recording and q fit an int

// The per-recording descriptor, as five int64 on both sides. first_item is the prefix array of the item -> recording map.
struct Rec {
    int64_t first_slot;     // first output row of the recording
    int64_t cols;           // columns in the track: 32 q (W - 1) + 384
    int64_t spec_cols;      // columns that have a spectrum: cols for a long recording, 96 * examples for a short one
    int64_t first_item;     // items of the recordings before this one
    int64_t q;              // hop_slots
};
constexpr int kRecFields = 5;

MLA_HD int64_t windows_of(int64_t cols, int64_t q) { return (cols - kWindowCols) / (kSlotStride * q) + 1; }

// kept slots of a recording
MLA_HD int64_t slots_of(int64_t cols, int64_t q) {
    const int64_t W = windows_of(cols, q);
    return q <= kWindowSlots ? q * (W - 1) + kWindowSlots : kWindowSlots * W;
}

// items between the starts of two windows: the whole hop while windows touch or overlap (q <= 12), else one window's 48
MLA_HD int64_t step_items(int64_t q) { return q * (kSlotStride / kItemCols) < kWindowItems ? q * (kSlotStride / kItemCols) : kWindowItems; }

MLA_HD int64_t items_of(int64_t cols, int64_t q) { return step_items(q) * (windows_of(cols, q) - 1) + kWindowItems; }

// samples that the columns [0, spec_cols) read: none, or up to the end of the last 400-sample frame
MLA_HD int64_t samples_read(int64_t spec_cols) {
    return spec_cols <= 0 ? 0 : (spec_cols - 1) * int64_t(logmel::kHop) + logmel::kWin;
}

// first sample, relative to the recording's row, of column `col`
MLA_HD int64_t column_sample(int64_t col) { return col * int64_t(logmel::kHop); }

// The arithmetic of the header comment for a recording of n samples: false where n < 240 or q < 1 (nothing is written then).
MLA_HD bool counts(int64_t n, int64_t q, int64_t* windows, int64_t* slots, int64_t* cols, int64_t* spec_cols) {
    if (n < kMinSamples || q < 1) return false;
    if (n >= kWindowSamples) {
        const int64_t W = 1 + (n - kWindowSamples) / (kSlotSamples * q);
        *windows = W;
        *cols = kSlotStride * q * (W - 1) + kWindowCols;
        *spec_cols = *cols;
    } else {
        // whole 0.96 s examples (mla_logmel_counts): 1 + floor((frames - 96) / 96) with frames = 1 + floor((n - 400) / 160)
        const int64_t frames = n >= logmel::kWin ? 1 + (n - logmel::kWin) / logmel::kHop : 0;
        *windows = 1;
        *cols = kWindowCols;
        *spec_cols = (frames / kSlotCols) * kSlotCols;
    }
    *slots = slots_of(*cols, q);
    return true;
}

// the recording that holds `item`: the last r with rec[r].first_item <= item (binary search; 0 <= item < n_items)
MLA_HD int find_rec(const Rec* rec, int n_rec, int64_t item) {
    int lo = 0, hi = n_rec - 1;
    while (lo < hi) {
        const int mid = (lo + hi + 1) >> 1;
        if (rec[mid].first_item <= item) lo = mid; else hi = mid - 1;
    }
    return lo;
}

// item of a recording (0 <= local < items_of) -> its first column
MLA_HD int item_column(int local, int cols, int q) {
    const int step = int(step_items(q)), last = int(windows_of(cols, q)) - 1;
    int j = local / step;
    if (j > last) j = last;
    return kSlotStride * (q * j) + kItemCols * (local - step * j);          // q j <= (cols - 96) / 32: no overflow for any q
}

// The slots that can hold column `col` are u = col / 32 - 2 + i, i < 3 (kColumnSlots). Whether candidate i is a kept slot of the
// track, and if so its output row relative to first_slot and x = col - 32 u inside it. Slot starts are multiples of 32 and
// kItemCols divides 32, so the 8 columns of an item share their slots.
constexpr int kColumnSlots = kSlotCols / kSlotStride;                      // 3
MLA_HD bool column_slot(int col, int cols, int q, int i, int* row, int* x) {
    const int u_max = (cols - kSlotCols) / kSlotStride, u = col / kSlotStride - (kColumnSlots - 1) + i;
    if (u < 0 || u > u_max) return false;
    const int j = u / q, t = u - j * q;
    if (t >= kWindowSlots) return false;
    *row = q <= kWindowSlots ? u : kWindowSlots * j + t;
    *x = col - kSlotStride * u;
    return true;
}

// element offset of out[first_slot + row][band][x]
MLA_HD int64_t out_offset(int64_t first_slot, int row, int band, int x) {
    return ((first_slot + row) * logmel::kBands + band) * int64_t(kSlotCols) + x;
}

// One descriptor against the rows it reads and the prefixes before it. 0, or which check failed (host only: mla_logmel_timeline
// turns it into a message). A descriptor that passes reads no sample >= n_samples and writes rows [first_slot, first_slot + slots).
inline int check_rec(const Rec& r, int64_t n_samples, int64_t slot_prefix, int64_t item_prefix) {
    if (r.q < 1 || r.q > kMaxCols) return 1;
    if (r.cols < kWindowCols || r.cols > kMaxCols || (r.cols - kWindowCols) % (kSlotStride * r.q) != 0) return 2;
    const bool whole = r.spec_cols == r.cols;
    const bool ragged = r.cols == kWindowCols && r.spec_cols >= 0 && r.spec_cols < kWindowCols && r.spec_cols % kSlotCols == 0;
    if (!whole && !ragged) return 3;
    if (samples_read(r.spec_cols) > n_samples) return 4;
    if (r.first_slot != slot_prefix) return 5;
    if (r.first_item != item_prefix) return 6;
    return 0;
}

}  // namespace logmel_timeline
#endif
