// logmel_bags_core.h -- index arithmetic of the ragged log-mel + re-framing kernel (logmel_bags_kernel in logmel.hip), written so
// that the SAME source runs inside the kernel on gfx950 and on the host in csrc/logmel_bags_hostsim.cpp (built with g++ by the CPU
// tests). Reference: dataset.py:318-324 (create_spec, native path: <= 4 examples in 4 slots, missing slots 0.0, transposed and
// concatenated to (64, 384)) and :329-363 (split: n_frames windows of 96 columns at `stride`).
//
//   clip c, slot s < 4, frame f < 96  <->  column col = 96 s + f of the clip's (64, 384) spectrogram
//   out[c][t][band][x] = spec_c[band][t * stride + x],  t < n_frames, x < 96
//
// Work item = 8 consecutive columns (one wave-iteration of pair_step: 4 groups x 2 frames): 12 items per slot, 48 per clip, no
// prefix sums. An item of a slot the clip has (slot < counts[c]) computes its columns; any other stores 0.0 for them. Either way
// the item writes its 8 columns into every window that holds them, so each element of `out` is written exactly once.
#ifndef MLA_LOGMEL_BAGS_CORE_H
#define MLA_LOGMEL_BAGS_CORE_H

#include <cstdint>

#include "logmel_core.h"

namespace logmel_bags {

constexpr int kSlots = 4;                                    // dataset.py:321: np.zeros((4, 96, 64))
constexpr int kItemCols = 8;                                 // columns (STFT frames) per item
constexpr int kSlotItems = logmel::kExFrames / kItemCols;    // 12
constexpr int kClipItems = kSlots * kSlotItems;              // 48
constexpr int kSpecCols = kSlots * logmel::kExFrames;        // 384
constexpr int kFrameLen = logmel::kExFrames;                 // 96 columns per output frame
constexpr int kExampleSamples = logmel::kExFrames * logmel::kHop;                                   // 15 360 new samples per example
constexpr int kFirstExampleSamples = (logmel::kExFrames - 1) * logmel::kHop + logmel::kWin;        // 15 600

// the two configurations of the reference: overlapping_split (10 windows, stride (384 - 96) // 9 = 32) and contiguous_split
MLA_HD bool config_ok(int n_frames, int stride) { return (n_frames == 10 && stride == 32) || (n_frames == 4 && stride == 96); }

// samples of a row that `count` examples read: 15 600 + 15 360 (count - 1); none for an empty clip
MLA_HD int64_t samples_read(int count) { return count <= 0 ? 0 : int64_t(kFirstExampleSamples) + int64_t(kExampleSamples) * (count - 1); }

// item -> (clip, slot, first frame of the item inside the slot)
MLA_HD void item_locate(int item, int* clip, int* slot, int* frame) {
    const int c = item / kClipItems, r = item - c * kClipItems;
    *clip = c;
    *slot = r / kSlotItems;
    *frame = (r - *slot * kSlotItems) * kItemCols;
}

// first sample, relative to the clip's row, of frame `frame` of slot `slot`
MLA_HD int64_t frame_sample(int slot, int frame) { return int64_t(slot) * kExampleSamples + int64_t(frame) * logmel::kHop; }

MLA_HD int item_column(int slot, int frame) { return slot * kFrameLen + frame; }

// the windows t_lo .. t_hi (inclusive; none when t_lo > t_hi) that hold column `col`: t * stride <= col < t * stride + 96.
// Window starts are multiples of 32 and kItemCols divides 32, so the 8 columns of an item share their windows.
MLA_HD void column_windows(int col, int n_frames, int stride, int* t_lo, int* t_hi) {
    *t_lo = col < kFrameLen ? 0 : (col - kFrameLen) / stride + 1;
    const int hi = col / stride;
    *t_hi = hi < n_frames - 1 ? hi : n_frames - 1;
}

// element offset of out[clip][t][band][col - t * stride]
MLA_HD int64_t out_offset(int64_t clip, int n_frames, int stride, int t, int band, int col) {
    return ((clip * n_frames + t) * logmel::kBands + band) * int64_t(kFrameLen) + (col - t * stride);
}

}  // namespace logmel_bags
#endif
