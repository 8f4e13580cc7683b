// melspec_track_core.h -- index arithmetic of the ResNet branch's image timeline (melspec_track_db_kernel, melspec_track_max_kernel
// and melspec_track_images_kernel in melspec.hip), written so that the SAME source runs inside the kernels on gfx950, in their
// launchers' validation and on the host in csrc/melspec_track_hostsim.cpp (built with g++ by the CPU tests).
//
// A recording at 22 050 Hz with n samples is scored in windows of 88 200 samples (the reference's 4 s clip, dataset.py:233-237)
// that start q = hop_images >= 1 image steps apart. An image step is 75 spectrogram columns of hop 98 = 7 350 samples = 1/3 s.
//   n >= 88 200: W = 1 + (n - 88 200) / (7 350 q) windows; a trailing stretch that fills no window is dropped
//   n <  88 200: W = 1; the recording is zero-filled to 88 200 samples
// The TRACK of the recording is its first L = 88 200 + 7 350 q (W - 1) samples, centre-padded by reflection at ITS two ends, with
// C = 1 + L / 98 = 901 + 75 q (W - 1) columns D[band][c] = 10 log10(max(amin, mel power)) (melspec_core.h, unchanged). Image u is
// columns [75 u, 75 u + 224) floored at the track-wide maximum - top_db; it is kept iff u mod q < 10 and u <= q (W - 1) + 9, and kept
// images are stored in order of u:
//   q <= 10: q (W - 1) + 10 rows, window j = rows q j .. q j + 9;      q > 10: 10 W rows, window j = rows 10 j .. 10 j + 9
// Work item of the spectrogram = a run of up to 16 consecutive columns of ONE track; the runs of the whole batch form one item space
// and a descriptor's first_run is the prefix that maps an item back to its recording.
#ifndef MLA_MELSPEC_TRACK_CORE_H
#define MLA_MELSPEC_TRACK_CORE_H

#include <cstdint>

#include "melspec_core.h"

namespace melspec_track {

constexpr int kHop = 98;                                        // dataset.py:309-311 for 88 200 samples and 224 columns per image
constexpr int kMels = 224, kImageW = 224;                       // S_RESNET_SHAPE
constexpr int kImageStep = 75;                                  // (901 - 224) // 9: columns between images (dataset.py:355-359)
constexpr int kWindowImages = 10;                               // T
constexpr int64_t kWindowSamples = 88200;                       // SAMPLES_NUM_RESNET
constexpr int64_t kStepSamples = int64_t(kImageStep) * kHop;    // 7 350
constexpr int kWindowCols = 1 + int(kWindowSamples / kHop);     // 901
constexpr int64_t kMaxSamples = int64_t(1) << 30;               // melspec_core.h indexes a row's padded samples with int
constexpr int64_t kMaxHop = int64_t(1) << 30;
constexpr int kImageVec = 4;                                    // floats per store of the images kernel
constexpr int kImageThreads = 256;
constexpr int kImageBlocks = kMels * (kImageW / kImageVec) / kImageThreads;        // 49 workgroups per image, no tail
static_assert(kImageBlocks * kImageThreads * kImageVec == kMels * kImageW && kImageW % kImageVec == 0, "an image is whole workgroups");
static_assert(melspec::kFft + (melspec::kRunFrames - 1) * kHop <= melspec::kStage, "a run of 16 frames fits the staging buffer");

// The per-recording descriptor, as six int64 on both sides. first_run and first_image are the prefixes of the two item -> recording maps.
struct Rec {
    int64_t samples;        // L: samples of the track
    int64_t cols;           // C = 1 + L / 98
    int64_t first_run;      // runs of the recordings before this one
    int64_t db_offset;      // floats of D before this recording's (224, C) block: 224 * the columns before it
    int64_t first_image;    // kept images of the recordings before this one: its first row of the images
    int64_t q;              // hop_images
};
constexpr int kRecFields = 6;

MLA_MS_HD int64_t runs_of(int64_t cols) { return (cols + melspec::kRunFrames - 1) / melspec::kRunFrames; }
MLA_MS_HD int64_t windows_of(int64_t samples, int64_t q) { return 1 + (samples - kWindowSamples) / (kStepSamples * q); }
MLA_MS_HD int64_t images_of(int64_t samples, int64_t q) {
    const int64_t W = windows_of(samples, q);
    return q <= kWindowImages ? q * (W - 1) + kWindowImages : kWindowImages * W;
}

// The arithmetic of the header comment for a recording of n samples: false where n < 0 or q < 1.
MLA_MS_HD bool counts(int64_t n, int64_t q, int64_t* windows, int64_t* images, int64_t* samples, int64_t* cols) {
    if (n < 0 || q < 1 || q > kMaxHop) return false;
    const int64_t W = n >= kWindowSamples ? 1 + (n - kWindowSamples) / (kStepSamples * q) : 1;
    *windows = W;
    *samples = kWindowSamples + kStepSamples * q * (W - 1);
    *cols = 1 + *samples / kHop;
    *images = images_of(*samples, q);
    return true;
}

// the recording that holds item `v` of the prefix F: the last r with rec[r].*F <= v (binary search; 0 <= v < the prefix's total)
template <int64_t Rec::*F>
MLA_MS_HD int find_rec(const Rec* rec, int n_rec, int64_t v) {
    int lo = 0, hi = n_rec - 1;
    while (lo < hi) {
        const int mid = (lo + hi + 1) >> 1;
        if (rec[mid].*F <= v) lo = mid; else hi = mid - 1;
    }
    return lo;
}

// kept image k of a recording (0 <= k < images_of) -> its first column 75 u
MLA_MS_HD int image_column(int64_t k, int64_t q) {
    const int64_t u = q <= kWindowImages ? k : (k / kWindowImages) * q + k % kWindowImages;
    return int(u * kImageStep);
}

// element offset of D_r[band][col] in the flat D, and of out[row][0][band][x] relative to the first row of a launch
MLA_MS_HD int64_t db_index(const Rec& r, int band, int64_t col) { return r.db_offset + int64_t(band) * r.cols + col; }
MLA_MS_HD int64_t image_index(int64_t row, int band, int x) { return (row * kMels + band) * int64_t(kImageW) + x; }

// One descriptor against the rows it reads and the prefixes before it. 0, or which check failed (host only: the launchers turn it
// into a message). A descriptor that passes reads no sample >= min(samples, n_samples), writes the runs [first_run, first_run +
// runs_of(cols)), the floats [db_offset, db_offset + 224 cols) of D and the image rows [first_image, first_image + images_of), and
// every kept image lies inside its columns.
inline int check_rec(const Rec& r, int64_t n_samples, int64_t run_prefix, int64_t col_prefix, int64_t image_prefix) {
    if (r.q < 1 || r.q > kMaxHop) return 1;
    if (r.samples < kWindowSamples || r.samples > kMaxSamples || (r.samples - kWindowSamples) % (kStepSamples * r.q) != 0) return 2;
    if (r.cols != 1 + r.samples / kHop) return 3;
    if (r.samples > n_samples) return 4;
    if (r.first_run != run_prefix) return 5;
    if (r.db_offset != col_prefix * kMels) return 6;
    if (r.first_image != image_prefix) return 7;
    return 0;
}

}  // namespace melspec_track
#endif
