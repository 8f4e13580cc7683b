// melspec_track_hostsim.cpp -- TEST HARNESS (never part of libmla_hip.so): the three track kernels of melspec.hip on the host, workgroup
// by workgroup in the kernels' own item space, with melspec_track_core.h's item / descriptor / offset arithmetic and melspec_core.h's
// per-thread phases in melspec_db_kernel's order (plain arrays standing in for LDS). Built with g++ by tests/test_melspec_track_cpu.py,
// which gives it write counters for every element of D and of the images and reads back the highest sample index each row was asked
// for: that every element is written exactly once and that nothing at or behind a track's end is read is checked without a GPU.
#include <cstdint>
#include <vector>

#include "melspec_core.h"
#include "melspec_tables.h"
#include "melspec_track_core.h"

using namespace melspec;
using melspec_track::Rec;

// pcm: (recordings, row_stride) floats; desc: (recordings, 6) int64 as mla_melspec_track_db takes them, total_runs their runs.
// D / d_writes: 224 * total columns; partial: total_runs; maxima: recordings; max_read[r]: highest sample index read in row r (-1: none).
// Returns the number of workgroups run, negative on bad arguments.
extern "C" int64_t hostsim_melspec_track_db(const float* pcm, int64_t recordings, int64_t row_stride, const int64_t* desc, int64_t total_runs,
                                            double sr, float amin, float* D, int32_t* d_writes, float* partial, float* maxima, int64_t* max_read) {
    const int n_mels = melspec_track::kMels, hop = melspec_track::kHop;
    if (recordings < 1 || !valid_config(sr, n_mels)) return -1;
    const Rec* recs = reinterpret_cast<const Rec*>(desc);
    std::vector<float> tab(table_floats(sr, n_mels));
    if (build_tables(sr, n_mels, tab.data()) != 0) return -1;
    std::vector<float> lds(lds_floats(n_mels));
    float* win = lds.data() + kLdsWin; float* tw = lds.data() + kLdsTw; float* stage = lds.data() + kLdsStage;
    float* zr = lds.data() + kLdsZr; float* zi = lds.data() + kLdsZi; float* pw = lds.data() + kLdsPw; float* tile = lds.data() + kLdsTile;
    const int* meta = reinterpret_cast<const int*>(tab.data() + kTabMeta);
    const float* weights = tab.data() + tab_weights(n_mels);
    for (int64_t r = 0; r < recordings; ++r) max_read[r] = -1;
    for (int64_t block = 0; block < total_runs; ++block) {                   // melspec_track_db_kernel, blockIdx.x = block
        const int rec = melspec_track::find_rec<&Rec::first_run>(recs, int(recordings), block);
        const Rec& r = recs[rec];
        const int n = int(r.samples), frames = int(r.cols);
        const int f0 = int(block - r.first_run) * kRunFrames;
        const int nf = frames - f0 < kRunFrames ? frames - f0 : kRunFrames;
        if (nf < 1) return -2;
        const float* row = pcm + rec * row_stride;
        const int count = kFft + (nf - 1) * hop;
        for (int i = 0; i < kFft + 2 * kTw; ++i) lds[i] = tab[i];
        for (int i = 0; i < count; ++i) {                                    // what stage_samples is about to read
            const int64_t at = reflect(f0 * hop + i, n);
            if (at < 0) return -3;
            if (at > max_read[rec]) max_read[rec] = at;
        }
        for (int t = 0; t < kThreads; ++t) stage_samples(t, row, n, f0 * hop, count, stage);
        float best = -INFINITY;
        for (int f = 0; f < nf; ++f) {
            for (int t = 0; t < kThreads; ++t) fft_first(t, stage + f * hop, win, zr, zi);
            for (int s = 1; s <= 4; ++s)
                for (int t = 0; t < kThreads; ++t) fft_stage(t, s, tw, zr, zi);
            for (int t = 0; t < kThreads; ++t) power(t, tw, zr, zi, pw);
            for (int t = 0; t < kThreads; ++t) best = mla::nan_max(best, mel_db(t, pw, meta, weights, n_mels, amin, f, tile));
        }
        for (int i = 0; i < n_mels * kRunFrames; ++i) {
            const int b = i / kRunFrames, f = i % kRunFrames;
            if (f < nf) {
                const int64_t at = melspec_track::db_index(r, b, f0 + f);
                D[at] = tile[i];
                ++d_writes[at];
            }
        }
        partial[block] = best;
    }
    for (int64_t block = 0; block < recordings; ++block) {                   // melspec_track_max_kernel
        const Rec& r = recs[block];
        float m = -INFINITY;
        for (int64_t i = 0; i < melspec_track::runs_of(r.cols); ++i) m = mla::nan_max(m, partial[r.first_run + i]);
        maxima[block] = m;
    }
    return total_runs;
}

// melspec_track_images_kernel for the rows [first, first + count): out / writes hold count * 224 * 224 elements. Returns the workgroups run.
extern "C" int64_t hostsim_melspec_track_images(const float* D, const float* maxima, int64_t recordings, const int64_t* desc, float top_db,
                                                int64_t first, int64_t count, float* out, int32_t* writes) {
    using namespace melspec_track;
    const Rec* recs = reinterpret_cast<const Rec*>(desc);
    for (int64_t block = 0; block < count * kImageBlocks; ++block) {
        for (int t = 0; t < kImageThreads; ++t) {
            const int64_t local = block / kImageBlocks, row = first + local;
            const int i = int(block - local * kImageBlocks) * kImageThreads + t;
            const int band = i / (kImageW / kImageVec), x = (i % (kImageW / kImageVec)) * kImageVec;
            const int rec = find_rec<&Rec::first_image>(recs, int(recordings), row);
            const Rec& r = recs[rec];
            const float lo = maxima[rec] - top_db;
            const float* src = D + db_index(r, band, image_column(row - r.first_image, r.q) + x);
            for (int k = 0; k < kImageVec; ++k) {
                const int64_t at = image_index(local, band, x + k);
                out[at] = mla::nan_max(src[k], lo);
                ++writes[at];
            }
        }
    }
    return count * kImageBlocks;
}
