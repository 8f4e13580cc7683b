// melspec_wave_core.h -- per-lane arithmetic of the mel-dB spectrogram of UNPADDED frames (center=False: the VGGish
// branch's librosa path, dataset.py:305-307, :316 of the reference), one wavefront per frame. Like melspec_core.h the
// SAME source runs (a) inside melspec.hip on gfx950 and (b) on the host, lane by lane and phase by phase, in
// csrc/melspec_wave_hostsim.cpp. A "phase" here is what the 64 lanes of ONE wave do between two wave-level
// synchronisations; the four waves of a workgroup work on four different frames and never exchange FFT data.
//
// Frame f of a clip is y[f * hop .. f * hop + 2047], no padding, frames = 1 + (n - 2048) / hop. The arithmetic is
// melspec_core.h's: a lane plays threads lane, lane + 64, lane + 128, lane + 192 of fft_first / fft_stage (a thread
// touches only its own four positions within a stage, so the order among them is free: all loads, then all stores), then
//   power_in_place  lane l: the bin pairs (k, 1024 - k), k = l, l + 64, ... < 512 (lane 0 also k = 512). Both powers
//                   of a pair need Z[k] and Z[1024 - k] and nothing else, so they are computed first and then written
//                   over zr[k] and zr[1024 - k]; P[1024] (paired with k = 0) goes to zr[1024] = zi[0], which only the
//                   pair k = 0 reads. After the phase zr[0 .. 1024] is what melspec_core.h calls pw.
//   wave_mel_db     lane l: bands l, l + 64, ... (with 64 bands: one lane per band)
#ifndef MLA_MELSPEC_WAVE_CORE_H
#define MLA_MELSPEC_WAVE_CORE_H

#include "melspec_core.h"

namespace melspec {

constexpr int kWave = 64, kWaves = kThreads / kWave;
constexpr int kMaxWeights = 2 * kBins;      // a bin lies inside at most two triangles of a mel basis
constexpr int kWaveFft = 2 * kHalf;         // floats of one wave's FFT buffer: zr then zi, contiguous (zr[1024] is zi[0])

MLA_MS_HD int64_t nopad_frames(int64_t n, int64_t hop) { return n < kFft || hop < 1 ? -1 : 1 + (n - kFft) / hop; }

// frames a workgroup owns: what the staging buffer holds, cut to a multiple of the four waves so that no round is part idle
// inside a clip (13 -> 12 at hop 160); below four the run is one round with idle waves
MLA_MS_HD int wave_run_frames(int64_t hop) {
    const int f = run_frames(hop);
    return f >= kWaves ? f - f % kWaves : f;
}

// LDS layout of one workgroup (float indices): window, twiddles and the run's samples as in melspec_core.h, then the four
// waves' FFT buffers, the packed mel weights and the (band, frame in run) tile
constexpr int kWLdsFft = kLdsStage + kStage, kWLdsWeights = kWLdsFft + kWaves * kWaveFft;
MLA_MS_HD int wave_lds_tile(int nnz) { return kWLdsWeights + ((nnz + 3) & ~3); }
MLA_MS_HD int wave_lds_floats(int n_mels, int nnz) { return wave_lds_tile(nnz) + n_mels * kRunFrames; }

// the run's samples: row[p0 .. p0 + count), all inside the row
MLA_MS_HD void stage_plain(int t, const float* row, int64_t p0, int count, float* stage) {
    for (int i = t; i < count; i += kThreads) stage[i] = row[p0 + i];
}

// A lane's four butterflies of a stage touch sixteen different positions, so all their loads are issued before the first
// store: one LDS round trip per stage instead of four (the compiler cannot prove that a store of one butterfly does not feed a
// load of the next and would keep them in program order). Same arithmetic as fft_first / fft_stage, value for value.
MLA_MS_HD void wave_fft_first(int lane, const float* x, const float* win, float* z) {
    float ar[kWaves][4], ai[kWaves][4], yr[4], yi[4];
    for (int j = 0; j < kWaves; ++j) {
        const int r = rev4(lane + kWave * j);
        for (int q = 0; q < 4; ++q) {
            const int m = 256 * q + r;
            ar[j][q] = x[2 * m] * win[2 * m];
            ai[j][q] = x[2 * m + 1] * win[2 * m + 1];
        }
    }
    for (int j = 0; j < kWaves; ++j) {
        const int t = lane + kWave * j;
        radix4(ar[j], ai[j], yr, yi);
        for (int q = 0; q < 4; ++q) { z[4 * t + q] = yr[q]; z[kHalf + 4 * t + q] = yi[q]; }
    }
}

MLA_MS_HD void wave_fft_stage(int lane, int s, const float* tw, float* z) {
    const int L = 1 << (2 * s), step = 512 >> (2 * s);
    float vr[kWaves][4], vi[kWaves][4], wr[kWaves][4], wi[kWaves][4];
    for (int j = 0; j < kWaves; ++j) {
        const int t = lane + kWave * j, pos = t & (L - 1), base = ((t >> (2 * s)) << (2 * s + 2)) + pos;
        for (int q = 0; q < 4; ++q) { vr[j][q] = z[base + q * L]; vi[j][q] = z[kHalf + base + q * L]; }
        for (int q = 1; q < 4; ++q) { wr[j][q] = tw[2 * (pos * q * step)]; wi[j][q] = tw[2 * (pos * q * step) + 1]; }
    }
    for (int j = 0; j < kWaves; ++j) {
        const int t = lane + kWave * j, pos = t & (L - 1), base = ((t >> (2 * s)) << (2 * s + 2)) + pos;
        float ar[4], ai[4], yr[4], yi[4];
        ar[0] = vr[j][0]; ai[0] = vi[j][0];
        for (int q = 1; q < 4; ++q) {
            ar[q] = vr[j][q] * wr[j][q] - vi[j][q] * wi[j][q];
            ai[q] = vr[j][q] * wi[j][q] + vi[j][q] * wr[j][q];
        }
        radix4(ar, ai, yr, yi);
        for (int q = 0; q < 4; ++q) { z[base + q * L] = yr[q]; z[kHalf + base + q * L] = yi[q]; }
    }
}

// mel_db for one wave: bands lane, lane + 64, ...; the same fmaf chain in ascending bins, with the loads of four bins issued
// together so that the chain does not wait for one LDS round trip per bin
MLA_MS_HD float wave_mel_db(int lane, const float* pw, const int* meta, const float* weights, int n_mels, float amin, int f, float* tile) {
    float best = -INFINITY;
    for (int b = lane; b < n_mels; b += kWave) {
        const int first = meta[3 * b], bins = meta[3 * b + 1];
        const float* w = weights + meta[3 * b + 2];
        const float* p = pw + first;
        float acc = 0.f;
        int i = 0;
        for (; i + 4 <= bins; i += 4) {
            const float w0 = w[i], w1 = w[i + 1], w2 = w[i + 2], w3 = w[i + 3];
            const float p0 = p[i], p1 = p[i + 1], p2 = p[i + 2], p3 = p[i + 3];
            acc = fmaf(w0, p0, acc); acc = fmaf(w1, p1, acc); acc = fmaf(w2, p2, acc); acc = fmaf(w3, p3, acc);
        }
        for (; i < bins; ++i) acc = fmaf(w[i], p[i], acc);
        const float d = 10.0f * log10f(mla::nan_max(amin, acc));
        tile[b * kRunFrames + f] = d;
        best = mla::nan_max(best, d);
    }
    return best;
}

MLA_MS_HD void power_in_place(int lane, const float* tw, float* z) {
    const float* zr = z;
    const float* zi = z + kHalf;
    for (int k0 = lane; k0 < kHalf / 2; k0 += 4 * kWave) {      // four disjoint pairs at a time: their loads before their stores
        float lo[4], hi[4];
        for (int j = 0; j < 4; ++j) {
            const int k = k0 + kWave * j;
            lo[j] = power_bin(k, tw, zr, zi);
            hi[j] = power_bin(kHalf - k, tw, zr, zi);
        }
        for (int j = 0; j < 4; ++j) {
            const int k = k0 + kWave * j;
            z[k] = lo[j];
            z[kHalf - k] = hi[j];
        }
    }
    if (lane == 0) z[kHalf / 2] = power_bin(kHalf / 2, tw, zr, zi);
}

}  // namespace melspec
#endif
