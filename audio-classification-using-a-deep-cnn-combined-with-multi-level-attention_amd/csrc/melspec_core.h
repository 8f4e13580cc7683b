// melspec_core.h -- per-thread arithmetic of the batched power mel-dB spectrogram (the ResNet branch's front-end:
// librosa.feature.melspectrogram + power_to_db as the reference calls them, dataset.py:309-316), written so that the
// SAME source runs (a) inside melspec.hip on gfx950 and (b) on the host, thread by thread and phase by phase, in
// csrc/melspec_hostsim.cpp (built with g++ by the CPU tests), with plain arrays standing in for LDS. A "phase" is
// what one of the workgroup's 256 threads does between two barriers.
//
// One STFT frame f of a clip of n samples (n_fft = win_length = 2048, centre padding 1024, reflect):
//   x[i] = y[reflect(f * hop + i - 1024)] * hann[i],  i < 2048
//   z[m] = x[2m] + i x[2m+1], m < 1024                 (real FFT through a half-size complex FFT)
//   Z = FFT1024(z): five radix-4 decimation-in-time stages, in place, on the base-4 digit-reversed input
//     fft_first   thread t loads z[256 q + rev4(t)], q < 4 (window applied), butterflies without twiddles,
//                 writes positions 4t + q
//     fft_stage   s = 1..4, L = 4^s: thread t owns positions base + q L, base = (t / L) 4L + t % L, multiplies
//                 by W_4L^(q (t % L)) and butterflies; every thread reads and writes only its own four positions
//   X[k] = (Z[k] + conj Z[1024-k]) / 2 - i W_2048^k (Z[k] - conj Z[1024-k]) / 2,  k <= 1024;  P[k] = |X[k]|^2
//     power       thread t: k = t, t + 256, ... (thread 0 also k = 1024)
//   S[b] = sum_k M[b][k] P[k] over the band's non-zero bins only, in ascending k, one fmaf chain per band
//   D[b] = 10 log10(max(amin, S[b]))        (max keeps NaN, as np.maximum does: nanprop.h)
//     mel_db      thread t: bands t, t + 256, ...; writes tile[b][frame in run], returns its maximum
#ifndef MLA_MELSPEC_CORE_H
#define MLA_MELSPEC_CORE_H

#include <cmath>
#include <cstdint>

#include "nanprop.h"

#if defined(__HIPCC__)
#define MLA_MS_HD __host__ __device__ __forceinline__
#else
#define MLA_MS_HD inline
#endif

namespace melspec {

constexpr int kFft = 2048, kHalf = 1024, kBins = 1025, kPad = 1024;
constexpr int kThreads = 256;
constexpr int kRunFrames = 16;             // frames per workgroup: 16 consecutive f32 of one band = one 64-byte store run
constexpr int kStage = 4096;               // staged padded samples per run: 2048 + (F - 1) * hop must fit
constexpr int kTw = 1536;                  // W_2048^k, k < 1536: the split needs k <= 1024, the stages 2 * 3 * 255 = 1530
constexpr int kMaxMels = 1024;
constexpr int kMinSamples = kPad + 1;      // a single reflection covers the padding only when n > 1024

// table layout (float indices); the mel part depends on (sr, n_mels)
constexpr int kTabWindow = 0;              // 2048 floats: periodic Hann
constexpr int kTabTw = kFft;               // kTw x (cos, -sin)(2 pi k / 2048)
constexpr int kTabMeta = kTabTw + 2 * kTw; // n_mels x (first bin, bins, offset into the packed weights), int32
MLA_MS_HD int tab_weights(int n_mels) { return kTabMeta + 3 * n_mels; }

// frames a workgroup owns for this hop: the run's samples must fit the staging buffer
MLA_MS_HD int run_frames(int64_t hop) {
    const int64_t f = 1 + (kStage - kFft) / hop;
    return f < kRunFrames ? int(f) : kRunFrames;
}

// padded index p in [0, n + 2048) -> index into the clip, numpy's pad_mode="reflect"
MLA_MS_HD int reflect(int p, int n) {
    const int j = p - kPad;
    return j < 0 ? -j : j >= n ? 2 * (n - 1) - j : j;
}

// LDS layout of one workgroup (float indices)
constexpr int kLdsWin = 0, kLdsTw = kLdsWin + kFft, kLdsStage = kLdsTw + 2 * kTw, kLdsZr = kLdsStage + kStage,
              kLdsZi = kLdsZr + kHalf, kLdsPw = kLdsZi + kHalf, kLdsTile = kLdsPw + kBins + 3;
MLA_MS_HD int lds_floats(int n_mels) { return kLdsTile + n_mels * kRunFrames; }

MLA_MS_HD void stage_samples(int t, const float* row, int n, int p0, int count, float* stage) {
    for (int i = t; i < count; i += kThreads) stage[i] = row[reflect(p0 + i, n)];
}

MLA_MS_HD int rev4(int t) { return ((t & 3) << 6) | ((t & 12) << 2) | ((t & 48) >> 2) | ((t & 192) >> 6); }

// y_r = sum_q (-i)^(q r) a_q
MLA_MS_HD void radix4(const float* ar, const float* ai, float* yr, float* yi) {
    const float s02r = ar[0] + ar[2], s02i = ai[0] + ai[2], d02r = ar[0] - ar[2], d02i = ai[0] - ai[2];
    const float s13r = ar[1] + ar[3], s13i = ai[1] + ai[3], d13r = ar[1] - ar[3], d13i = ai[1] - ai[3];
    yr[0] = s02r + s13r; yi[0] = s02i + s13i;
    yr[1] = d02r + d13i; yi[1] = d02i - d13r;          // -i (a1 - a3) = (d13i, -d13r)
    yr[2] = s02r - s13r; yi[2] = s02i - s13i;
    yr[3] = d02r - d13i; yi[3] = d02i + d13r;
}

MLA_MS_HD void fft_first(int t, const float* x, const float* win, float* zr, float* zi) {
    const int r = rev4(t);
    float ar[4], ai[4], yr[4], yi[4];
    for (int q = 0; q < 4; ++q) {
        const int m = 256 * q + r;
        ar[q] = x[2 * m] * win[2 * m];
        ai[q] = x[2 * m + 1] * win[2 * m + 1];
    }
    radix4(ar, ai, yr, yi);
    for (int q = 0; q < 4; ++q) { zr[4 * t + q] = yr[q]; zi[4 * t + q] = yi[q]; }
}

MLA_MS_HD void fft_stage(int t, int s, const float* tw, float* zr, float* zi) {
    const int L = 1 << (2 * s), pos = t & (L - 1), base = ((t >> (2 * s)) << (2 * s + 2)) + pos, step = 512 >> (2 * s);
    float ar[4], ai[4], yr[4], yi[4];
    ar[0] = zr[base]; ai[0] = zi[base];
    for (int q = 1; q < 4; ++q) {
        const float vr = zr[base + q * L], vi = zi[base + q * L];
        const float wr = tw[2 * (pos * q * step)], wi = tw[2 * (pos * q * step) + 1];
        ar[q] = vr * wr - vi * wi;
        ai[q] = vr * wi + vi * wr;
    }
    radix4(ar, ai, yr, yi);
    for (int q = 0; q < 4; ++q) { zr[base + q * L] = yr[q]; zi[base + q * L] = yi[q]; }
}

MLA_MS_HD float power_bin(int k, const float* tw, const float* zr, const float* zi) {
    const int a = k & (kHalf - 1), b = (kHalf - k) & (kHalf - 1);
    const float er = 0.5f * (zr[a] + zr[b]), ei = 0.5f * (zi[a] - zi[b]);       // (Z[k] + conj Z[N-k]) / 2
    const float orr = 0.5f * (zi[a] + zi[b]), oi = -0.5f * (zr[a] - zr[b]);     // -i (Z[k] - conj Z[N-k]) / 2
    const float wr = tw[2 * k], wi = tw[2 * k + 1];
    const float xr = er + (wr * orr - wi * oi), xi = ei + (wr * oi + wi * orr);
    return xr * xr + xi * xi;
}

MLA_MS_HD void power(int t, const float* tw, const float* zr, const float* zi, float* pw) {
    for (int k = t; k < kHalf; k += kThreads) pw[k] = power_bin(k, tw, zr, zi);
    if (t == 0) pw[kHalf] = power_bin(kHalf, tw, zr, zi);
}

// returns the largest dB value this thread wrote (-inf if it owns no band)
MLA_MS_HD float mel_db(int t, const float* pw, const int* meta, const float* weights, int n_mels, float amin, int f, float* tile) {
    float best = -INFINITY;
    for (int b = t; b < n_mels; b += kThreads) {
        const int first = meta[3 * b], bins = meta[3 * b + 1];
        const float* w = weights + meta[3 * b + 2];
        float acc = 0.f;
        for (int i = 0; i < bins; ++i) acc = fmaf(w[i], pw[first + i], acc);
        const float d = 10.0f * log10f(mla::nan_max(amin, acc));
        tile[b * kRunFrames + f] = d;
        best = mla::nan_max(best, d);
    }
    return best;
}

}  // namespace melspec
#endif
