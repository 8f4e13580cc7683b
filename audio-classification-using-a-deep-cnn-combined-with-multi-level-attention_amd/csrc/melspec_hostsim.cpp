// melspec_hostsim.cpp -- TEST HARNESS (never part of libmla_hip.so): runs melspec_core.h's per-thread phases on the
// host exactly as melspec_db_kernel orders them (all 256 threads of a phase, then the next phase), with plain arrays
// standing in for LDS. Built with g++ by tests/test_melspec_cpu.py to check the reflect / FFT / real-split / sparse-mel
// index arithmetic and the tables against the float64 restatement without a GPU.
#include <cstdint>
#include <vector>

#include "melspec_core.h"
#include "melspec_tables.h"

using namespace melspec;

extern "C" int64_t hostsim_melspec_table_floats(double sr, int64_t n_mels) { return table_floats(sr, n_mels); }
extern "C" int hostsim_melspec_build_tables(double sr, int64_t n_mels, float* tab) { return build_tables(sr, n_mels, tab); }

// pcm: n floats; out: (n_mels, frames) unclipped dB, frames = 1 + n / hop. Returns frames, negative on bad arguments.
extern "C" int64_t hostsim_melspec_db(const float* pcm, int64_t n, int64_t hop, double sr, int64_t n_mels, float amin, float* out) {
    if (n < kMinSamples || hop < 1 || !valid_config(sr, n_mels)) return -1;
    std::vector<float> tab(table_floats(sr, n_mels));
    if (build_tables(sr, n_mels, tab.data()) != 0) return -1;
    const int frames = int(1 + n / hop), per = run_frames(hop);
    std::vector<float> lds(lds_floats(int(n_mels)));
    float* win = lds.data() + kLdsWin; float* tw = lds.data() + kLdsTw; float* stage = lds.data() + kLdsStage;
    float* zr = lds.data() + kLdsZr; float* zi = lds.data() + kLdsZi; float* pw = lds.data() + kLdsPw; float* tile = lds.data() + kLdsTile;
    const int* meta = reinterpret_cast<const int*>(tab.data() + kTabMeta);
    const float* weights = tab.data() + tab_weights(int(n_mels));
    for (int i = 0; i < kFft + 2 * kTw; ++i) lds[i] = tab[i];
    for (int f0 = 0; f0 < frames; f0 += per) {
        const int nf = frames - f0 < per ? frames - f0 : per;
        for (int t = 0; t < kThreads; ++t) stage_samples(t, pcm, int(n), int(f0 * hop), int(kFft + (nf - 1) * hop), stage);
        for (int f = 0; f < nf; ++f) {
            for (int t = 0; t < kThreads; ++t) fft_first(t, stage + f * hop, win, zr, zi);
            for (int s = 1; s <= 4; ++s)
                for (int t = 0; t < kThreads; ++t) fft_stage(t, s, tw, zr, zi);
            for (int t = 0; t < kThreads; ++t) power(t, tw, zr, zi, pw);
            for (int t = 0; t < kThreads; ++t) mel_db(t, pw, meta, weights, int(n_mels), amin, f, tile);
        }
        for (int i = 0; i < n_mels * kRunFrames; ++i) {
            const int b = i / kRunFrames, f = i % kRunFrames;
            if (f < nf) out[int64_t(b) * frames + f0 + f] = tile[i];
        }
    }
    return frames;
}
