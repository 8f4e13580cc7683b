// melspec_wave_hostsim.cpp -- TEST HARNESS (never part of libmla_hip.so): runs melspec_wave_core.h's per-lane phases on the
// host exactly as melspec_nopad_db_kernel orders them, with plain arrays standing in for LDS: per run the staging pass of all
// 256 threads, then round by round the four waves' frames, each wave all 64 lanes of a phase before the next phase. A lane
// that read what another lane of its phase had already overwritten would show here as a wrong value. Built with g++ by
// tests/test_melspec_htk_cpu.py.
#include <cstdint>
#include <vector>

#include "melspec_tables.h"
#include "melspec_wave_core.h"

using namespace melspec;

// pcm: n floats; out: (n_mels, frames) unclipped dB, frames = 1 + (n - 2048) / hop. Returns frames, negative on bad arguments.
extern "C" int64_t hostsim_melspec_nopad_db(const float* pcm, int64_t n, int64_t hop, double sr, int64_t n_mels, double fmin, double fmax,
                                            int htk, float amin, float* out) {
    const MelConfig cfg{sr, n_mels, fmin, fmax, htk != 0};
    const int64_t frames = nopad_frames(n, hop), floats = table_floats(cfg);
    if (frames < 0 || floats < 0) return -1;
    std::vector<float> tab(floats);
    if (build_tables(cfg, tab.data()) != 0) return -1;
    const int nnz = int(floats - tab_weights(int(n_mels))), per = wave_run_frames(hop), rounds = (per + kWaves - 1) / kWaves;
    if (nnz > kMaxWeights) return -1;
    std::vector<float> lds(wave_lds_floats(int(n_mels), nnz));
    float* win = lds.data() + kLdsWin; float* tw = lds.data() + kLdsTw; float* stage = lds.data() + kLdsStage;
    float* wts = lds.data() + kWLdsWeights; float* tile = lds.data() + wave_lds_tile(nnz);
    const int* meta = reinterpret_cast<const int*>(tab.data() + kTabMeta);
    for (int i = 0; i < kFft + 2 * kTw; ++i) lds[i] = tab[i];
    for (int i = 0; i < nnz; ++i) wts[i] = tab[tab_weights(int(n_mels)) + i];
    for (int64_t f0 = 0; f0 < frames; f0 += per) {
        const int nf = frames - f0 < per ? int(frames - f0) : per;
        for (int t = 0; t < kThreads; ++t) stage_plain(t, pcm, f0 * hop, int(kFft + (nf - 1) * hop), stage);
        for (int r = 0; r < rounds; ++r)
            for (int w = 0; w < kWaves; ++w) {
                const int f = r * kWaves + w;
                if (f >= nf) continue;                                       // an idle frame of the last run
                float* z = lds.data() + kWLdsFft + w * kWaveFft;
                for (int l = 0; l < kWave; ++l) wave_fft_first(l, stage + f * hop, win, z);
                for (int s = 1; s <= 4; ++s)
                    for (int l = 0; l < kWave; ++l) wave_fft_stage(l, s, tw, z);
                for (int l = 0; l < kWave; ++l) power_in_place(l, tw, z);
                for (int l = 0; l < kWave; ++l) wave_mel_db(l, z, meta, wts, int(n_mels), amin, f, tile);
            }
        for (int i = 0; i < n_mels * kRunFrames; ++i) {
            const int b = i / kRunFrames, f = i % kRunFrames;
            if (f < nf) out[int64_t(b) * frames + f0 + f] = tile[i];
        }
    }
    return frames;
}
