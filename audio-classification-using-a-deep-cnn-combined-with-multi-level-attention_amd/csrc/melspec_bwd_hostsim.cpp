// melspec_bwd_hostsim.cpp -- TEST HARNESS (never part of libmla_hip.so): runs every workgroup of melspec_images_bwd_kernel,
// melspec_db_bwd_kernel and melspec_fold_kernel on the host in the kernels' order -- workgroup by workgroup (ascending, or
// descending with order = 1: no workgroup depends on another), per workgroup phase by phase, every thread of a phase before the
// next phase -- through the functions of melspec_bwd_core.h the kernels use, with plain arrays standing in for LDS. Built with
// g++ -ffp-contract=off by tests/test_melspec_bwd_cpu.py. Every store to d_db and d_pcm also counts in `writes`, and the highest
// element read of each input is kept, so the test can show that each element is written exactly once and that no input is read
// outside its rows. hostsim_melspec_fwd is the forward (melspec_core.h as melspec_db_kernel orders it) with its partial maxima.
#include <cstdint>
#include <vector>

#include "melspec_bwd_core.h"
#include "melspec_tables.h"

using namespace melspec_bwd;

namespace {
struct CountingReader {
    const float* p;
    int64_t* max_read;
    float operator()(int64_t i) const {
        if (i > *max_read) *max_read = i;
        return p[i];
    }
};
struct CountingWriter {
    float* p;
    int32_t* writes;
    void operator()(int64_t i, float v) const {
        p[i] = v;
        ++writes[i];
    }
};
}  // namespace

extern "C" int hostsim_melspec_bwd_run_frames(int64_t hop) { return bwd_run_frames(hop); }
extern "C" int64_t hostsim_melspec_bwd_runs(int64_t n, int64_t hop) { return bwd_runs(n, hop); }
extern "C" int hostsim_melspec_bwd_span(int64_t hop) { return bwd_span(hop); }
extern "C" int hostsim_melspec_bwd_lds_bytes(void) { return kBLdsFloats * int(sizeof(float)); }
extern "C" int64_t hostsim_melspec_fwd_runs(int64_t n, int64_t hop) { return (1 + n / hop + run_frames(hop) - 1) / run_frames(hop); }

// pcm: clips rows of n floats at `stride`; D: (clips, n_mels, frames); partial: (clips, forward runs). Returns frames.
extern "C" int64_t hostsim_melspec_fwd(const float* pcm, int64_t clips, int64_t n, int64_t stride, int64_t hop, double sr, int64_t n_mels,
                                       float amin, float* D, float* partial) {
    if (n < kMinSamples || hop < 1 || stride < n || !valid_config(sr, n_mels)) return -1;
    std::vector<float> tab(table_floats(sr, n_mels));
    if (build_tables(sr, n_mels, tab.data()) != 0) return -1;
    const int frames = int(1 + n / hop), per = run_frames(hop), runs = (frames + per - 1) / per;
    std::vector<float> lds(lds_floats(int(n_mels)));
    float* win = lds.data() + kLdsWin; float* tw = lds.data() + kLdsTw; float* stage = lds.data() + kLdsStage;
    float* zr = lds.data() + kLdsZr; float* zi = lds.data() + kLdsZi; float* pw = lds.data() + kLdsPw; float* tile = lds.data() + kLdsTile;
    const int* meta = reinterpret_cast<const int*>(tab.data() + kTabMeta);
    const float* weights = tab.data() + tab_weights(int(n_mels));
    for (int i = 0; i < kFft + 2 * kTw; ++i) lds[i] = tab[i];
    for (int64_t c = 0; c < clips; ++c)
        for (int run = 0; run < runs; ++run) {
            const int f0 = run * per, nf = frames - f0 < per ? frames - f0 : per;
            float best = -INFINITY;
            for (int t = 0; t < kThreads; ++t) stage_samples(t, pcm + c * stride, int(n), int(f0 * hop), int(kFft + (nf - 1) * hop), stage);
            for (int f = 0; f < nf; ++f) {
                for (int t = 0; t < kThreads; ++t) fft_first(t, stage + f * hop, win, zr, zi);
                for (int s = 1; s <= 4; ++s)
                    for (int t = 0; t < kThreads; ++t) fft_stage(t, s, tw, zr, zi);
                for (int t = 0; t < kThreads; ++t) power(t, tw, zr, zi, pw);
                for (int t = 0; t < kThreads; ++t) best = mla::nan_max(best, mel_db(t, pw, meta, weights, int(n_mels), amin, f, tile));
            }
            for (int i = 0; i < n_mels * kRunFrames; ++i) {
                const int b = i / kRunFrames, f = i % kRunFrames;
                if (f < nf) D[(c * n_mels + b) * frames + f0 + f] = tile[i];
            }
            partial[c * runs + run] = best;
        }
    return frames;
}

// g: (clips, n_images, 1, n_mels, image_w); D / d_db / writes: (clips, n_mels, frames); partial as hostsim_melspec_fwd left it.
// max_read[2]: highest element read of g and of D (-1: none). Returns 0, negative for bad arguments.
extern "C" int hostsim_melspec_images_bwd(const float* g, const float* D, const float* partial, int64_t clips, int64_t n, int64_t hop,
                                          int64_t n_mels, float top_db, int64_t n_images, int64_t image_w, int64_t stride, int floor_grad,
                                          int order, float* d_db, int32_t* writes, int64_t* max_read) {
    if (clips < 0 || n < kMinSamples || hop < 1 || n_mels < 1 || n_images < 1 || image_w < 1 || stride < 0) return -1;
    const int frames = int(1 + n / hop), fwd_runs = int(hostsim_melspec_fwd_runs(n, hop));
    if ((n_images - 1) * stride + image_w > frames) return -2;
    max_read[0] = max_read[1] = -1;
    const Images s{int(n_mels), frames, int(n_images), int(image_w), int(stride)};
    const CountingReader gr{g, &max_read[0]}, dr{D, &max_read[1]};
    const CountingWriter out{d_db, writes};
    std::vector<float> red(kImgThreads);
    std::vector<int64_t> cell(kImgThreads);
    for (int64_t wg = 0; wg < clips; ++wg) {
        const int64_t clip = order ? clips - 1 - wg : wg;
        for (int tid = 0; tid < kImgThreads; ++tid) red[tid] = max_partial(tid, partial + clip * fwd_runs, fwd_runs);
        for (int st = kImgThreads / 2; st > 0; st >>= 1)
            for (int tid = 0; tid < kImgThreads; ++tid) max_step(tid, st, red.data());
        const float m = red[0], floor = m - top_db;
        const int64_t g_clip = clip * n_images * n_mels * image_w, d_clip = clip * n_mels * frames;
        for (int tid = 0; tid < kImgThreads; ++tid) red[tid] = images_phase1(tid, gr, g_clip, dr, out, d_clip, s, m, floor, &cell[tid]);
        for (int st = kImgThreads / 2; st > 0; st >>= 1)
            for (int tid = 0; tid < kImgThreads; ++tid) sum_step(tid, st, red.data(), cell.data());
        const float term = floor_grad ? red[0] : 0.f;
        const int64_t first = cell[0];
        for (int tid = 0; tid < kImgThreads; ++tid) images_phase2(tid, gr, g_clip, dr, out, d_clip, s, m, floor, term, first);
    }
    return 0;
}

// pcm: clips rows at `stride`; d_db: (clips, n_mels, frames); ws: clips * runs * span floats; d_pcm / writes: clips rows at d_stride
// (writes zeroed by the caller). fold_threads: threads per workgroup of the fold (0 = the launcher's). max_read[2]: highest element
// read of pcm and of d_db.
extern "C" int hostsim_melspec_db_bwd(const float* pcm, int64_t clips, int64_t n, int64_t stride, int64_t hop, double sr, int64_t n_mels,
                                      float amin, const float* d_db, int order, int fold_threads, float* ws, float* d_pcm, int64_t d_stride,
                                      int32_t* writes, int64_t* max_read) {
    if (clips < 0 || n < kMinSamples || n > (1 << 30) || hop < 1 || stride < n || d_stride < n || !valid_config(sr, n_mels)) return -1;
    std::vector<float> tabv(table_floats(sr, n_mels));
    if (build_tables(sr, n_mels, tabv.data()) != 0) return -1;
    const float* tab = tabv.data();
    max_read[0] = max_read[1] = -1;
    const Runs r = runs_for(n, hop < (1 << 30) ? hop : (1 << 30));
    const int* meta = reinterpret_cast<const int*>(tab + kTabMeta);
    const float* weights = tab + tab_weights(int(n_mels));
    const CountingReader in{pcm, &max_read[0]}, ddr{d_db, &max_read[1]};
    std::vector<float> lds(kBLdsFloats);
    float* win = lds.data() + kBLdsWin; float* tw = lds.data() + kBLdsTw; float* stage = lds.data() + kBLdsStage;
    float* acc = lds.data() + kBLdsAcc; float* zr = lds.data() + kBLdsZr; float* zi = lds.data() + kBLdsZi;
    float* pw = lds.data() + kBLdsPw; float* dp = lds.data() + kBLdsDp;
    struct Regs { float g[2][2], xr[5], xi[5]; };
    std::vector<Regs> regs(kThreads);
    const int64_t n_wg = clips * r.runs;
    for (int64_t w = 0; w < n_wg; ++w) {
        const int64_t wg = order ? n_wg - 1 - w : w, clip = wg / r.runs;
        const int run = int(wg - clip * r.runs);
        const int f0 = run * r.per, nf = run_count(run, r.per, r.frames), span = span_of(nf, r.hop);
        if (span > kSpan) return -3;
        const int64_t dd = clip * n_mels * r.frames + f0;
        for (int i = 0; i < kFft + 2 * kTw; ++i) lds[i] = tab[i];
        for (int t = 0; t < kThreads; ++t) stage_row(t, in, clip * stride, r.n, f0 * r.hop, span, stage);
        for (int i = 0; i < span; ++i) acc[i] = 0.f;
        for (int f = 0; f < nf; ++f) {
            for (int t = 0; t < kThreads; ++t) {
                for (int parity = 0; parity < 2; ++parity)
                    for (int j = 0; j < 2; ++j) {
                        const int b = pass_band(t, j, parity);
                        regs[t].g[parity][j] = b < n_mels ? ddr(dd + int64_t(b) * r.frames + f) : 0.f;
                    }
                fft_first(t, stage + f * r.hop, win, zr, zi);
            }
            for (int st = 1; st <= 4; ++st)
                for (int t = 0; t < kThreads; ++t) fft_stage(t, st, tw, zr, zi);
            for (int t = 0; t < kThreads; ++t) spectrum(t, tw, zr, zi, regs[t].xr, regs[t].xi, pw, dp);
            for (int parity = 0; parity < 2; ++parity)
                for (int t = 0; t < kThreads; ++t) mel_pass(t, parity, pw, meta, weights, int(n_mels), amin, regs[t].g[parity], dp);
            for (int t = 0; t < kThreads; ++t) spectrum_grad(t, regs[t].xr, regs[t].xi, dp, pw);
            // ifft_first reads dp / pw at other threads' bins and writes zr / zi: separate buffers, one phase
            for (int t = 0; t < kThreads; ++t) ifft_first(t, tw, dp, pw, zr, zi);
            for (int st = 1; st <= 4; ++st)
                for (int t = 0; t < kThreads; ++t) fft_stage(t, st, tw, zr, zi);
            for (int t = 0; t < kThreads; ++t) overlap_add(t, win, zr, zi, acc + f * r.hop);
        }
        float* slot = ws + (clip * r.runs + run) * int64_t(r.span);
        for (int i = 0; i < span; ++i) slot[i] = acc[i];
    }
    if (fold_threads == 0) fold_threads = kFoldThreads;
    const CountingWriter out{d_pcm, writes};
    int64_t ws_read = -1;
    const CountingReader wsr{ws, &ws_read};
    const int64_t blocks = (n + fold_threads - 1) / fold_threads, n_fold = clips * blocks;
    for (int64_t w = 0; w < n_fold; ++w) {
        const int64_t wg = order ? n_fold - 1 - w : w, clip = wg / blocks;
        for (int t = 0; t < fold_threads; ++t) {
            const int64_t s = (wg - clip * blocks) * fold_threads + t;
            if (s < n) out(clip * d_stride + s, fold_sample(wsr, clip * int64_t(r.runs) * r.span, r, int(s)));
        }
    }
    if (ws_read >= clips * int64_t(r.runs) * r.span) return -4;
    return 0;
}
