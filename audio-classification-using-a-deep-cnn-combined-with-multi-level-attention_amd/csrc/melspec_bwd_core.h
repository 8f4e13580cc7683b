// melspec_bwd_core.h -- per-thread arithmetic and ALL index arithmetic of the mel-dB front-end's backward (the ResNet branch:
// gradients from the (clips, images, 1, bands, width) mel-dB images to the waveform), written so that the SAME source runs
// (a) inside melspec_bwd.hip on gfx950 and (b) on the host, thread by thread and phase by phase, in csrc/melspec_bwd_hostsim.cpp
// (built with g++ by the CPU tests), after the pattern of melspec_core.h / logmel_bwd_core.h. A "phase" is what one thread does
// between two barriers. Global memory is reached through callables (Reader / Writer here, counting ones in the host simulation).
//
// What is differentiated, per clip y[0 .. n-1] (melspec_core.h: x_f = w . p[f hop ..], X = rFFT2048(x_f), P = |X|^2, S = M P,
// D = 10 log10(max(amin, S)), out[t][0][b][x] = max(D[b, t stride + x], max(D) - top_db)), given G = dL / d out:
//
//   gD[b, f] = sum_t G[t][0][b][f - t stride]           over the images that hold column f, ascending t
//   dD[b, f] = gD[b, f] where D[b, f] > floor, else 0
//   dD[b*, f*] += sum_{D < floor} gD                    (b*, f*) = first cell in (band, column) order that holds max(D)
//   r_b   = dD[b, f] (10 / ln 10) / S_b where S_b > amin, else 0
//   dP_k  = sum_b M[b, k] r_b                            bands of one parity have disjoint bins: two passes, no atomics, no table
//   U_k   = 2 dP_k X_k
//   dx[m] = w[m] Re sum_{k=0}^{1024} U_k e^(+i theta k m),  theta = 2 pi / 2048   (one-sided: every bin once)
//   dp[f hop + m] += dx[m];   dy[s] = dp[1024 + s] + (1 <= s <= 1024: dp[1024 - s]) + (n - 1025 <= s <= n - 2: dp[1024 + 2 (n - 1) - s])
//
// The one-sided inverse runs through ONE 1024-point complex transform, the forward's real-FFT split backwards: with V = U / 2
//   C_k = (V_k + conj V_(1024-k)) + i e^(i theta k) (V_k - conj V_(1024-k)),  k = 1 .. 1023
//   C_0 = 2 (V_0 + V_1024) + 2 i (V_0 - V_1024)          (X_0 and X_1024 are real; a bin that enters once counts double here)
//   c[p] = sum_k C_k e^(+2 pi i k p / 1024) = dx[2 p] + i dx[2 p + 1],  and c = conj FFT1024(conj C):
// melspec_core.h's radix-4 stages serve both directions.
//
// Three kernels, none persistent (no grid cap):
//   images_bwd   one workgroup of 1024 threads per clip. Thread `tid` owns columns tid, tid + 1024, ... of every band. Phase 1
//                stores every dD whose D is not the clip's maximum and sums gD over its clipped cells in a fixed order;
//                a fixed tree adds the 1024 sums and finds the first maximum cell; phase 2 stores the cells that hold the
//                maximum, the first of them with the floor term. Every dD element is stored exactly once.
//   db_bwd       one workgroup of 256 threads per run of up to 32 consecutive frames of one clip (runs are cut per clip). It
//                stages the run's padded samples, recomputes each frame's spectrum, and overlap-adds the windowed inverse in
//                LDS in ascending frame order; the span of 2048 + (frames - 1) hop floats goes to the run's workspace slot.
//   fold         one thread per sample: the spans that cover a padded index are summed in run order, then the reflect fold in
//                the order of the formula above. Every d_pcm[c][s], s < n, is stored exactly once.
#ifndef MLA_MELSPEC_BWD_CORE_H
#define MLA_MELSPEC_BWD_CORE_H

#include <cstdint>

#include "melspec_core.h"

namespace melspec_bwd {

using namespace melspec;

constexpr int kBwdRunFrames = 32;                   // frames per db_bwd workgroup
constexpr int kSpan = 5120;                         // floats of one run's staged samples and of its overlap-added gradient
constexpr int kBuf = kHalf + 4;                     // a 1025-entry buffer, padded
constexpr int kImgThreads = 1024, kFoldThreads = 256;
constexpr int kBandStep = 4;                        // bands whose loads one thread of images_bwd has in flight together
constexpr float kTenOverLn10 = 4.342944819032518f;
constexpr int64_t kNoCell = INT64_MAX;

// LDS of a db_bwd workgroup (float indices): 77 888 bytes, two workgroups per CU
constexpr int kBLdsWin = 0, kBLdsTw = kBLdsWin + kFft, kBLdsStage = kBLdsTw + 2 * kTw, kBLdsAcc = kBLdsStage + kSpan,
              kBLdsZr = kBLdsAcc + kSpan, kBLdsZi = kBLdsZr + kBuf, kBLdsPw = kBLdsZi + kBuf, kBLdsDp = kBLdsPw + kBuf,
              kBLdsFloats = kBLdsDp + kBuf;

struct Reader {
    const float* p;
    MLA_MS_HD float operator()(int64_t i) const { return p[i]; }
};
struct Writer {
    float* p;
    MLA_MS_HD void operator()(int64_t i, float v) const { p[i] = v; }
};

// ---- run geometry (hop <= 2^30: the launcher clamps it, a hop beyond the clip gives one frame whatever it is) ---------------------
MLA_MS_HD int bwd_run_frames(int64_t hop) {
    const int64_t f = 1 + (kSpan - kFft) / hop;
    return f < kBwdRunFrames ? int(f) : kBwdRunFrames;
}
MLA_MS_HD int64_t bwd_frames(int64_t n, int64_t hop) { return 1 + n / hop; }
MLA_MS_HD int64_t bwd_runs(int64_t n, int64_t hop) {
    const int64_t per = bwd_run_frames(hop);
    return (bwd_frames(n, hop) + per - 1) / per;
}
// floats of a run's workspace slot, and of the part a run of nf frames fills
MLA_MS_HD int span_of(int nf, int hop) { return kFft + (nf - 1) * hop; }
MLA_MS_HD int bwd_span(int64_t hop) { return span_of(bwd_run_frames(hop), int(hop)); }
MLA_MS_HD int run_count(int run, int per, int frames) { return frames - run * per < per ? frames - run * per : per; }

// ---- images_bwd ------------------------------------------------------------------------------------------------------------
struct Images {
    int n_mels, frames, n_images, image_w, stride;
};

// the images t_lo .. t_hi that hold column f (empty: t_hi < t_lo)
MLA_MS_HD void image_range(const Images& s, int f, int* t_lo, int* t_hi) {
    if (s.stride == 0) {
        *t_lo = 0;
        *t_hi = f < s.image_w ? s.n_images - 1 : -1;
        return;
    }
    const int hi = f / s.stride, lo = f - s.image_w + 1;
    *t_hi = hi < s.n_images - 1 ? hi : s.n_images - 1;
    *t_lo = lo <= 0 ? 0 : (lo + s.stride - 1) / s.stride;
}

// D and gD of kBandStep consecutive bands b0 .. at column f (bands from n_mels on are not read): the loads of a step are independent
// of each other, so they are in flight together; a cell's gD is still summed over its images in ascending t
template <typename G, typename Dv>
MLA_MS_HD void load_cells(const G& g, int64_t g_clip, const Dv& D, int64_t d_clip, const Images& s, int b0, int f, int t_lo, int t_hi,
                          float* d, float* gd) {
    for (int u = 0; u < kBandStep; ++u) {
        d[u] = b0 + u < s.n_mels ? D(d_clip + int64_t(b0 + u) * s.frames + f) : 0.f;
        gd[u] = 0.f;
    }
    for (int t = t_lo; t <= t_hi; ++t)
        for (int u = 0; u < kBandStep; ++u)
            if (b0 + u < s.n_mels) gd[u] += g(g_clip + (int64_t(t) * s.n_mels + b0 + u) * s.image_w + (f - t * s.stride));
}

MLA_MS_HD float max_partial(int tid, const float* partial, int runs) {
    float m = -INFINITY;
    for (int i = tid; i < runs; i += kImgThreads) m = mla::nan_max(m, partial[i]);
    return m;
}
MLA_MS_HD void max_step(int tid, int s, float* red) {
    if (tid < s) red[tid] = mla::nan_max(red[tid], red[tid + s]);
}

// phase 1: every cell of the thread that does not hold the maximum m. Returns the sum of gD over the thread's clipped cells,
// columns ascending and bands ascending within a column, and leaves in *first the thread's lowest cell index (band * frames +
// column) that holds m (kNoCell: none).
template <typename G, typename Dv, typename Out>
MLA_MS_HD float images_phase1(int tid, const G& g, int64_t g_clip, const Dv& D, const Out& out, int64_t d_clip, const Images& s, float m,
                              float floor, int64_t* first) {
    float clipped = 0.f;
    *first = kNoCell;
    for (int f = tid; f < s.frames; f += kImgThreads) {
        int t_lo, t_hi;
        image_range(s, f, &t_lo, &t_hi);
        for (int b0 = 0; b0 < s.n_mels; b0 += kBandStep) {
            float d[kBandStep], gd[kBandStep];
            load_cells(g, g_clip, D, d_clip, s, b0, f, t_lo, t_hi, d, gd);
            for (int u = 0; u < kBandStep && b0 + u < s.n_mels; ++u) {
                const int64_t cell = int64_t(b0 + u) * s.frames + f;
                if (d[u] == m) {
                    if (cell < *first) *first = cell;
                    continue;
                }
                out(d_clip + cell, d[u] > floor ? gd[u] : 0.f);
                if (d[u] < floor) clipped += gd[u];
            }
        }
    }
    return clipped;
}
MLA_MS_HD void sum_step(int tid, int s, float* sum, int64_t* first) {
    if (tid < s) {
        sum[tid] += sum[tid + s];
        if (first[tid + s] < first[tid]) first[tid] = first[tid + s];
    }
}
// phase 2: the cells that hold the maximum; `term` (the clip's clipped sum, or 0 without the floor's gradient) goes to `first`
template <typename G, typename Dv, typename Out>
MLA_MS_HD void images_phase2(int tid, const G& g, int64_t g_clip, const Dv& D, const Out& out, int64_t d_clip, const Images& s, float m,
                             float floor, float term, int64_t first) {
    for (int f = tid; f < s.frames; f += kImgThreads) {
        int t_lo, t_hi;
        image_range(s, f, &t_lo, &t_hi);
        for (int b0 = 0; b0 < s.n_mels; b0 += kBandStep) {
            float d[kBandStep];
            for (int u = 0; u < kBandStep; ++u) d[u] = b0 + u < s.n_mels ? D(d_clip + int64_t(b0 + u) * s.frames + f) : 0.f;
            for (int u = 0; u < kBandStep && b0 + u < s.n_mels; ++u) {
                if (!(d[u] == m)) continue;
                const int64_t cell = int64_t(b0 + u) * s.frames + f;
                float gd = 0.f;
                for (int t = t_lo; t <= t_hi; ++t) gd += g(g_clip + (int64_t(t) * s.n_mels + b0 + u) * s.image_w + (f - t * s.stride));
                float v = d[u] > floor ? gd : 0.f;
                if (cell == first) v += term;
                out(d_clip + cell, v);
            }
        }
    }
}

// ---- db_bwd ----------------------------------------------------------------------------------------------------------------
template <typename In>
MLA_MS_HD void stage_row(int t, const In& pcm, int64_t row, int n, int p0, int count, float* stage) {
    for (int i = t; i < count; i += kThreads) stage[i] = pcm(row + reflect(p0 + i, n));
}

// the band a thread owns in the pass of one parity: j = 0, 1 (bands beyond n_mels do not exist)
MLA_MS_HD int pass_band(int t, int j, int parity) { return 2 * (t + kThreads * j) + parity; }

// X_k as melspec::power_bin forms it
MLA_MS_HD void spectrum_bin(int k, const float* tw, const float* zr, const float* zi, float* xr, float* xi) {
    const int a = k & (kHalf - 1), b = (kHalf - k) & (kHalf - 1);
    const float er = 0.5f * (zr[a] + zr[b]), ei = 0.5f * (zi[a] - zi[b]);
    const float orr = 0.5f * (zi[a] + zi[b]), oi = -0.5f * (zr[a] - zr[b]);
    const float wr = tw[2 * k], wi = tw[2 * k + 1];
    *xr = er + (wr * orr - wi * oi);
    *xi = ei + (wr * oi + wi * orr);
}
// thread t keeps X_k of its bins k = t + 256 j (j < 4; j = 4 is bin 1024, thread 0 only), writes P_k to pw and clears dp
MLA_MS_HD void spectrum(int t, const float* tw, const float* zr, const float* zi, float* xr, float* xi, float* pw, float* dp) {
    for (int j = 0; j < 4; ++j) {
        const int k = t + kThreads * j;
        spectrum_bin(k, tw, zr, zi, &xr[j], &xi[j]);
        pw[k] = xr[j] * xr[j] + xi[j] * xi[j];
        dp[k] = 0.f;
    }
    xr[4] = xi[4] = 0.f;
    if (t == 0) {
        spectrum_bin(kHalf, tw, zr, zi, &xr[4], &xi[4]);
        pw[kHalf] = xr[4] * xr[4] + xi[4] * xi[4];
        dp[kHalf] = 0.f;
    }
}
// the bands of one parity: S_b as melspec::mel_db sums it, r_b, and dp[k] += M[b, k] r_b over the band's bins. g[j] = dD of band
// pass_band(t, j, parity) in this frame.
MLA_MS_HD void mel_pass(int t, int parity, const float* pw, const int* meta, const float* weights, int n_mels, float amin, const float* g,
                        float* dp) {
    for (int j = 0; j < 2; ++j) {
        const int b = pass_band(t, j, parity);
        if (b >= n_mels) return;
        const int first = meta[3 * b], bins = meta[3 * b + 1];
        const float* w = weights + meta[3 * b + 2];
        float acc = 0.f;
        for (int i = 0; i < bins; ++i) acc = fmaf(w[i], pw[first + i], acc);
        const float r = acc > amin ? g[j] * kTenOverLn10 / acc : 0.f;
        for (int i = 0; i < bins; ++i) dp[first + i] += w[i] * r;
    }
}
// V_k = dP_k X_k for the thread's bins: the real part over dp[k] in place, the imaginary part to vi[k]
MLA_MS_HD void spectrum_grad(int t, const float* xr, const float* xi, float* dp, float* vi) {
    for (int j = 0; j < 4; ++j) {
        const int k = t + kThreads * j;
        const float d = dp[k];
        dp[k] = d * xr[j];
        vi[k] = d * xi[j];
    }
    if (t == 0) {
        const float d = dp[kHalf];
        dp[kHalf] = d * xr[4];
        vi[kHalf] = d * xi[4];
    }
}
// conj C_m, m < 1024
MLA_MS_HD void join_bin(int m, const float* tw, const float* vr, const float* vi, float* cr, float* ci) {
    if (m == 0) {
        *cr = 2.f * (vr[0] + vr[kHalf]);
        *ci = -2.f * (vr[0] - vr[kHalf]);
        return;
    }
    const float ar = vr[m], ai = vi[m], br = vr[kHalf - m], bi = vi[kHalf - m];
    const float sr = ar + br, si = ai - bi;             // V_m + conj V_(1024-m)
    const float dr = ar - br, di = ai + bi;             // V_m - conj V_(1024-m)
    // e^(i theta m) = (twr, -twi);  e d = (twr dr + twi di, twr di - twi dr);  i e d = (-(twr di - twi dr), twr dr + twi di)
    const float twr = tw[2 * m], twi = tw[2 * m + 1];
    *cr = sr - (twr * di - twi * dr);
    *ci = -(si + (twr * dr + twi * di));
}
// melspec::fft_first on conj C instead of the windowed samples
MLA_MS_HD void ifft_first(int t, const float* tw, const float* vr, const float* vi, float* zr, float* zi) {
    const int r = rev4(t);
    float ar[4], ai[4], yr[4], yi[4];
    for (int q = 0; q < 4; ++q) join_bin(256 * q + r, tw, vr, vi, &ar[q], &ai[q]);
    radix4(ar, ai, yr, yi);
    for (int q = 0; q < 4; ++q) { zr[4 * t + q] = yr[q]; zi[4 * t + q] = yi[q]; }
}
// then melspec::fft_stage 1 .. 4: conj c[p] is in (zr, zi)[p]; dx[2 p] = zr[p], dx[2 p + 1] = -zi[p], windowed and added at the frame
MLA_MS_HD void overlap_add(int t, const float* win, const float* zr, const float* zi, float* acc) {
    for (int j = 0; j < 4; ++j) {
        const int p = t + kThreads * j;
        acc[2 * p] += win[2 * p] * zr[p];
        acc[2 * p + 1] += win[2 * p + 1] * -zi[p];
    }
}

// ---- fold ------------------------------------------------------------------------------------------------------------------
struct Runs {
    int n, hop, frames, per, runs, span;
};
MLA_MS_HD Runs runs_for(int64_t n, int64_t hop) {
    return Runs{int(n), int(hop), int(bwd_frames(n, hop)), bwd_run_frames(hop), int(bwd_runs(n, hop)), bwd_span(hop)};
}
// the gradient at padded index q: the spans that cover it, runs ascending; 0 where no frame reaches
template <typename W>
MLA_MS_HD float padded_grad(const W& ws, int64_t ws_clip, const Runs& g, int q) {
    const int step = g.per * g.hop;
    int r_hi = q / step;
    if (r_hi > g.runs - 1) r_hi = g.runs - 1;
    const int r_lo = q - g.span + 1 <= 0 ? 0 : int((int64_t(q) - g.span + step) / step);
    float acc = 0.f;
    for (int r = r_lo; r <= r_hi; ++r) {
        const int off = q - r * step;
        if (off < span_of(run_count(r, g.per, g.frames), g.hop)) acc += ws(ws_clip + int64_t(r) * g.span + off);
    }
    return acc;
}
template <typename W>
MLA_MS_HD float fold_sample(const W& ws, int64_t ws_clip, const Runs& g, int s) {
    float v = padded_grad(ws, ws_clip, g, kPad + s);
    if (s >= 1 && s <= kPad) v += padded_grad(ws, ws_clip, g, kPad - s);
    if (s >= g.n - 1 - kPad && s <= g.n - 2) v += padded_grad(ws, ws_clip, g, kPad + 2 * (g.n - 1) - s);
    return v;
}

}  // namespace melspec_bwd
#endif
