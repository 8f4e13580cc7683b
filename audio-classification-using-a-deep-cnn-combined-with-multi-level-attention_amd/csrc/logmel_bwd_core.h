// logmel_bwd_core.h -- per-lane arithmetic and ALL index arithmetic of the log-mel front-end's backward kernel, written so that
// the SAME source runs (a) inside logmel_bwd.hip on gfx950 and (b) on the host, lane by lane, in csrc/logmel_bwd_hostsim.cpp
// (built with g++ by the CPU tests), after the pattern of logmel_core.h / conv1_dgrad_core.h.
//
// What is differentiated (mel_features.py:71-92 stft_magnitude, :220-223 mel + log, framed as vggish_input.py:56-76), for one
// STFT frame f of a waveform row, y[m] = w[m] x[160 f + m] zero-padded to 512, t = 2 pi / 512:
//
//   X_k = sum_m y[m] e^(-i t k m), k = 0 .. 256     A_k = |X_k|     mel_b = sum_k M[k, b] A_k     out[f, b] = log(mel_b + 0.01)
//
// and, given G[f, b] = dL / d out[f, b]:
//
//   r_b   = G[f, b] / (mel_b + 0.01)
//   dA_k  = sum_b M[k, b] r_b                    (M is non-zero for bins 5 .. 239, <= 2 adjacent bands per bin)
//   U_k   = dA_k X_k / A_k, 0 where A_k = 0      (torch's sgn(0) = 0 convention)
//   dy[m] = Re sum_k U_k e^(+i t k m)            (one-sided: every bin enters once, no factor 2)
//   dx[160 f + m] += w[m] dy[m]
//
// The one-sided inverse runs through ONE 256-point complex transform, the forward's real-FFT split backwards: with U_0 = U_256 = 0
//   C_k = 1/2 [ (U_k + conj U_(256-k)) + i e^(i t k) (U_k - conj U_(256-k)) ],  k = 0 .. 255     (C_0 = 0)
//   c[p] = sum_k C_k e^(+2 pi i k p / 256) = dy[2 p] + i dy[2 p + 1]
// and c = conj FFT256(conj C), so the forward's radix-16 x radix-16 transform (logmel_core.h) serves both directions.
//
// A 16-lane group owns one frame; lane j owns bins j + 16 s (s = 0 .. 15) in the bin domain -- which is both what the forward's
// second radix-16 leaves in the lane (Z[j + 16 k2]) and what the inverse's first radix-16 takes from it (C[16 n1 + j]) -- and the
// sample pairs 2 j + 32 n (+1) in the sample domain. The stages below are separated by group-wide hand-offs through two buffers
// (LDS in the kernel, plain arrays on the host):
//   bufA (576 floats)  exchange rows -> Z (natural order) -> U / 2 (natural order) -> exchange rows -> w[m] dy[m], m < 400
//   bufB (320 floats)  |2 X_k| for k < 256, then r_b at 256 + b
//
// Work item = (row, 14 consecutive hop-chunks of 160 samples c0 .. c0 + 13), computed from the 16 frames c0 - 2 .. c0 + 13 by the
// 16 groups of a 256-lane workgroup; the gather then sums, per sample, its <= 3 frames in ascending frame order and stores once.
// Frames outside [0, 96 N) contribute nothing and read nothing. Nothing about a row depends on the other rows, a stride or the grid.
#ifndef MLA_LOGMEL_BWD_CORE_H
#define MLA_LOGMEL_BWD_CORE_H

#include <cstdint>

#include "logmel_core.h"

namespace logmel_bwd {

using namespace logmel;

constexpr int kItemChunks = 14;                     // hop-chunks (160 samples) stored by one work item
constexpr int kItemFrames = 16;                     // frames c0 - 2 .. c0 + 13 that reach them: one per 16-lane group
constexpr int kThreads = 16 * kItemFrames;          // 256
constexpr int kMaxWg = 512;                         // grid cap: the 2 workgroups per CU that fit (LDS) on a 256-CU part; beyond it workgroups loop
constexpr int kBufA = 2 * 16 * kXchStride;          // 576
constexpr int kBufB = 256 + kBands;                 // 320
constexpr int kGroupFloats = kBufA + kBufB + 32;     // 928 = 32 mod 64: the two groups of a 32-lane half read opposite halves of a bank row
constexpr float kTiny = 1.17549435e-38f;            // |2X|^2 below the smallest normal float counts as A_k = 0

// backward table layout (float indices) ---------------------------------------------
constexpr int kTabT = 0;                            // 256 bins x (int32 b0, M[k][b0] / 2, M[k][b0 + 1] / 2, 0): the transposed mel step
constexpr int kTabW = 1024;                         // 256 x (cos, -sin)(2 pi k / 512), k = 0 .. 255
constexpr int kBwdTabFloats = 1536;

// ---- index arithmetic ---------------------------------------------------------------------------------------------------------
MLA_HD int64_t chunks_of(int64_t n_samples) { return (n_samples + kHop - 1) / kHop; }
MLA_HD int64_t items_per_row(int64_t n_samples) { return (chunks_of(n_samples) + kItemChunks - 1) / kItemChunks; }
MLA_HD int64_t used_frames(int64_t n_samples) {      // 96 N: the frames that make whole examples (mla_logmel_counts)
    if (n_samples < kWin) return 0;
    return ((1 + (n_samples - kWin) / kHop) / kExFrames) * kExFrames;
}
MLA_HD int grid_of(int64_t n_items) { return int(n_items < kMaxWg ? n_items : kMaxWg); }
MLA_HD void item_locate(int64_t item, int64_t ipr, int64_t* row, int64_t* c0) {
    *row = item / ipr;
    *c0 = (item - *row * ipr) * kItemChunks;
}
MLA_HD int64_t group_frame(int64_t c0, int g) { return c0 - 2 + g; }
MLA_HD bool frame_live(int64_t f, int64_t used) { return f >= 0 && f < used; }
// sample m of frame f in a row; pair n (0 .. 12), element e of lane j is m = 32 n + 2 j + e
MLA_HD int lane_sample(int j, int n, int e) { return 32 * n + 2 * j + e; }
MLA_HD int64_t pcm_index(int64_t row, int64_t stride, int64_t f, int m) { return row * stride + f * kHop + m; }
// G is (W * N, 96, 64): row-major examples, so a row's frame f is row * used + f
MLA_HD int64_t g_index(int64_t row, int64_t used, int64_t f, int band) { return (row * used + f) * kBands + band; }
// the gather: local output i (0 .. 14 * 160) of an item -> its chunk and offset; term d (0, 1, 2) comes from group cl + d (frame
// c0 + cl - 2 + d, ascending) at window position o + 160 (2 - d), which exists below 400 only
MLA_HD void out_locate(int i, int* cl, int* o) { *cl = i / kHop; *o = i - *cl * kHop; }
MLA_HD int term_pos(int o, int d) { return o + kHop * (2 - d); }

// ---- the backward table, read where it is used (LDS-resident in the kernel) ----------
MLA_HD int bin_band0(const float* btab, int k) { return reinterpret_cast<const int*>(btab + kTabT)[4 * k]; }   // b0 + 1 <= 63
MLA_HD float bin_w0(const float* btab, int k) { return btab[kTabT + 4 * k + 1]; }                              // M[k][b0] / 2
MLA_HD float bin_w1(const float* btab, int k) { return btab[kTabT + 4 * k + 2]; }                              // M[k][b0 + 1] / 2
MLA_HD float bin_twr(const float* btab, int k) { return btab[kTabW + 2 * k]; }                                 // (cos, -sin)(2 pi k / 512)
MLA_HD float bin_twi(const float* btab, int k) { return btab[kTabW + 2 * k + 1]; }

// 1 / sqrt(v) for a normal v > 0 and 1 / v for v >= 0.01: one v_rsq_f32 / v_rcp_f32 (1 ulp) on the device
MLA_HD float inv_sqrt(float v) {
#if defined(__HIP_DEVICE_COMPILE__)
    return __builtin_amdgcn_rsqf(v);
#else
    return 1.0f / __builtin_sqrtf(v);
#endif
}
MLA_HD float inv(float v) {
#if defined(__HIP_DEVICE_COMPILE__)
    return __builtin_amdgcn_rcpf(v);
#else
    return 1.0f / v;
#endif
}

// ---- stage 1: window. x[2 n + e] = the lane's sample lane_sample(j, n, e) as a float (0 beyond 399), win = Hann(400) then zeros
MLA_HD void window_lane(int j, const float* x, const float* win, float* re, float* im) {
    _Pragma("unroll") for (int n = 0; n < kN1; ++n) {
        re[n] = x[2 * n] * win[lane_sample(j, n, 0)];
        im[n] = x[2 * n + 1] * win[lane_sample(j, n, 1)];
    }
}
// then logmel::phase1_fft(c, j, re, im, bufA) | hand-off | logmel::phase2_read(j, bufA, re, im) | hand-off | logmel::phase2_fft

// ---- stage 3: Z[j + 16 k2] (element dr16(k2) of the lane) to bufA in natural order
MLA_HD void store_z(int j, const float* re, const float* im, float* z) {
    _Pragma("unroll") for (int k2 = 0; k2 < 16; ++k2) {
        z[2 * (j + 16 * k2)] = re[dr16(k2)];
        z[2 * (j + 16 * k2) + 1] = im[dr16(k2)];
    }
}

// ---- stage 4: the lane's 16 bins: 2 X_k from Z_k and Z_(256-k), |2 X_k| to mag[k], the unit phasor X_k / A_k (0 where A_k = 0)
// to pr / pi. Bin 0 carries no mel weight: phasor and magnitude 0 (Z[256] does not exist).
MLA_HD void split_lane(int j, const float* btab, const float* z, float* mag, float* pr, float* pi) {
    _Pragma("unroll") for (int s = 0; s < 16; ++s) {
        const int k = j + 16 * s;
        if (k == 0) { mag[0] = 0.f; pr[s] = 0.f; pi[s] = 0.f; continue; }
        const float a = z[2 * k], b = z[2 * k + 1], p = z[2 * (256 - k)], q = z[2 * (256 - k) + 1];
        const float er = a + p, ei = b - q;                 // 2 E[k] = Z[k] + conj Z[256-k]
        float orr = b + q, oi = p - a;                      // 2 O[k] = (Z[k] - conj Z[256-k]) / i
        cmul(orr, oi, bin_twr(btab, k), bin_twi(btab, k));
        const float ur = er + orr, ui = ei + oi;
        const float ss = ur * ur + ui * ui;
        const bool live = ss >= kTiny;
        const float rs = live ? inv_sqrt(ss) : 0.f;
        mag[k] = ss * rs;
        pr[s] = ur * rs;
        pi[s] = ui * rs;
    }
}

// ---- stage 5: lane j's four bands (logmel::band_of), mel_b as the forward sums it (weights M / 2 over |2 X|, 4-bin aligned
// windows), then r_b = g[slot] / (mel_b + 0.01) to r[b]
MLA_HD void ratio_lane(const LaneConsts& c, int j, const float* mag, const float* melw, const float* g, float* r) {
    constexpr int first[4] = {0, kSlot0, kSlot0 + kSlot1, kSlot0 + kSlot1 + kSlot2};
    constexpr int count[4] = {kSlot0, kSlot1, kSlot2, kSlot3};
    _Pragma("unroll") for (int s = 0; s < 4; ++s) {
        float acc = 0.f;
        _Pragma("unroll") for (int t = 0; t < count[s]; ++t) acc += melw[first[s] + t] * mag[c.mel_start[s] + t];
        r[band_of(j, s)] = g[s] * inv(acc + 0.01f);
    }
}

// ---- stage 6: U_k / 2 = (dA_k / 2) X_k / A_k for the lane's bins, kept in ur / ui and written to bufA in natural order
MLA_HD void spectrum_grad_lane(int j, const float* btab, const float* r, const float* pr, const float* pi, float* ur, float* ui, float* u) {
    _Pragma("unroll") for (int s = 0; s < 16; ++s) {
        const int k = j + 16 * s;
        const int b0 = bin_band0(btab, k);
        const float da = bin_w0(btab, k) * r[b0] + bin_w1(btab, k) * r[b0 + 1];
        ur[s] = da * pr[s];
        ui[s] = da * pi[s];
        u[2 * k] = ur[s];
        u[2 * k + 1] = ui[s];
    }
}

// ---- stage 7: conj C_k for the lane's bins into re / im[s]: the input of the inverse's first radix-16
MLA_HD void join_lane(int j, const float* btab, const float* ur, const float* ui, const float* u, float* re, float* im) {
    _Pragma("unroll") for (int s = 0; s < 16; ++s) {
        const int k = j + 16 * s;
        if (k == 0) { re[s] = 0.f; im[s] = 0.f; continue; }
        const float vr = u[2 * (256 - k)], vi = u[2 * (256 - k) + 1];
        const float sr = ur[s] + vr, si = ui[s] - vi;       // U_k + conj U_(256-k)   (halves)
        const float dr = ur[s] - vr, di = ui[s] + vi;       // U_k - conj U_(256-k)
        // e^(i t k) = (twr, -twi);  e d = (twr dr + twi di, twr di - twi dr);  i e d = (-(twr di - twi dr), twr dr + twi di)
        const float twr = bin_twr(btab, k), twi = bin_twi(btab, k);
        const float cr = sr - (twr * di - twi * dr);
        const float ci = si + (twr * dr + twi * di);
        re[s] = cr;
        im[s] = -ci;
    }
}

// ---- stage 8: the inverse's first radix-16 on 16 full inputs, then as logmel::phase1_fft
MLA_HD void phase1_fft_full(const LaneConsts& c, int j, float* re, float* im, float* xch) {
    dft16<false>(re, im);
    _Pragma("unroll") for (int k1 = 0; k1 < 16; ++k1) {
        float r = re[dr16(k1)], i = im[dr16(k1)];
        if (k1) cmul(r, i, c.tw_re[k1], c.tw_im[k1]);
        xch[2 * (k1 * kXchStride + j)] = r;
        xch[2 * (k1 * kXchStride + j) + 1] = i;
    }
}
// | hand-off | logmel::phase2_read | hand-off | logmel::phase2_fft

// ---- stage 10: conj c[j + 16 k2] sits in element dr16(k2): dy[2 p] = re, dy[2 p + 1] = -im; windowed, to dyw[m] for m < 400
MLA_HD void window_out_lane(int j, const float* re, const float* im, const float* win, float* dyw) {
    _Pragma("unroll") for (int k2 = 0; k2 < kN1; ++k2) {
        const int m = lane_sample(j, k2, 0);
        if (m < kWin) {
            dyw[m] = win[m] * re[dr16(k2)];
            dyw[m + 1] = win[m + 1] * -im[dr16(k2)];
        }
    }
}

}  // namespace logmel_bwd

// ---- host only: the backward table, in double precision from the forward's mel matrix ------------------------------------------
#include <cmath>
#include <cstring>
#include <vector>

#include "logmel_tables.h"

namespace logmel_bwd {

// returns 0, or negative if a bin feeds more than two bands or two bands that are not adjacent
inline int build_bwd_tables(float* tab) {
    const double pi = 3.14159265358979323846;
    std::memset(tab, 0, sizeof(float) * kBwdTabFloats);
    std::vector<double> mel(257 * kBands);
    mel_dense(mel.data());
    int* bi = reinterpret_cast<int*>(tab + kTabT);
    for (int b = 0; b < kBands; ++b)
        if (mel[256 * kBands + b] != 0.0) return -3;                // bin 256 must carry no weight: the inverse drops it
    for (int k = 0; k < 256; ++k) {
        int lo = -1, hi = -1, n = 0;
        for (int b = 0; b < kBands; ++b)
            if (mel[k * kBands + b] != 0.0) { if (lo < 0) lo = b; hi = b; ++n; }
        if (n > 2) return -1;
        if (n == 2 && hi != lo + 1) return -2;
        int b0 = n == 0 ? 0 : lo;
        if (b0 > kBands - 2) b0 = kBands - 2;
        bi[4 * k] = b0;
        tab[kTabT + 4 * k + 1] = (float)(0.5 * mel[k * kBands + b0]);
        tab[kTabT + 4 * k + 2] = (float)(0.5 * mel[k * kBands + b0 + 1]);
        tab[kTabW + 2 * k] = (float)std::cos(2.0 * pi * k / 512.0);
        tab[kTabW + 2 * k + 1] = (float)(-std::sin(2.0 * pi * k / 512.0));
    }
    return 0;
}

}  // namespace logmel_bwd

#endif
