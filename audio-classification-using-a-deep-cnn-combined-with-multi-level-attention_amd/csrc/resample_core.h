// resample_core.h -- the ONE arithmetic of the resampling front-end: the mono mix of mla_mono_mix, the band-limited sinc
// interpolation of mla_resample (resampy/interpn.py, filter 'kaiser_best') and the whole workgroup body of the batched
// "recordings -> clips" kernel (csrc/clips.hip). The SAME source runs (a) in clips.hip and stft_generic.hip on gfx950 and
// (b) on the host, workgroup by workgroup, in csrc/clips_hostsim.cpp (built with g++ by the CPU tests) with a plain array
// standing in for LDS: a row of mla_clips_prepare equals mla_mono_mix + mla_resample bit for bit because both call this file.
//
// Output sample t of a clip resampled by ratio = sr_out / sr_in sits at input time t / ratio:
//   position   n = int(t * (1 / ratio)), the fractional part scaled to table entries gives (offset, eta) of each wing
//   wings      left  wing: sum_i (win[off_l + i * step] + eta_l * delta[..]) * mono[n - i],      i < min(n + 1, (nwin - off_l) / step)
//              right wing: sum_k (win[off_r + k * step] + eta_r * delta[..]) * mono[n + k + 1],  k < min(n_in - n - 1, (nwin - off_r) / step)
//              one double accumulator, left wing first, one rounding to float32 by the caller. The filter table comes through
//              a reader: PairTable, (win, delta) pairs tab[2 * idx] and tab[2 * idx + 1], one 16-byte gather per tap (the clips
//              kernel), or SplitTable, separate win[idx] and delta[idx] arrays (mla_resample's arguments).
//   mono mix   the source is BYTES with a sample format code (8/16/24/32-bit PCM, float32, float64; include/mla_hip.h's
//              MLA_*): the samples of a frame are summed in double (exactly, for the integers), the mean is scaled by the format's
//              power of two and rounded once. No byte outside [clip, clip + frames * channels * bytes_per_sample) is read:
//              24-bit samples are assembled from their three bytes, the 2/4/8-byte formats use naturally aligned loads (the
//              clip starts on a multiple of its sample size).
//   workgroup  Clip (one recording's record), plan_tile (what the 256 outputs from t0 on need: copy, zero or filter, and the
//              span of input frames to stage), stage_span_raw (one lane's share of the staging) and tile_output (the value of
//              out[t]). The kernel runs plan, stage, barrier, store; the host simulation plan, all lanes stage, all outputs.
//
// Contraction is switched off in this file and the three fused expressions are spelled fma(), so that the bits do not depend
// on what a compiler decides for a translation unit; the host build (g++ -ffp-contract=off, correctly rounded fma from libm)
// then computes the same values as the device.
#ifndef MLA_RESAMPLE_CORE_H
#define MLA_RESAMPLE_CORE_H

#include <cmath>
#include <cstdint>

#if defined(__HIPCC__)
#define MLA_RS_HD __host__ __device__ __forceinline__
#else
#define MLA_RS_HD inline
#endif
#if defined(__clang__)
#define MLA_RS_NO_CONTRACT _Pragma("clang fp contract(off)")
#else
#define MLA_RS_NO_CONTRACT
#endif

namespace resample_core {

constexpr int kThreads = 256;              // outputs per workgroup
constexpr int kMaxRateFactor = 16;         // input rates up to 16 * sr_out are staged; faster ones are refused

MLA_RS_HD double scale_of(double ratio) { return ratio < 1.0 ? ratio : 1.0; }
MLA_RS_HD int index_step_of(double ratio, int num_table) { return int(scale_of(ratio) * num_table); }
// most taps a wing can have: (nwin - offset) / index_step with offset >= 0
MLA_RS_HD int wing_taps(int nwin, int index_step) { return nwin / index_step; }
MLA_RS_HD int64_t resampled_length(int64_t n_in, double ratio) { return int64_t(double(n_in) * ratio); }

struct Setup {
    int64_t n;                 // input sample at or left of the output's position
    int off_l, off_r;          // first table entry of each wing
    double eta_l, eta_r;       // its distance to the next entry, in entries
};

// input sample left of output t: monotone in t, so a workgroup's first and last outputs bound its span
MLA_RS_HD int64_t position(int64_t t, double ratio) {
    MLA_RS_NO_CONTRACT
    return int64_t(double(t) * (1.0 / ratio));
}

MLA_RS_HD Setup setup(int64_t t, double ratio, int num_table) {
    MLA_RS_NO_CONTRACT
    Setup s;
    const double scale = scale_of(ratio), inv = 1.0 / ratio, nt = double(num_table);
    s.n = int64_t(double(t) * inv);
    const double frac_l = scale * fma(inv, double(t), -double(s.n));
    const double if_l = frac_l * nt;
    s.off_l = int(if_l);
    s.eta_l = if_l - double(s.off_l);
    const double frac_r = scale - frac_l;
    const double if_r = frac_r * nt;
    s.off_r = int(if_r);
    s.eta_r = if_r - double(s.off_r);
    return s;
}

// the two layouts of a filter table: entry idx of the window and of its first difference
struct PairTable {
    const double* tab;
    MLA_RS_HD double win(int idx) const { return tab[2 * idx]; }
    MLA_RS_HD double delta(int idx) const { return tab[2 * idx + 1]; }
};
struct SplitTable {
    const double* w;
    const double* d;
    MLA_RS_HD double win(int idx) const { return w[idx]; }
    MLA_RS_HD double delta(int idx) const { return d[idx]; }
};

// x[j - x0] is mono[j] for every j the wings touch: [max(0, n - taps + 1), min(n_in - 1, n + taps)]
template <typename Table>
MLA_RS_HD double wings(const Setup& s, const float* x, int64_t x0, int64_t n_in, const Table& tab, int nwin, int index_step) {
    MLA_RS_NO_CONTRACT
    double acc = 0.0;
    const float* xc = x + (s.n - x0);
    int64_t i_max = (nwin - s.off_l) / index_step;
    if (s.n + 1 < i_max) i_max = s.n + 1;
    for (int i = 0; i < int(i_max); ++i) {
        const int idx = s.off_l + i * index_step;
        acc = fma(fma(s.eta_l, tab.delta(idx), tab.win(idx)), double(xc[-i]), acc);
    }
    int64_t k_max = (nwin - s.off_r) / index_step;
    if (n_in - s.n - 1 < k_max) k_max = n_in - s.n - 1;
    for (int k = 0; k < int(k_max); ++k) {
        const int idx = s.off_r + k * index_step;
        acc = fma(fma(s.eta_r, tab.delta(idx), tab.win(idx)), double(xc[k + 1]), acc);
    }
    return acc;
}

// Input frames [*first, *first + count) that outputs t_first..t_last of a clip need, clamped to the clip.
MLA_RS_HD void span(int64_t t_first, int64_t t_last, double ratio, int taps, int64_t n_in, int64_t* first, int* count) {
    const int64_t lo = position(t_first, ratio) - taps + 1, hi = position(t_last, ratio) + taps;
    const int64_t a = lo < 0 ? 0 : lo, b = hi > n_in - 1 ? n_in - 1 : hi;
    *first = a;
    *count = b >= a ? int(b - a + 1) : 0;
}

// Upper bound of span()'s count for any 256 consecutive outputs: the positions of the first and the last are at most
// 255 / ratio + 1 apart (+ 2 for the roundings of 1 / ratio and of the product).
MLA_RS_HD int64_t span_capacity(double ratio, int taps) { return int64_t(double(kThreads - 1) / ratio) + 3 + 2 * int64_t(taps); }

// ---- the source: interleaved samples as they sit in memory or in a file's data chunk (little endian) ----
enum : int { kF32 = 0, kI16 = 2, kF64 = 4, kI32 = 5, kU8 = 6, kI24 = 7 };        // MLA_F32, MLA_I16, MLA_F64, MLA_I32, MLA_U8, MLA_I24

// bytes per sample of a format code, 0 for a code that is no sample format
MLA_RS_HD int sample_bytes(int fmt) {
    switch (fmt) {
        case kU8: return 1;
        case kI16: return 2;
        case kI24: return 3;
        case kI32: case kF32: return 4;
        case kF64: return 8;
        default: return 0;
    }
}

// what a clip's first byte has to be a multiple of: the sample size of the formats read with aligned loads, 1 for bytes
MLA_RS_HD int sample_align(int fmt) { return fmt == kI24 ? 1 : sample_bytes(fmt); }

// what the mean of a frame's load_sample_as() values is multiplied by: full scale of the integer formats -> 1.0
MLA_RS_HD double sample_scale(int fmt) {
    switch (fmt) {
        case kU8: return 1.0 / 128.0;
        case kI16: return 1.0 / 32768.0;
        case kI24: return 1.0 / 8388608.0;
        case kI32: return 1.0 / 2147483648.0;
        default: return 1.0;
    }
}

// sample `elem` of a clip that starts at `clip` (a multiple of the sample size for the 2/4/8-byte formats): bytes
// [elem * sample_bytes, (elem + 1) * sample_bytes) of the clip and no others
template <int FMT>
MLA_RS_HD double load_sample_as(const unsigned char* clip, int64_t elem) {
    if constexpr (FMT == kU8) return double(int(clip[elem]) - 128);
    if constexpr (FMT == kI16) return double(reinterpret_cast<const int16_t*>(clip)[elem]);
    if constexpr (FMT == kI24) {
        const unsigned char* b = clip + 3 * elem;
        const uint32_t v = uint32_t(b[0]) | uint32_t(b[1]) << 8 | uint32_t(b[2]) << 16;
        return double(int32_t(v << 8) >> 8);                                      // sign extension of bit 23
    }
    if constexpr (FMT == kI32) return double(reinterpret_cast<const int32_t*>(clip)[elem]);
    if constexpr (FMT == kF32) return double(reinterpret_cast<const float*>(clip)[elem]);
    return double(float(reinterpret_cast<const double*>(clip)[elem]));            // kF64: rounded to float32 per sample, as a float read
}

// frame `frame` of a clip -> mono float32: mean over the channels in double, times the format's scale, rounded once
template <int FMT>
MLA_RS_HD float mono_mix_as(const unsigned char* clip, int64_t frame, int channels) {
    MLA_RS_NO_CONTRACT
    double acc = 0.0;
    for (int c = 0; c < channels; ++c) acc += load_sample_as<FMT>(clip, frame * channels + c);
    return float(acc / double(channels) * sample_scale(FMT));
}

MLA_RS_HD float mono_mix_raw(const unsigned char* clip, int64_t frame, int channels, int fmt) {
    switch (fmt) {
        case kU8: return mono_mix_as<kU8>(clip, frame, channels);
        case kI16: return mono_mix_as<kI16>(clip, frame, channels);
        case kI24: return mono_mix_as<kI24>(clip, frame, channels);
        case kI32: return mono_mix_as<kI32>(clip, frame, channels);
        case kF32: return mono_mix_as<kF32>(clip, frame, channels);
        default: return mono_mix_as<kF64>(clip, frame, channels);
    }
}

template <int FMT>
MLA_RS_HD void stage_span_as(int lane, const unsigned char* clip, int channels, int64_t first, int count, float* stage) {
    for (int i = lane; i < count; i += kThreads) stage[i] = mono_mix_as<FMT>(clip, first + i, channels);
}

// thread `lane` of the workgroup: mono-mix frames first + lane, first + lane + 256, ... into stage[0 .. count). The format is
// uniform over the workgroup, so it is dispatched once, outside the loop
MLA_RS_HD void stage_span_raw(int lane, const unsigned char* clip, int channels, int fmt, int64_t first, int count, float* stage) {
    switch (fmt) {
        case kU8: return stage_span_as<kU8>(lane, clip, channels, first, count, stage);
        case kI16: return stage_span_as<kI16>(lane, clip, channels, first, count, stage);
        case kI24: return stage_span_as<kI24>(lane, clip, channels, first, count, stage);
        case kI32: return stage_span_as<kI32>(lane, clip, channels, first, count, stage);
        case kF32: return stage_span_as<kF32>(lane, clip, channels, first, count, stage);
        default: return stage_span_as<kF64>(lane, clip, channels, first, count, stage);
    }
}

// ---- the workgroup body of the clips kernel ----
struct Clip {
    const unsigned char* src;  // first byte of the recording
    int64_t frames;
    int channels, format;
    double rate;
    const double* table;       // its filter table, nwin (win, delta) pairs
};

// Record of clip `c` of a batch. formats == nullptr: every clip has `uniform_format` and `offsets` count elements of it;
// otherwise `offsets` count bytes and the format is the clip's own.
MLA_RS_HD Clip clip_record(int64_t c, const unsigned char* packed, const int64_t* offsets, const int64_t* frames, const int32_t* channels,
                           const double* rates, const int32_t* table_index, const int32_t* formats, int uniform_format,
                           const double* tables, int nwin) {
    const int fmt = formats ? formats[c] : uniform_format;
    const int64_t off = formats ? offsets[c] : offsets[c] * sample_bytes(uniform_format);
    return Clip{packed + off, frames[c], channels[c], fmt, rates[c], tables + int64_t(table_index[c]) * 2 * nwin};
}

enum : int { kCopy, kZero, kFilter };

// What outputs [t0, t0 + 256) of a clip need; uniform over their workgroup.
struct TilePlan {
    int mode;                  // kCopy: the clip is at sr_out already (librosa does not resample an equal rate; the filter is no
                               // identity); kZero: the tile lies past the resampled clip; kFilter: stage [first, first + count)
    double ratio;
    int n_valid;               // outputs of the row that are resampled values: min(n_res, samples_num); zeros follow
    int index_step;
    int64_t first;
    int count;
};

MLA_RS_HD TilePlan plan_tile(const Clip& c, int t0, double sr_out, int samples_num, int nwin, int num_table) {
    TilePlan p{kCopy, 1.0, 0, 0, 0, 0};
    if (c.rate == sr_out) return p;
    p.ratio = sr_out / c.rate;
    const int64_t n_res = resampled_length(c.frames, p.ratio);
    p.n_valid = n_res < samples_num ? int(n_res) : samples_num;
    p.mode = kZero;
    if (t0 >= p.n_valid) return p;
    p.mode = kFilter;
    p.index_step = index_step_of(p.ratio, num_table);
    const int t_last = t0 + kThreads - 1 < p.n_valid - 1 ? t0 + kThreads - 1 : p.n_valid - 1;
    span(t0, t_last, p.ratio, wing_taps(nwin, p.index_step), c.frames, &p.first, &p.count);
    return p;
}

// out[t] of the row, t in the plan's tile; `stage` holds the plan's span (kFilter only)
MLA_RS_HD float tile_output(const Clip& c, const TilePlan& p, int t, const float* stage, int nwin, int num_table) {
    if (p.mode == kCopy) return t < c.frames ? mono_mix_raw(c.src, t, c.channels, c.format) : 0.f;
    if (p.mode != kFilter || t >= p.n_valid) return 0.f;
    return float(wings(setup(t, p.ratio, num_table), stage, p.first, c.frames, PairTable{c.table}, nwin, p.index_step));
}

}  // namespace resample_core
#endif
