// clips_hostsim.cpp -- TEST HARNESS (never part of libmla_hip.so): runs resample_core.h on the host exactly as clips_kernel and
// clips_raw_kernel order it, workgroup by workgroup (all 256 lanes stage, then all 256 lanes run their wings), with a plain array of
// `capacity` floats standing in for LDS. Built with g++ -ffp-contract=off by tests/test_clips_cpu.py to check the span, staging
// and tap index arithmetic against the float64 restatement without a GPU. The stage array is refilled with NaN before every
// workgroup, so a tap read outside the staged span shows in the output. The two kernels differ in their source only: a Source
// gives the mono mix of one frame of a clip and stages a span of it, as the kernel's lanes do.
#include <cmath>
#include <cstdint>
#include <vector>

#include "resample_core.h"

using namespace resample_core;

namespace {
template <typename T>
struct TypedSource {                       // clips_kernel<T>: elements of T, offsets in elements
    const T* packed;
    const int64_t* offsets;
    const int32_t* channels;
    double pcm_scale;
    float mix(int64_t c, int64_t frame) const { return mono_mix(packed + offsets[c] + frame * channels[c], channels[c], pcm_scale); }
    void stage(int lane, int64_t c, int64_t first, int count, float* dst) const {
        stage_span(lane, packed + offsets[c], channels[c], pcm_scale, first, count, dst);
    }
};

struct RawSource {                         // clips_raw_kernel: bytes, offsets in bytes, a format code per clip
    const unsigned char* packed;
    const int64_t* offsets;
    const int32_t* channels;
    const int32_t* formats;
    float mix(int64_t c, int64_t frame) const { return mono_mix_raw(packed + offsets[c], frame, channels[c], formats[c]); }
    void stage(int lane, int64_t c, int64_t first, int count, float* dst) const {
        stage_span_raw(lane, packed + offsets[c], channels[c], formats[c], first, count, dst);
    }
};

template <typename Source>
int64_t run(const Source& source, int64_t clips, const int64_t* frames, const int32_t* channels, const double* rates,
            const int32_t* table_index, double sr_out, int64_t samples_num, const double* tables, int nwin, int num_table, float* out) {
    int64_t capacity = 0;
    for (int64_t c = 0; c < clips; ++c) {
        if (!(rates[c] > 0.0) || channels[c] < 1 || frames[c] < 0) return -1;
        if (rates[c] == sr_out) continue;
        const double ratio = sr_out / rates[c];
        const int step = index_step_of(ratio, num_table);
        if (step < 1 || rates[c] > kMaxRateFactor * sr_out) return -2;
        const int64_t cap = span_capacity(ratio, wing_taps(nwin, step));
        capacity = cap > capacity ? cap : capacity;
    }
    std::vector<float> stage(size_t(capacity) + 1);
    const int64_t tiles = (samples_num + kThreads - 1) / kThreads;
    for (int64_t c = 0; c < clips; ++c) {
        const int64_t n_in = frames[c];
        float* row = out + c * samples_num;
        for (int64_t tile = 0; tile < tiles; ++tile) {
            const int t0 = int(tile) * kThreads;
            if (rates[c] == sr_out) {
                for (int t = t0; t < t0 + kThreads && t < samples_num; ++t) row[t] = t < n_in ? source.mix(c, t) : 0.f;
                continue;
            }
            const double ratio = sr_out / rates[c];
            const int64_t n_res = resampled_length(n_in, ratio);
            const int n_valid = n_res < samples_num ? int(n_res) : int(samples_num);
            if (t0 >= n_valid) {
                for (int t = t0; t < t0 + kThreads && t < samples_num; ++t) row[t] = 0.f;
                continue;
            }
            const int index_step = index_step_of(ratio, num_table);
            const int t_last = t0 + kThreads - 1 < n_valid - 1 ? t0 + kThreads - 1 : n_valid - 1;
            int64_t first;
            int count;
            span(t0, t_last, ratio, wing_taps(nwin, index_step), n_in, &first, &count);
            if (count > capacity) return -3;                       // the bound the launch sizes LDS from does not hold
            for (auto& v : stage) v = NAN;
            for (int lane = 0; lane < kThreads; ++lane) source.stage(lane, c, first, count, stage.data());
            for (int t = t0; t < t0 + kThreads && t < samples_num; ++t) {
                float v = 0.f;
                if (t < n_valid) {
                    const Setup s = setup(t, ratio, num_table);
                    v = float(wings(s, stage.data(), first, n_in, tables + int64_t(table_index[c]) * 2 * nwin, nwin, index_step));
                }
                row[t] = v;
            }
        }
    }
    return capacity;
}
}  // namespace

// Same arguments as the kernel (host arrays). pcm_dtype: 0 = float32, 2 = int16. Returns the staged floats the launch would
// size LDS for, or a negative number: -1 bad descriptor, -2 unsupported rate, -3 a span exceeded span_capacity().
extern "C" int64_t hostsim_clips_prepare(const void* packed, int pcm_dtype, int64_t clips, const int64_t* offsets, const int64_t* frames,
                                         const int32_t* channels, const double* rates, const int32_t* table_index, double sr_out,
                                         int64_t samples_num, const double* tables, int nwin, int num_table, float* out) {
    if (pcm_dtype == 0)
        return run(TypedSource<float>{static_cast<const float*>(packed), offsets, channels, 1.0}, clips, frames, channels, rates, table_index,
                   sr_out, samples_num, tables, nwin, num_table, out);
    if (pcm_dtype == 2)
        return run(TypedSource<int16_t>{static_cast<const int16_t*>(packed), offsets, channels, 1.0 / 32768.0}, clips, frames, channels, rates,
                   table_index, sr_out, samples_num, tables, nwin, num_table, out);
    return -1;
}

// clips_raw_kernel: `packed` holds bytes, offsets are byte offsets, formats the MLA_* sample format codes (include/mla_hip.h).
// Returns as above; -1 also for an unknown format and for an offset that is no multiple of the clip's sample size.
extern "C" int64_t hostsim_clips_prepare_raw(const void* packed, int64_t clips, const int64_t* offsets, const int64_t* frames,
                                             const int32_t* channels, const int32_t* formats, const double* rates, const int32_t* table_index,
                                             double sr_out, int64_t samples_num, const double* tables, int nwin, int num_table, float* out) {
    for (int64_t c = 0; c < clips; ++c) {
        if (sample_bytes(formats[c]) == 0 || offsets[c] < 0 || offsets[c] % sample_align(formats[c]) != 0) return -1;
    }
    return run(RawSource{static_cast<const unsigned char*>(packed), offsets, channels, formats}, clips, frames, channels, rates, table_index,
               sr_out, samples_num, tables, nwin, num_table, out);
}
