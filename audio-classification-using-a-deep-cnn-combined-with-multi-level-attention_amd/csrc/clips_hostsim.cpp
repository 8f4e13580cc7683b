// clips_hostsim.cpp -- TEST HARNESS (never part of libmla_hip.so): runs resample_core.h on the host exactly as clips_kernel
// orders it, workgroup by workgroup (all 256 lanes stage, then all 256 lanes run their wings), with a plain array of
// `capacity` floats standing in for LDS. Built with g++ -ffp-contract=off by tests/test_clips_cpu.py to check the span, staging
// and tap index arithmetic against the float64 restatement without a GPU. The stage array is refilled with NaN before every
// workgroup, so a tap read outside the staged span shows in the output.
#include <cmath>
#include <cstdint>
#include <vector>

#include "resample_core.h"

using namespace resample_core;

namespace {
template <typename T>
int64_t run(const T* packed, int64_t clips, const int64_t* offsets, const int64_t* frames, const int32_t* channels, const double* rates,
            const int32_t* table_index, double sr_out, int64_t samples_num, const double* tables, int nwin, int num_table,
            double pcm_scale, float* out) {
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
        const int ch = channels[c];
        const T* src = packed + offsets[c];
        float* row = out + c * samples_num;
        for (int64_t tile = 0; tile < tiles; ++tile) {
            const int t0 = int(tile) * kThreads;
            if (rates[c] == sr_out) {
                for (int t = t0; t < t0 + kThreads && t < samples_num; ++t) row[t] = t < n_in ? mono_mix(src + int64_t(t) * ch, ch, pcm_scale) : 0.f;
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
            for (int lane = 0; lane < kThreads; ++lane) stage_span(lane, src, ch, pcm_scale, first, count, stage.data());
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
        return run(static_cast<const float*>(packed), clips, offsets, frames, channels, rates, table_index, sr_out, samples_num, tables, nwin,
                   num_table, 1.0, out);
    if (pcm_dtype == 2)
        return run(static_cast<const int16_t*>(packed), clips, offsets, frames, channels, rates, table_index, sr_out, samples_num, tables,
                   nwin, num_table, 1.0 / 32768.0, out);
    return -1;
}
