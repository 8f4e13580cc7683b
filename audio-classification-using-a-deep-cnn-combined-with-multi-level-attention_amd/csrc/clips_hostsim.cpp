// clips_hostsim.cpp -- TEST HARNESS (never part of libmla_hip.so): runs clips_kernel's workgroup body on the host, workgroup by
// workgroup, with a plain array of `capacity` floats standing in for LDS. The body IS the kernel's: clip_record, plan_tile,
// stage_span_raw and tile_output of resample_core.h; only the order differs (all 256 lanes stage, then all 256 outputs, where
// the kernel has a barrier). Built with g++ -ffp-contract=off by tests/test_clips_cpu.py to check the span, staging and tap index
// arithmetic against the float64 restatement without a GPU. The stage array is refilled with NaN before every workgroup, so a
// tap read outside the staged span shows in the output.
#include <cmath>
#include <cstdint>
#include <vector>

#include "resample_core.h"

using namespace resample_core;

namespace {
// formats == nullptr: offsets in elements of `uniform_format`, as mla_clips_prepare launches; else bytes and a code per clip
int64_t run(const unsigned char* packed, int64_t clips, const int64_t* offsets, const int64_t* frames, const int32_t* channels,
            const int32_t* formats, int uniform_format, const double* rates, const int32_t* table_index, double sr_out, int64_t samples_num,
            const double* tables, int nwin, int num_table, float* out) {
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
        const Clip clip = clip_record(c, packed, offsets, frames, channels, rates, table_index, formats, uniform_format, tables, nwin);
        float* row = out + c * samples_num;
        for (int64_t tile = 0; tile < tiles; ++tile) {
            const int t0 = int(tile) * kThreads;
            const TilePlan p = plan_tile(clip, t0, sr_out, int(samples_num), nwin, num_table);
            if (p.mode == kFilter) {
                if (p.count > capacity) return -3;                 // the bound the launch sizes LDS from does not hold
                for (auto& v : stage) v = NAN;
                for (int lane = 0; lane < kThreads; ++lane)
                    stage_span_raw(lane, clip.src, clip.channels, clip.format, p.first, p.count, stage.data());
            }
            for (int t = t0; t < t0 + kThreads && t < samples_num; ++t) row[t] = tile_output(clip, p, t, stage.data(), nwin, num_table);
        }
    }
    return capacity;
}
}  // namespace

// Same arguments as the kernel (host arrays). pcm_dtype: 0 = float32, 2 = int16; offsets in elements. Returns the staged floats
// the launch would size LDS for, or a negative number: -1 bad descriptor, -2 unsupported rate, -3 a span exceeded span_capacity().
extern "C" int64_t hostsim_clips_prepare(const void* packed, int pcm_dtype, int64_t clips, const int64_t* offsets, const int64_t* frames,
                                         const int32_t* channels, const double* rates, const int32_t* table_index, double sr_out,
                                         int64_t samples_num, const double* tables, int nwin, int num_table, float* out) {
    if (pcm_dtype != kF32 && pcm_dtype != kI16) return -1;
    return run(static_cast<const unsigned char*>(packed), clips, offsets, frames, channels, nullptr, pcm_dtype, rates, table_index, sr_out,
               samples_num, tables, nwin, num_table, out);
}

// `packed` holds bytes, offsets are byte offsets, formats the MLA_* sample format codes (include/mla_hip.h).
// Returns as above; -1 also for an unknown format and for an offset that is no multiple of the clip's sample size.
extern "C" int64_t hostsim_clips_prepare_raw(const void* packed, int64_t clips, const int64_t* offsets, const int64_t* frames,
                                             const int32_t* channels, const int32_t* formats, const double* rates, const int32_t* table_index,
                                             double sr_out, int64_t samples_num, const double* tables, int nwin, int num_table, float* out) {
    for (int64_t c = 0; c < clips; ++c) {
        if (sample_bytes(formats[c]) == 0 || offsets[c] < 0 || offsets[c] % sample_align(formats[c]) != 0) return -1;
    }
    return run(static_cast<const unsigned char*>(packed), clips, offsets, frames, channels, formats, 0, rates, table_index, sr_out,
               samples_num, tables, nwin, num_table, out);
}
